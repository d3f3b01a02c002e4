"""Host side of lime_encoder_oproj_sp without a GPU: the applicability rule as a pure function and the staleness rule's sources.
(The pack layout is read back from the device: tests/test_oproj_sp_gpu.py; the args struct against the header: tests/test_abi.py.)"""
import os
import subprocess
import sys

from lime_cikm25_amd import make_config, newsEncoders

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rule():
    rule = newsEncoders.oproj_sp_rule
    ok = dict(on=True, split_on=True, M=117760, E=300, has_bias=True, aligned=True)
    assert rule(**ok)
    assert rule(**dict(ok, M=29500))                       # the title launch of the flagship batch: 231 tiles
    assert not rule(**dict(ok, on=False))                  # LIME_SP_OPROJ=0
    assert not rule(**dict(ok, split_on=False))            # the split GEMM switched off
    assert not rule(**dict(ok, has_bias=False))
    assert not rule(**dict(ok, aligned=False))
    for E, want in ((304, True), (64, True), (4, True), (308, False), (302, False), (0, False)):
        assert rule(**dict(ok, E=E)) is want, E
    # 160 tiles of 128 rows: the last row count below, the first at the threshold
    assert not rule(**dict(ok, M=159 * 128)) and rule(**dict(ok, M=159 * 128 + 1))
    assert not rule(**dict(ok, M=4095)) and not rule(**dict(ok, M=4096))
    assert not rule(**dict(ok, M=0))


def test_switch_is_read_from_the_environment():
    assert newsEncoders.SP_OPROJ is (os.environ.get('LIME_SP_OPROJ', '1') != '0')
    code = 'from lime_cikm25_amd import newsEncoders; print(newsEncoders.SP_OPROJ)'
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=dict(os.environ, LIME_SP_OPROJ='0'), check=True,
                         capture_output=True, text=True).stdout
    assert out.strip() == 'False'


def test_out_proj_weights_are_sources_of_the_weight_products():
    """An edit of Wo must make the kept pack stale: every layer's out_proj weight is among the tensors the state is taken over."""
    enc = newsEncoders.CROWN(make_config(vocabulary_size=50))
    src = [t.data_ptr() for t in enc._product_sources()]
    for tr in (enc.title_transformer, enc.body_transformer):
        for layer in tr.layers:
            assert layer.self_attn.out_proj.weight.data_ptr() in src
