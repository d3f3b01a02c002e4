"""lime_encoder_ffn_sp (csrc/ffn_sp_f32.hip): the fp32 feed-forward half of an encoder layer -- linear1, ReLU, linear2, residual,
LayerNorm, optionally the 32-token block means -- in one split-product launch, against an fp64 torch-CPU statement of the same
operation and beside the two-launch lime_linear_f32 path (split-product GEMMs) on the same inputs."""
import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu
TIGHT = 2e-5                                   # test_split_gemm_gpu.py's tolerance for the split-product GEMMs
E = 300


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available()
    from lime_cikm25_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def _restore(ops):
    prev = ops.set_split_gemm(True, force=True)        # the two-launch reference on the split kernel at every shape below
    yield
    ops.set_split_gemm(prev)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def layer(F, seed=1):
    w1 = rnd(F, E, seed=seed, scale=E ** -0.5)
    b1 = rnd(F, seed=seed + 1, scale=0.1)
    w2 = rnd(E, F, seed=seed + 2, scale=F ** -0.5)
    b2 = rnd(E, seed=seed + 3, scale=0.1)
    g = 1 + rnd(E, seed=seed + 4, scale=0.2)
    be = rnd(E, seed=seed + 5, scale=0.1)
    return [t.cuda() for t in (w1, b1, w2, b2, g, be)]


def ref64(x, w1, b1, w2, b2, g, be, eps=1e-5, pool32=False):
    d = lambda t: t.double().cpu()
    x = d(x)
    h = torch.relu(x @ d(w1).T + d(b1))
    y = torch.nn.functional.layer_norm(x + h @ d(w2).T + d(b2), (E,), d(g), d(be), eps)
    return y.reshape(-1, 32, E).mean(1) if pool32 else y


def fused(ops, x, w, pool32=False, m_dev=None, out=None):
    w1, b1, w2, b2, g, be = w
    w1p, w2p = ops.ffn_pack_sp(w1, w2)
    return ops.encoder_ffn_sp(x, w1p, w2p, b1, b2, (g, be), 1e-5, pool32=pool32, m_dev=m_dev, out=out)


def two_launch(ops, x, w, pool32=False):
    w1, b1, w2, b2, g, be = w
    h = ops.linear(x, w1, b1, act='relu')
    return ops.linear(h, w2, b2, res=x, ln=(g, be), ln_eps=1e-5, pool32=pool32)


@pytest.mark.parametrize('F', [512, 1024])
@pytest.mark.parametrize('pool32', [False, True])
def test_matches_fp64_and_two_launch_path(ops, F, pool32):
    M = 4096 + 96                                  # not a multiple of the 128-row tile
    x = rnd(M, E, seed=7).cuda()
    w = layer(F)
    got = fused(ops, x, w, pool32=pool32)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    want = ref64(x, *w, pool32=pool32)
    two = two_launch(ops, x, w, pool32=pool32).cpu()
    e_got, e_two = rel_err(got.cpu(), want), rel_err(two, want)
    assert e_got < TIGHT, (e_got, e_two)
    assert e_got <= 4 * e_two + 2e-6, (e_got, e_two)


def test_strided_out_and_small_m(ops):
    M = 200
    x = rnd(M, E, seed=9).cuda()
    w = layer(512, seed=3)
    big = torch.full((M, 320), 7.0, device='cuda')
    out = big[:, :E]
    ops.encoder_ffn_sp(x, *ops.ffn_pack_sp(w[0], w[2]), w[1], w[3], (w[4], w[5]), 1e-5, out=out)
    torch.cuda.synchronize()
    assert rel_err(out.cpu(), ref64(x, *w)) < TIGHT
    assert (big[:, E:] == 7.0).all()               # nothing written behind the E columns


@pytest.mark.parametrize('pool32', [False, True])
def test_device_row_count(ops, pool32):
    M = 1024
    x = rnd(M, E, seed=11).cuda()
    w = layer(512, seed=5)
    want = ref64(x, *w, pool32=pool32)
    for m in (0, 64, 160, 1024):
        rows = m // 32 if pool32 else m
        out = torch.full((M // 32 if pool32 else M, E), 3.0, device='cuda')
        fused(ops, x, w, pool32=pool32, m_dev=torch.tensor([m], dtype=torch.int32, device='cuda'), out=out)
        torch.cuda.synchronize()
        o = out.cpu()
        if rows:
            assert rel_err(o[:rows], want[:rows]) < TIGHT, m
        assert (o[rows:] == 3.0).all(), m          # rows beyond the device count untouched


def test_bitwise_repeatable(ops):
    M = 4096
    x = rnd(M, E, seed=13).cuda()
    w = layer(512, seed=7)
    a = fused(ops, x, w, pool32=True).clone()
    b = fused(ops, x, w, pool32=True).clone()
    c = fused(ops, x, w).clone()
    d = fused(ops, x, w).clone()
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(c, d)


def test_graph_replay_sees_weight_updates(ops):
    """The pack runs inside the captured step: weights changed in place between replays reach the kernel."""
    M = 4096
    x = rnd(M, E, seed=15).cuda()
    w = layer(512, seed=9)
    out = torch.empty((M // 32, E), device='cuda')
    fused(ops, x, w, pool32=True, out=out)          # warm up (library load, lazy state) outside the capture
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            fused(ops, x, w, pool32=True, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert rel_err(out.cpu(), ref64(x, *w, pool32=True)) < TIGHT
    with torch.no_grad():
        w[0].mul_(-0.5)
        w[2].add_(0.01)
        w[1].mul_(2.0)
    g.replay()
    torch.cuda.synchronize()
    assert rel_err(out.cpu(), ref64(x, *w, pool32=True)) < TIGHT


def test_unsupported_shapes_are_refused(ops):
    x = rnd(256, E).cuda()
    w1 = rnd(200, E).cuda()                        # F not a multiple of 128
    w2 = rnd(E, 200).cuda()
    with pytest.raises(Exception):
        ops.ffn_pack_sp(w1, w2)
