"""lime_encoder_oproj_sp (csrc/oproj_sp_f32.hip) on a workgroup's THIRD trip through the persistent loop, and with a device count that
leaves workgroup 0's next tile entirely dead: the attention fragments of the next tile are requested unconditionally behind a tile's
last step, the residual rows of its first half before it.  Both with the gathered and with the dense residual, into a sentinel-filled,
wider output, against the fp64 statement and with the bounds of test_oproj_sp_gpu.py; bitwise repeatable."""
import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu
TIGHT = 2e-5                                   # test_oproj_sp_gpu.py's bounds
V = 500
E = 300
S = 128
EPS = 1e-5
SENTINEL = 7.0


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available()
    from lime_cikm25_amd import ops as _ops
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


_BUILT = {}


def case(ops, kind):
    """Inputs, the fp64 reference and lime_linear_f32's launch of the third-trip shape with one kind of residual: computed once,
    shared, never written to."""
    if kind in _BUILT:
        return _BUILT[kind]
    M = 128 * (2 * ops.device_cus() + 1) + 64
    seed = 1000 if kind == 'dense' else 2000
    c = dict(M=M)
    c['attn'] = rnd(M, E, seed=seed + 1).cuda()
    c['w'] = rnd(E, E, seed=seed + 2, scale=E ** -0.5).cuda()
    c['b'] = rnd(E, seed=seed + 3, scale=0.1).cuda()
    c['g'] = (1 + rnd(E, seed=seed + 4, scale=0.2)).cuda()
    c['be'] = rnd(E, seed=seed + 5, scale=0.1).cuda()
    if kind == 'dense':
        c['res'] = dict(res=rnd(M, E, seed=seed + 6).cuda())
        res64 = c['res']['res'].double().cpu()
    else:
        table, pe = rnd(V, E, seed=seed + 6).cuda(), rnd(S, E, seed=seed + 7, scale=0.5).cuda()
        ids = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(seed + 8), dtype=torch.int32).cuda()
        c['res'] = dict(res=table, res_ids=ids, res_pe=pe, res_period=S)
        res64 = table.double().cpu()[ids.cpu().long()] + pe.double().cpu()[torch.arange(M) % S]
    d = lambda t: t.double().cpu()
    c['want'] = torch.nn.functional.layer_norm(res64 + d(c['attn']) @ d(c['w']).T + d(c['b']), (E,), d(c['g']), d(c['be']), EPS)
    c['fp32'] = ops.linear(c['attn'], c['w'], c['b'], ln=(c['g'], c['be']), ln_eps=EPS, **c['res']).cpu()
    c['wp'] = ops.oproj_pack_sp(c['w'])
    _BUILT[kind] = c
    return c


def run(ops, c, m_dev=None):
    big = torch.full((c['M'], E + 4), SENTINEL, device='cuda')
    dev = None if m_dev is None else torch.tensor([m_dev], dtype=torch.int32, device='cuda')
    ops.encoder_oproj_sp(c['attn'], c['wp'], c['b'], (c['g'], c['be']), EPS, m_dev=dev, out=big[:, :E], **c['res'])
    torch.cuda.synchronize()
    return big


@pytest.mark.parametrize('kind', ['gathered', 'dense'])
def test_third_trip_and_dead_next_tile(ops, kind):
    c = case(ops, kind)
    M, cu = c['M'], ops.device_cus()
    e_fp32 = rel_err(c['fp32'], c['want'])
    for m in (None, 128 * cu - 5):
        big = run(ops, c, m_dev=m).cpu()
        rows = M if m is None else m
        assert (big[:, E:] == SENTINEL).all(), (kind, m)               # nothing written behind the E columns
        assert (big[rows:, :E] == SENTINEL).all(), (kind, m)           # rows at or beyond the device count untouched
        got = big[:rows, :E]
        assert torch.isfinite(got).all(), (kind, m)
        e_got = rel_err(got, c['want'][:rows])
        print('%s m_dev=%s: error %.3g (lime_linear_f32: %.3g)' % (kind, m, e_got, e_fp32))
        assert e_got < TIGHT, (kind, m, e_got, e_fp32)
        assert e_got <= 4 * e_fp32 + 2e-6, (kind, m, e_got, e_fp32)


@pytest.mark.parametrize('kind', ['gathered', 'dense'])
def test_bitwise_repeatable(ops, kind):
    c = case(ops, kind)
    assert torch.equal(run(ops, c), run(ops, c))
    m = 128 * ops.device_cus() - 5
    assert torch.equal(run(ops, c, m_dev=m), run(ops, c, m_dev=m))
