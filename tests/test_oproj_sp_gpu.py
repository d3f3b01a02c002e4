"""lime_encoder_oproj_sp (csrc/oproj_sp_f32.hip): out_proj + residual + norm1 of an fp32 encoder layer in one split-product launch,
against an fp64 torch-CPU statement of LayerNorm(res + attn Wo^T + bo) and beside today's lime_linear_f32 launch on the same inputs.

Shapes: the smallest that reach every branch of the kernel -- full tiles only, a second trip through the persistent loop with a
partly dead last tile (the CU count is the library's own), a residual period that divides no tile, the dense residual, and a second E
inside the build (quads beyond E).  Every case runs with the device counts M, M - 3 and 0 into a sentinel-filled, wider output."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu
TIGHT = 2e-5                                   # the project's split-product bound (test_ffn_sp_gpu.py, test_split_gemm_gpu.py)
V = 500
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


def n_cu(ops):
    return ops.device_cus()


CASES = {       # name: (M or a function of the CU count, S or None for the dense residual, E)
    'full_tiles': (4224, 32, 300),
    'second_trip': (lambda cu: 128 * (cu + 1) + 37, 128, 300),
    'period_7': (5000, 7, 300),
    'dense': (4200, None, 300),
    'e64': (4100, 5, 64),
}
_BUILT = {}


def case(ops, name):
    """Inputs, the fp64 reference and today's launch of one case: computed once, shared, never written to."""
    if name in _BUILT:
        return _BUILT[name]
    M, S, E = CASES[name]
    M = M(n_cu(ops)) if callable(M) else M
    seed = 100 * sorted(CASES).index(name)
    c = dict(M=M, S=S, E=E)
    c['attn'] = rnd(M, E, seed=seed + 1).cuda()
    c['w'] = rnd(E, E, seed=seed + 2, scale=E ** -0.5).cuda()
    c['b'] = rnd(E, seed=seed + 3, scale=0.1).cuda()
    c['g'] = (1 + rnd(E, seed=seed + 4, scale=0.2)).cuda()
    c['be'] = rnd(E, seed=seed + 5, scale=0.1).cuda()
    if S is None:
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
    _BUILT[name] = c
    return c


def run(ops, c, m_dev=None, ldo=None):
    """The launch into a sentinel-filled [M, ldo] buffer; returns the whole buffer."""
    big = torch.full((c['M'], ldo or c['E'] + 4), SENTINEL, device='cuda')
    dev = None if m_dev is None else torch.tensor([m_dev], dtype=torch.int32, device='cuda')
    ops.encoder_oproj_sp(c['attn'], c['wp'], c['b'], (c['g'], c['be']), EPS, m_dev=dev, out=big[:, :c['E']], **c['res'])
    torch.cuda.synchronize()
    return big


@pytest.mark.parametrize('name', sorted(CASES))
def test_matches_fp64_and_the_fp32_launch(ops, name):
    c = case(ops, name)
    M, E = c['M'], c['E']
    e_fp32 = rel_err(c['fp32'], c['want'])
    for m in (None, M - 3, 0):
        big = run(ops, c, m_dev=m).cpu()
        rows = M if m is None else m
        assert (big[:, E:] == SENTINEL).all(), (name, m)             # nothing written behind the E columns
        assert (big[rows:, :E] == SENTINEL).all(), (name, m)         # rows at or beyond the device count untouched
        if rows:
            got = big[:rows, :E]
            assert torch.isfinite(got).all(), (name, m)
            e_got = rel_err(got, c['want'][:rows])
            print('%s m_dev=%s: error %.3g (lime_linear_f32: %.3g)' % (name, m, e_got, e_fp32))
            assert e_got < TIGHT, (name, m, e_got, e_fp32)
            assert e_got <= 4 * e_fp32 + 2e-6, (name, m, e_got, e_fp32)


@pytest.mark.parametrize('name', ['second_trip', 'dense'])
def test_bitwise_repeatable(ops, name):
    c = case(ops, name)
    assert torch.equal(run(ops, c), run(ops, c))


def test_rows_do_not_depend_on_tile_or_launch(ops):
    """A 128-row block computed alone (M = 128) is bitwise what the same rows are at tile 1 and at tile n_cu (the second trip of
    workgroup 0) of a large launch, with and without a smaller device count."""
    c = case(ops, 'second_trip')
    cu, E, S = n_cu(ops), c['E'], c['S']
    whole = run(ops, c)[:, :E]
    fewer = run(ops, c, m_dev=128 * (cu + 1) + 5)[:, :E]
    for tile in (1, cu):
        r0 = 128 * tile
        assert r0 % S == 0                                           # the block starts a period: pe[r % S] lines up
        alone = torch.full((128, E + 4), SENTINEL, device='cuda')
        res = dict(c['res'], res_ids=c['res']['res_ids'][r0:r0 + 128].contiguous())
        ops.encoder_oproj_sp(c['attn'][r0:r0 + 128], c['wp'], c['b'], (c['g'], c['be']), EPS, out=alone[:, :E], **res)
        torch.cuda.synchronize()
        assert torch.equal(alone[:, :E], whole[r0:r0 + 128]), tile
        assert torch.equal(alone[:, :E], fewer[r0:r0 + 128]), tile
    d = case(ops, 'dense')
    whole = run(ops, d)[:, :E]
    alone = torch.empty((128, E), device='cuda')
    ops.encoder_oproj_sp(d['attn'][128:256], d['wp'], d['b'], (d['g'], d['be']), EPS, res=d['res']['res'][128:256], out=alone)
    torch.cuda.synchronize()
    assert torch.equal(alone, whole[128:256])


def _swz4(q):
    return (0x78 >> (2 * q)) & 3


def _bf16_rne(x):
    """float32 array -> (the bf16 bit patterns, their float32 values), round to nearest even."""
    bits = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    r = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint32)
    return r.astype(np.uint16), (r << 16).astype(np.uint32).view(np.float32)


@pytest.mark.parametrize('E', [300, 64])
def test_pack_layout(ops, E):
    """[10 chunks][3 terms][304 rows][32] bf16: hi / mid / lo of split_pair's rounding, logical 16-byte segment kg of row n at
    physical kg ^ swz4((n >> 2) & 3), zeros for rows and k beyond E."""
    w = rnd(E, E, seed=5, scale=E ** -0.5)
    got = ops.oproj_pack_sp(w.cuda()).view(torch.int16).cpu().numpy().view(np.uint16).reshape(10, 3, 304, 32)
    full = np.zeros((304, 320), dtype=np.float32)
    full[:E, :E] = w.numpy()
    hb, hv = _bf16_rne(full)
    r1 = full - hv
    mb, mv = _bf16_rne(r1)
    lb, _ = _bf16_rne(r1 - mv)
    want = np.zeros((10, 3, 304, 32), dtype=np.uint16)
    n = np.arange(304)[:, None]
    pk = np.arange(32)[None, :]
    swz = np.array([_swz4(q) for q in range(4)])[(n >> 2) & 3]
    for c in range(10):
        k = 32 * c + 8 * ((pk >> 3) ^ swz) + (pk & 7)
        for t, img in enumerate((hb, mb, lb)):
            want[c, t] = img[n, k]
    assert np.array_equal(got, want)
    assert not got[:, :, E:].any() and got.any()


def test_bad_arguments_are_refused_without_a_launch(ops):
    from lime_cikm25_amd import _lib
    lib = _lib.load()
    c = case(ops, 'dense')
    M, E = 256, c['E']
    out = torch.full((M, E), SENTINEL, device='cuda')
    flat = torch.zeros(M * E + 4, device='cuda')

    def args(**kw):
        a = _lib.OprojSpArgs()
        a.attn, a.lda = c['attn'].data_ptr(), E
        a.wp, a.bias = c['wp'].data_ptr(), c['b'].data_ptr()
        a.res, a.ldr = c['res']['res'].data_ptr(), E
        a.ln_gamma, a.ln_beta, a.ln_eps = c['g'].data_ptr(), c['be'].data_ptr(), EPS
        a.out, a.ldo = out.data_ptr(), E
        a.M, a.E = M, E
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    call = lambda a: lib.lime_encoder_oproj_sp(ctypes.byref(a), None)
    assert lib.lime_encoder_oproj_sp(None, None) == -1
    assert call(args(attn=None)) == -1 and b'NULL' in lib.lime_last_error_string()
    assert call(args(wp=None)) == -1 and call(args(res=None)) == -1 and call(args(out=None)) == -1
    assert call(args(attn=flat.data_ptr() + 4)) == -1                # misaligned pointer
    assert call(args(res=flat.data_ptr() + 4)) == -1
    assert call(args(lda=E + 1)) == -1 and call(args(ldo=E + 2)) == -1
    assert call(args(res_pe=c['g'].data_ptr())) == -1                # positional rows without ids
    assert call(args(E=302)) == -2 and call(args(E=308)) == -2
    assert lib.lime_oproj_pack_sp(None, E, E, None, None) == -1
    assert lib.lime_oproj_pack_sp(c['w'].data_ptr(), E, 302, c['wp'].data_ptr(), None) == -2
    assert lib.lime_oproj_pack_sp_size() == 10 * 3 * 304 * 32
    assert call(args(M=0)) == 0
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()                                   # none of them launched anything
