"""Every kernel that draws the dropout mask of csrc/dropout.h, at every branch of its index arithmetic, against the host statement of
the mask (tests/dropout_cases.py, itself pinned by tests/test_dropout_reference_cpu.py) -- never a mask read back from the GPU.

Bounds are the project's own for the same kernels without dropout: forward results and rstd 5e-5 against fp64 (TIGHT of
test_backward_gpu.py), the GEMM epilogue 2e-5 (TIGHT of test_split_gemm_gpu.py), gradients 2e-4 against fp64 autograd (BWD).  Where
an output element is one multiplication of an input the comparison is bitwise: where(keep, fl32(x * scale), 0) with |x| in [0.5, 1.5],
so an output is zero iff the element was dropped.  Each comparison prints its figure on a line that starts with 'PIN'.

Worst figures observed on the MI355X (no case needed a bound of its own; the whole file runs in about 5 s):

  kernel branch                                     reached by                                    worst error (bound)
  dropout_vec4_kernel                               (37, 300) ld 308 / 304, in place              bitwise
  dropout_kernel (by shape / by alignment)          (37, 50), (33, 33); (37, 300) off 1 ld 301    bitwise
  second grid-stride sweep, scalar / vec4           (8200, 513) / (32800, 512)                    bitwise
  p = 0 / 0.1 / 0.5, wrapping seed and site         (37, 300)                                     bitwise
  read-back shapes of the other suites              (48, 300) (48, 512) (20 S, S) (64, 50)        bitwise
  dropout2_vec4_kernel / two-pass fallback          (37, 300) / (37, 50)                          bitwise
  embed_pe_dropout_vec4_kernel                      48 x 300, period 16, ld_table 308, no pe      1.5e-7 (5e-5), zero pattern exact
  embed_pe_dropout_kernel                           dim 50; dim 300 ld_pe 301; no pe              1.5e-7 (5e-5), zero pattern exact
  dropout_add_ln_vec_kernel<2 / 5 / 8>              E 100 / 300 / 400, 512, ld E + 4              y 4.1e-7, rstd 1.2e-7 (5e-5)
  dropout_add_ln_kernel<2 / 5 / 8>                  E 50 / 301 / 450; E 300 ld 301                y 3.3e-7, rstd 1.2e-7 (5e-5)
  second persistent sweep, vec / scalar             M 32789 at E 100 / E 50                       y 4.9e-7, rstd 1.7e-7 (5e-5)
  layernorm_bwd_vec_kernel<2 / 5 / 8> + dropout     E 100 / 300 / 400, dy_div 1 / 16, lddd E + 4  dz 2.1e-7, dgamma 4.0e-7, dzsum 3.9e-7 (2e-4), dz_drop bitwise
  its second persistent sweep                       M 12309, E 100                                dz 2.2e-7, dzsum 7.4e-7 (2e-4), dz_drop bitwise
  ops.layernorm_bwd fallback                        E 50 (the C entry returns UNSUPPORTED)        dz 2.1e-7 (2e-4), dz_drop bitwise
  linear: fused split-product ReLU epilogue         M 4096 N 512 K 64                             1.2e-6 (2e-5)
  linear: second pass (M 4000, act none, M 300)     N 512                                         1.2e-6 (2e-5)
  linear: scalar second pass                        M 300 N 50                                    9.1e-7 (2e-5)
  attention forward, split product                  S 32 / 64 / 128, hd 30 / 32                   1.1e-6 (5e-5)
  token_attn_fwd_dropout_kernel<32 / 64 / 128>      S 7 .. 128, hs 32 and packed hd 20            6.1e-7 / 1.3e-6 / 1.3e-6 (5e-5)
  attn_fwd_long_dropout_kernel                      S 129 / 131 / 256 / 300, split on and off     2.4e-6 (5e-5)
  wide-head forward                                 S 33 / 64 / 65 / 130, hd 36 / 100             1.6e-6 (5e-5)
  token_attn_bwd_kernel (one pass, fp32)            S 31 / 33 / 65 / 127                          2.2e-6 (2e-4)
  split-product one-pass backward (phase A and B)   S 68 / 100 / 128                              1.9e-6 (2e-4)
  attn_bwd_long_kernel / attn_bwd_long_sp_kernel    S 129 / 131 / 300                             3.6e-6 / 4.3e-6 (2e-4)
  wide-head backward                                S 33 / 130, hd 36 / 100                       2.2e-6 (2e-4)
  cand_attn_train_kernel, forward / backward        the five shapes of dropout_cases.CAND_CASES   agg 1.5e-7 (5e-5), dqp 3.3e-6, dkp 4.4e-6 (2e-4)"""
import ctypes
import math

import numpy as np
import pytest
import torch

import dropout_cases as dc
import linear_route_cases
from helpers import rel_err

pytestmark = pytest.mark.gpu

P, TIGHT, GEMM_TIGHT, BWD = dc.P, dc.TIGHT, dc.GEMM_TIGHT, dc.BWD
PAIRS = dc.SEED_SITES
LIME_ERR_UNSUPPORTED = -2


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from lime_cikm25_amd import ops as _ops
    from lime_cikm25_amd import _lib
    _lib.load()
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def mag(*shape, seed=0):
    """|x| in [0.5, 1.5], random sign: never zero, never denormal after one multiplication."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) + 0.5) * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def view(t, ld=None, off=0, fill=0.0):
    """A CUDA view holding t with leading dimension ld, starting `off` floats into a 16-byte aligned buffer -> (view, buffer)."""
    rows, cols = t.shape
    ld = cols if ld is None else ld
    buf = torch.full((rows * ld + off + 8,), fill, dtype=torch.float32, device='cuda')
    v = buf.as_strided((rows, cols), (ld, 1), off)
    v.copy_(t)
    return v, buf


def close(got, want, tol, what):
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape), (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what
    e = rel_err(got.numpy(), want.detach().numpy())
    print('PIN %s: rel err %.3e (bound %.1e)' % (what, e, tol))
    assert e <= tol, '%s: rel err %.3e > %.1e' % (what, e, tol)
    return e


def bitwise(got, want, what):
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = int((got != want).sum())
    print('PIN %s: bitwise, %d of %d elements differ' % (what, bad, got.size))
    assert bad == 0, '%s: %d of %d elements differ from the host statement' % (what, bad, got.size)


def keep2d(p, seed, site, rows, cols):
    return dc.keep_mask(p, seed, site, rows * cols).reshape(rows, cols)


# ---------------------------------------------------------------------------------------------------
# a. lime_dropout_f32
# ---------------------------------------------------------------------------------------------------
# (id, rows, cols, lds, ldd, off, in place, (seed, site) pairs)
DROPOUT_CASES = [
    ('vec4', 37, 300, 308, 304, 0, False, PAIRS),
    ('vec4-inplace', 37, 300, 308, 308, 0, True, PAIRS[:1]),
    ('scalar-cols50', 37, 50, 50, 50, 0, False, PAIRS),
    ('scalar-cols33', 33, 33, 33, 33, 0, False, PAIRS[:1]),
    ('scalar-unaligned-ld301', 37, 300, 301, 301, 1, False, PAIRS),
    ('scalar-second-sweep', 8200, 513, 513, 513, 0, False, PAIRS[1:2]),      # 8200 * 513 > 16384 * 256 threads
    ('vec4-second-sweep', 32800, 512, 512, 512, 0, False, PAIRS[1:2]),        # 32800 * 128 > 16384 * 256 threads
]


@pytest.mark.parametrize('case', DROPOUT_CASES, ids=[c[0] for c in DROPOUT_CASES])
def test_dropout(ops, case):
    name, rows, cols, lds, ldd, off, inplace, pairs = case
    x = mag(rows, cols, seed=rows + cols)
    for seed, site in pairs:
        src, sbuf = view(x, lds, off)
        dst, dbuf = (src, sbuf) if inplace else view(torch.zeros(rows, cols), ldd, off, fill=-7.0)
        ops.dropout(src, P, seed, site, out=dst)
        keep = keep2d(P, seed, site, rows, cols)
        bitwise(dst, dc.dropped_f32(x.numpy(), keep, P), 'dropout %s seed %d site %d' % (name, seed, site))
        assert np.array_equal(dst.cpu().numpy() == 0, ~keep)
        if not inplace and ldd > cols:                                           # nothing outside the [rows, cols] window is written
            rest = dbuf.clone()
            rest.as_strided((rows, cols), (ldd, 1), off).fill_(-7.0)
            assert bool((rest == -7.0).all()), 'wrote outside the result'


@pytest.mark.parametrize('p', [0.0, 0.1, 0.5])
def test_dropout_rates(ops, p):
    rows, cols = 37, 300
    x = mag(rows, cols, seed=3)
    for seed, site in PAIRS[:2]:
        got = ops.dropout(x.cuda(), p, seed, site)
        bitwise(got, dc.dropped_f32(x.numpy(), keep2d(p, seed, site, rows, cols), p), 'dropout p=%g' % p)
    if p == 0.0:
        assert torch.equal(got.cpu(), x)                                         # the identity


def test_dropout_wrapping_seed_and_site(ops):
    """Seed 2^63 + 5 and site 0xFFFFFFFF (site + 1 wraps to 0 in 32 bits) through the ctypes binding."""
    rows, cols = 37, 300
    x = mag(rows, cols, seed=4)
    for seed, site in (((1 << 63) + 5, 0xFFFFFFFF), ((1 << 64) - 1, 3), (5, 0xFFFFFFFF)):
        got = ops.dropout(x.cuda(), P, seed, site)
        bitwise(got, dc.dropped_f32(x.numpy(), keep2d(P, seed, site, rows, cols), P), 'dropout seed %d site %d' % (seed, site))


READ_BACK = [(48, 300), (48, 512), (2 * 10 * 16, 16), (2 * 10 * 50, 50), (2 * 10 * 200, 200), (64, 50)]


@pytest.mark.parametrize('rows,cols', READ_BACK)
def test_read_back_masks_of_the_other_suites(ops, rows, cols):
    """test_dropout_gpu.py, test_wide_heads_gpu.py, test_backward_gpu.py, the content-encoder suites and
    test_workspace_contract_gpu.py read their masks back as ops.dropout(ones): (tok, 300) / (tok, 512) for the layer sites,
    (M * nh * S, S) for the attention site, (M, 50) -- each is bitwise keep_mask * scale."""
    ones = torch.ones(rows, cols, device='cuda')
    for seed, site in PAIRS:
        want = dc.dropped_f32(np.ones((rows, cols), np.float32), keep2d(P, seed, site, rows, cols), P)
        bitwise(ops.dropout(ones, P, seed, site), want, 'read-back (%d, %d) site %d' % (rows, cols, site))


# ---------------------------------------------------------------------------------------------------
# b. lime_dropout2_f32
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,cols,what', [(37, 300, 'fused'), (37, 50, 'two-pass')])
def test_dropout2(ops, rows, cols, what):
    x = mag(rows, cols, seed=5)
    for seed, _ in PAIRS[:2]:
        s1, s2 = 1, 0
        keep = keep2d(P, seed, s1, rows, cols) & keep2d(P, seed, s2, rows, cols)
        got = ops.dropout2(x.cuda(), P, seed, s1, s2)
        bitwise(got, dc.dropped_f32(x.numpy(), keep, P, times=2), 'dropout2 %s seed %d' % (what, seed))


# ---------------------------------------------------------------------------------------------------
# c. lime_embed_pe_dropout_f32
# ---------------------------------------------------------------------------------------------------
# (id, dim, ld_table, ld_pe (None: no pe))
EMBED_CASES = [('vec4', 300, 300, 300), ('vec4-ldtable', 300, 308, 304), ('vec4-nope', 300, 300, None), ('scalar-dim50', 50, 50, 50),
               ('scalar-dim50-ldtable', 50, 53, 51), ('scalar-ldpe301', 300, 300, 301), ('scalar-nope', 50, 50, None)]


@pytest.mark.parametrize('case', EMBED_CASES, ids=[c[0] for c in EMBED_CASES])
def test_embed_pe_dropout(ops, case):
    name, dim, ld_table, ld_pe = case
    rows, period, V = 48, 16, 20                                                 # 48 rows over 20 ids: repeated ids
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, V, (rows,), generator=g, dtype=torch.int32)
    assert ids.unique().numel() < rows
    table = mag(V, dim, seed=12)
    pe = None if ld_pe is None else mag(period, dim, seed=13) * 0.1              # |pe| <= 0.15 < 0.5 * scale: drop(t) + pe is never zero
    site_emb, site_pe = 0, 1
    for seed, _ in PAIRS[:2]:
        got = ops.embed_pe_dropout(ids.cuda(), view(table, ld_table)[0], None if pe is None else view(pe, ld_pe)[0], period, P, seed,
                                   site_emb, site_pe)
        k_emb, k_pe = keep2d(P, seed, site_emb, rows, dim), keep2d(P, seed, site_pe, rows, dim)
        zero = got.cpu().numpy() == 0
        assert np.array_equal(zero, ~k_pe if pe is not None else ~(k_pe & k_emb)), 'the zero pattern is not the site_pe mask'
        s = float(dc.scale(P))
        want = dc.embed_pe_dropout_ref(table, ids, pe, period, torch.from_numpy(k_emb * s), torch.from_numpy(k_pe * s))
        close(got, want, TIGHT, 'embed_pe_dropout %s seed %d' % (name, seed))


# ---------------------------------------------------------------------------------------------------
# d. lime_dropout_add_layernorm_f32
# ---------------------------------------------------------------------------------------------------
# (id, M, E, ld of t and res)
DALN_CASES = [('vec-V2', 37, 100, 104), ('vec-V5', 37, 300, 304), ('vec-V8-E400', 37, 400, 404), ('vec-V8-E512', 37, 512, 516),
              ('scalar-CPL2', 37, 50, 50), ('scalar-CPL2-ld', 37, 50, 51), ('scalar-CPL5', 37, 301, 301), ('scalar-CPL8', 37, 450, 450),
              ('scalar-ld301', 37, 300, 301),
              ('vec-second-sweep', 32789, 100, 100),            # 2048 workgroups * 16 rows per sweep
              ('scalar-second-sweep', 32789, 50, 50)]           # 8192 workgroups * 4 rows per sweep


@pytest.mark.parametrize('case', DALN_CASES, ids=[c[0] for c in DALN_CASES])
def test_dropout_add_layernorm(ops, case):
    name, M, E, ld = case
    t, res = rnd(M, E, seed=21), rnd(M, E, seed=22)
    gamma, beta = rnd(E, seed=23) * 0.5 + 1.0, rnd(E, seed=24)
    tv, rv = view(t, ld)[0], view(res, ld)[0]
    for seed, site in (PAIRS[:2] if M < 1000 else PAIRS[1:2]):
        y, rstd = ops.dropout_add_layernorm(tv, rv, gamma.cuda(), beta.cuda(), 1e-5, P, seed, site)
        want_y, want_rstd = dc.dropout_add_ln_ref(t, res, gamma, beta, 1e-5, dc.multiplier(P, seed, site, (M, E)))
        close(y, want_y, TIGHT, 'dropout_add_layernorm %s y seed %d' % (name, seed))
        close(rstd, want_rstd, TIGHT, 'dropout_add_layernorm %s rstd seed %d' % (name, seed))
        y2, none = ops.dropout_add_layernorm(tv, rv, gamma.cuda(), beta.cuda(), 1e-5, P, seed, site, want_rstd=False)
        assert none is None and torch.equal(y, y2)                               # without rstd: the same y


# ---------------------------------------------------------------------------------------------------
# e. lime_layernorm_bwd_dropout_f32
# ---------------------------------------------------------------------------------------------------
def _ln_bwd_dropout(dy, div, y, gamma, beta, rstd, lddd, p, seed, site):
    """The C entry directly (ops.layernorm_bwd allocates a contiguous dz_drop) -> (status, dz, dgamma, dbeta, dzsum, dz_drop view, its buffer)."""
    from lime_cikm25_amd import _lib
    lib = _lib.load()
    M, E = y.shape
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    dz = torch.empty(M, E, device='cuda')
    dg, db, dzs = (torch.empty(E, device='cuda') for _ in range(3))
    ws = torch.empty(max(1, lib.lime_layernorm_bwd_workspace(M, E)), device='cuda')
    dt, dbuf = view(torch.zeros(M, E), lddd, fill=-7.0)
    st = lib.lime_layernorm_bwd_dropout_f32(ptr(dy), dy.stride(0), div, 1.0 / div, ptr(y), y.stride(0), ptr(gamma), ptr(beta), ptr(rstd), ptr(dz),
                                            E, M, E, ptr(dg), ptr(db), ptr(dzs), 0, ptr(ws), ws.numel(), ptr(dt), lddd, p, seed, site,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return st, dz, dg, db, dzs, dt, dbuf


def _ln_bwd_inputs(M, E, div):
    z, gamma, beta = rnd(M, E, seed=31), rnd(E, seed=32) * 0.5 + 1.0, rnd(E, seed=33)
    dy = rnd((M + div - 1) // div, E, seed=34)
    return z, gamma, beta, dy


LNB_CASES = [(37, 100, 1), (37, 100, 16), (37, 300, 1), (37, 300, 16), (37, 400, 1), (37, 400, 16), (12309, 100, 16)]       # 12309 > 768 * 16 rows


@pytest.mark.parametrize('M,E,div', LNB_CASES)
def test_layernorm_bwd_dropout(ops, M, E, div):
    z, gamma, beta, dy = _ln_bwd_inputs(M, E, div)
    lddd = E + 4
    for seed, site in (PAIRS[:2] if M < 1000 else PAIRS[1:2]):
        m = dc.multiplier(P, seed, site, (M, E))
        y, rstd, dz, dg, db, dzsum, dt = dc.layernorm_bwd_ref(z, gamma, beta, dy, div, m=m)
        st, gdz, gdg, gdb, gdzs, gdt, dbuf = _ln_bwd_dropout(dy.cuda(), div, y.float().cuda(), gamma.cuda(), beta.cuda(), rstd.float().cuda(),
                                                             lddd, P, seed, site)
        assert st == 0
        what = 'layernorm_bwd_dropout M%d E%d div%d seed %d' % (M, E, div, seed)
        close(gdz, dz, BWD, what + ' dz')
        close(gdg, dg, BWD, what + ' dgamma')
        close(gdb, db, BWD, what + ' dbeta')
        bitwise(gdt, dc.dropped_f32(gdz.cpu().numpy(), keep2d(P, seed, site, M, E), P), what + ' dz_drop')
        close(gdzs, dzsum, BWD, what + ' dzsum')
        rest = dbuf.clone()
        rest.as_strided((M, E), (lddd, 1), 0).fill_(-7.0)
        assert bool((rest == -7.0).all()), 'wrote outside dz_drop'


def test_layernorm_bwd_dropout_without_16_byte_rows(ops):
    """E = 50: the C entry refuses the fused copy; ops.layernorm_bwd's fallback (a dropout pass of its own) states the same thing."""
    M, E, div = 37, 50, 1
    seed, site = PAIRS[1]
    z, gamma, beta, dy = _ln_bwd_inputs(M, E, div)
    m = dc.multiplier(P, seed, site, (M, E))
    y, rstd, dz, dg, db, dzsum, dt = dc.layernorm_bwd_ref(z, gamma, beta, dy, div, m=m)
    args = (y.float().cuda(), gamma.cuda(), beta.cuda(), rstd.float().cuda())
    st = _ln_bwd_dropout(dy.cuda(), div, *args, E, P, seed, site)[0]
    assert st == LIME_ERR_UNSUPPORTED
    gdz, gdg, gdb, gdzs, gdt = ops.layernorm_bwd(dy.cuda(), *args, dropout=(P, seed, site))
    close(gdz, dz, BWD, 'layernorm_bwd fallback E50 dz')
    bitwise(gdt, dc.dropped_f32(gdz.cpu().numpy(), keep2d(P, seed, site, M, E), P), 'layernorm_bwd fallback E50 dz_drop')
    close(gdzs, dzsum, BWD, 'layernorm_bwd fallback E50 dzsum')
    close(gdg, dg, BWD, 'layernorm_bwd fallback E50 dgamma')
    close(gdb, db, BWD, 'layernorm_bwd fallback E50 dbeta')


# ---------------------------------------------------------------------------------------------------
# f. lime_linear_f32 with dropout_p
# ---------------------------------------------------------------------------------------------------
# (id, M, N, act, fused in the GEMM's epilogue); the operands of tests/linear_route_cases.py's dropout_relu_m4096_n512 (K = 64), which the
# split-product kernel takes when the fill rules are off
_ROUTE_CASE = next(c for c in linear_route_cases.CASES if c['id'] == 'dropout_relu_m4096_n512')
assert (_ROUTE_CASE['M'], _ROUTE_CASE['N'], _ROUTE_CASE['act']) == (4096, 512, 'relu')
LINEAR_CASES = [('fused-m4096', 4096, 512, 'relu', True), ('second-pass-m4000', 4000, 512, 'relu', False), ('act-none', 4096, 512, None, False),
                ('m300', 300, 512, 'relu', False), ('scalar-pass-n50', 300, 50, 'relu', False)]


@pytest.mark.parametrize('case', LINEAR_CASES, ids=[c[0] for c in LINEAR_CASES])
def test_linear_dropout(ops, case):
    from lime_cikm25_amd import _lib
    name, M, N, act, fused = case
    K = _ROUTE_CASE['K']
    a, w, b = rnd(M, K, seed=41), rnd(N, K, seed=42, scale=0.3), rnd(N, seed=43)
    seed, site = PAIRS[1]
    prev = ops.set_split_gemm(True, force=True)
    try:
        plan = ops.linear_plan(a.cuda(), w.cuda(), b.cuda(), act=act, dropout=(P, seed, site))
        got = ops.linear(a.cuda(), w.cuda(), b.cuda(), act=act, dropout=(P, seed, site))
        ran = _lib.load().lime_last_linear_kernel().decode()
    finally:
        ops.set_split_gemm(prev)
    assert plan['kernel'] == ran
    assert plan['dropout'] == (not fused), (plan, ran)                           # the second_pass bit says which form ran
    assert ran.startswith('gemm_sp_kernel') or not fused, ran
    want = dc.linear_dropout_ref(a, w, b, act, dc.multiplier(P, seed, site, (M, N)))
    close(got, want, GEMM_TIGHT, 'linear dropout %s (%s)' % (name, ran.split('<')[0]))
    keep = keep2d(P, seed, site, M, N)
    assert bool((got.cpu().numpy()[~keep] == 0).all())


# ---------------------------------------------------------------------------------------------------
# g / h. attention with dropout on the probabilities
# ---------------------------------------------------------------------------------------------------
def _attn_operands(S, hd, hs):
    n_seq, h = dc.N_SEQ, dc.N_HEAD
    tok = n_seq * S
    vals = rnd(tok, 3, h, hd, seed=S + hd)
    buf = torch.zeros(tok, 3, h, hs)
    buf[..., :hd] = vals
    g = buf.view(tok, 3 * h * hs).cuda()
    W = h * hs
    return vals, (g[:, :W], g[:, W:2 * W], g[:, 2 * W:])


class _split:
    def __init__(self, ops, split):
        self.ops, self.split = ops, split

    def __enter__(self):
        self.prev = self.ops.set_split_gemm(self.split) if self.split is not None else None

    def __exit__(self, *exc):
        if self.split is not None:
            self.ops.set_split_gemm(self.prev)


@pytest.mark.parametrize('case', dc.ATTN_FWD_CASES, ids=[dc.attn_case_id(c) for c in dc.ATTN_FWD_CASES])
def test_token_attention_dropout(ops, case):
    route, S, hd, hs, split = case
    n_seq, h, scale = dc.N_SEQ, dc.N_HEAD, 1.0 / math.sqrt(hd)
    vals, (q, k, v) = _attn_operands(S, hd, hs)
    for seed, site in PAIRS[:2]:
        with _split(ops, split):
            got = ops.token_attention_dropout(q, k, v, n_seq, S, h, hd, scale, P, seed, site, head_stride=hs)
        want, _ = dc.attn_ref(vals.double(), n_seq, S, h, hd, scale, m=dc.multiplier(P, seed, site, (n_seq, h, S, S)))
        close(got, want, TIGHT, 'attention forward %s seed %d' % (dc.attn_case_id(case), seed))


@pytest.mark.parametrize('case', dc.ATTN_BWD_CASES, ids=[dc.attn_case_id(c) for c in dc.ATTN_BWD_CASES])
def test_token_attention_bwd_dropout(ops, case):
    route, S, hd, hs, split = case
    n_seq, h, scale = dc.N_SEQ, dc.N_HEAD, 1.0 / math.sqrt(hd)
    tok = n_seq * S
    vals, (q, k, v) = _attn_operands(S, hd, hs)
    dout = rnd(tok, h * hd, seed=S)
    for seed, site in PAIRS[:2]:
        drop = (P, seed, site)
        want_o, want = dc.attn_bwd_ref(vals, dout, n_seq, S, h, hd, scale, m=dc.multiplier(P, seed, site, (n_seq, h, S, S)))
        with _split(ops, split):
            out = ops.token_attention_dropout(q, k, v, n_seq, S, h, hd, scale, *drop, head_stride=hs)
            dqkv = ops.token_attention_bwd(q, k, v, dout.cuda(), n_seq, S, h, hd, scale, head_stride=hs, out=out, dropout=drop)
            again = ops.token_attention_bwd(q, k, v, dout.cuda(), n_seq, S, h, hd, scale, head_stride=hs, out=out, dropout=drop)
        what = 'attention backward %s seed %d' % (dc.attn_case_id(case), seed)
        close(out, want_o, TIGHT, what + ' out')
        d4 = dqkv.view(tok, 3, h, hs)
        close(d4[..., :hd], want, BWD, what + ' dqkv')
        assert bool((d4[..., hd:] == 0).all()), 'pad columns of dq / dk / dv must be exact zeros'
        assert torch.equal(dqkv, again), 'two runs of the backward differ'


# ---------------------------------------------------------------------------------------------------
# i. lime_cand_attn_weights_train_f32 / _bwd_f32
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,N,H,nh,hd,p', dc.CAND_CASES)
def test_cand_attn_weights_on_host_masks(ops, B, N, H, nh, hd, p):
    D = nh * hd
    qp, kp = rnd(B * N, D, seed=1, scale=2.0), rnd(B * H, D, seed=2, scale=2.0)
    g = torch.Generator().manual_seed(9)
    mask = torch.rand(B, H, generator=g) < 0.7
    if B > 1:
        mask[0] = False                                                          # an impression with an empty history
    dagg = rnd(B, H, seed=3)
    for seed, site in PAIRS[1:]:
        m = dc.multiplier(p, seed, site, (B, nh, N, H))
        qd, kd = qp.double().requires_grad_(), kp.double().requires_grad_()
        agg = dc.cand_attn_ref(qd, kd, mask, m, B, N, H, nh, hd)
        agg.backward(dagg.double())
        args = (qp.cuda().view(-1), kp.cuda().view(-1), mask.cuda())
        what = 'cand_attn (%d, %d, %d, %d, %d) seed %d' % (B, N, H, nh, hd, seed)
        close(ops.cand_attn_weights_train(*args, B, N, H, D, nh, p, seed, site), agg.detach(), TIGHT, what + ' agg')
        dqp, dkp = ops.cand_attn_weights_bwd(*args, dagg.cuda(), B, N, H, D, nh, p, seed, site)
        close(dqp, qd.grad, BWD, what + ' dqp')
        close(dkp, kd.grad, BWD, what + ' dkp')
