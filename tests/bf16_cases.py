"""The bf16 token-encoder kernels (csrc/token_attn_bf16.hip, inproj_bf16.hip, ffn_bf16.hip, lime_linear_bf16) stated in fp64, the
criterion their results are held to, and the case lists of tests/test_bf16_kernels_gpu.py.  Imports without a GPU.

Statements.  One function per kernel, the arithmetic of the kernel's header comment: an operand is rounded to bf16 exactly where the
kernel rounds it (the rounding points tests/test_bf16_budget.py::POINTS names: word rows, weights, qkv, attention output, x1, h -- and
the unnormalised softmax exponentials the bf16 attention feeds to P.V), everything else is exact in the evaluation's dtype, and the
result is NOT rounded.  ``dt=torch.float64`` is the reference (``inproj64``, ``attn64``, ``ffn64``, ``block64``, ``linear64``);
``dt=torch.float32`` with ``perm=None`` / ``perm=<seed>`` is the same statement as a correct fp32 implementation would compute it, with
the k axis of every product in natural / in a permuted order (tests/test_bf16_reference_cpu.py).

Criterion (``assert_bf16_matches``).  Distances are in bf16 ulps taken at max(|want|, mean |want| of the element's row): an element
that cancelled to nearly zero is judged against the scale of its row, where an ulp still means something.
  * Hard bound on every element.
      - single-rounding results (in_proj, the plain GEMM): 0.5 ulp for the one rounding + the fp32 accumulation bound
        n 2^-24 sum |a_i w_i| of an n-term sum in ANY order (n = the K products and the added fp32 row), expressed in ulps.  Derived.
      - multi-rounding results (attention, fused ffn, fused block): 0.5 ulp for the final rounding + ALLOWANCE_ULPS for an
        intermediate bf16 rounding (P, h, x1) that falls the other way under another summation order.  ALLOWANCE_ULPS is 2 x the largest
        pre-rounding deviation between the fp64 statement and its fp32 evaluations (natural and permuted k order) over every case
        below, as tests/test_bf16_reference_cpu.py measures it on the CPU -- nothing in it comes from the kernels:
            largest deviation: attention 1.12 ulp, ffn 0.22 ulp, block 2.35 ulp; 2 x 2.347 = 4.69, carried as ALLOWANCE_ULPS = 4.7:
            bound 5.2 ulp.  (The large deviations are single events: ONE x1 element of the 9.9 M of the block's largest case rounds the
            other way and moves its own output by gamma2 rstd2 ulp(x1) -- more than two ulps of an output that beta2 has pulled
            below its row's mean; in the attention, one exponential of a sharply peaked row.  Without such an event the deviations
            are a few hundredths of an ulp.  The hard bound is therefore the coarse part of the criterion; the share cap is the fine one.)
  * Share cap: at most 1 % of the elements may differ from bf16(want64).  The fp32 CPU evaluations differ, per case, in
            in_proj    0.000-0.104 % of the elements (the most: 1 element of a one-row case), worst distance 0.500 ulp
            linear     0.005-0.010 %, 0.500 ulp
            attention  0.000-0.098 %, 1.46 ulp
            ffn        0.000-0.140 %, 0.61 ulp
            block      0.023-0.185 %, 2.47 ulp
    so the cap leaves a correct implementation more than five times the room it needs on its worst case, and a kernel that is one ulp
    off in one lane of 64 (1.6 % of the elements) fails it.
(The figures above are what ``pytest -s tests/test_bf16_reference_cpu.py`` prints; that test fails if they stop covering the cases.)

The fp32 block means (pool32) are compared with the fp64 mean of the UNROUNDED fp64 rows, ``helpers.rel_err`` below POOL_TOL_FFN /
POOL_TOL_BLOCK."""
import functools
import math

import pytest
import torch

ALLOWANCE_ULPS = 4.7            # see the docstring; tests/test_bf16_reference_cpu.py checks it against what it measures
SHARE_CAP = 0.01
POOL_TOL_FFN, POOL_TOL_BLOCK = 2e-3, 4e-3
NOMINAL_CUS = 256               # the MI355X's CU count: what the CPU module sizes the persistent-loop cases with
EP = 304                        # the column count the fused kernels carry the model dimension in
SENTINEL = 7.0


# ---------------------------------------------------------------------------------------------------
# generators, rounding
# ---------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(*shape, seed, scale=1.0):
    return (torch.rand(*shape, generator=gen(seed)) * 2 - 1) * scale


def bf(t):
    """fp32 -> the bf16 tensor a kernel is given."""
    return t.to(torch.bfloat16)


def padded_bf16(t, cols, rows=None):
    """fp32 [R, C] -> bf16 [rows or R, cols], zero padded (what ops.to_bf16 produces)."""
    out = torch.zeros(t.shape[0] if rows is None else rows, cols, dtype=torch.bfloat16)
    out[:t.shape[0], :t.shape[1]] = bf(t)
    return out


def round_bf16(t):
    """Round-to-nearest-even to bf16 precision, dtype kept.  fp64 is rounded ONCE (through fp32 it would be rounded twice)."""
    if t.dtype != torch.float64:
        return t.to(torch.bfloat16).to(t.dtype)
    b = t.contiguous().view(torch.int64)
    b = (b + ((1 << 44) - 1) + ((b >> 45) & 1)) & ~((1 << 45) - 1)
    r = b.view(torch.float64)
    tiny = t.abs() < 2.0 ** -120                          # bf16 subnormals (and zero): the plain conversion
    return torch.where(tiny, t.to(torch.float32).to(torch.bfloat16).to(torch.float64), r)


def _mm(a, b_t, perm):
    """a [.., M, K] . b_t [.., N, K]^T, the k axis in natural (perm None) or a seeded permuted order."""
    if perm is not None:
        p = torch.randperm(a.shape[-1], generator=gen(perm + a.shape[-1]))
        a, b_t = a[..., p], b_t[..., p]
    return a @ b_t.transpose(-1, -2)


def _layer_norm(y, g, beta, eps, dt):
    mean = y.mean(dim=1, keepdim=True)
    var = ((y - mean) ** 2).mean(dim=1, keepdim=True)
    return (y - mean) / torch.sqrt(var + eps) * g.to(dt) + beta.to(dt)


# ---------------------------------------------------------------------------------------------------
# the statements
# ---------------------------------------------------------------------------------------------------
def inproj64(rows_bf16, w, add, out_row, dt=torch.float64, perm=None):
    """rows_bf16 [M, >= E] (the operand rows of the M results, already gathered), w fp32 [N, E], add fp32 [period, N], out_row int64 [M]:
    rows . bf16(w)^T + add[out_row % period] -- the fp32 periodic row of the OUTPUT row."""
    E = w.shape[1]
    return _mm(rows_bf16[:, :E].to(dt), bf(w).to(dt), perm) + add.to(dt)[out_row % add.shape[0]]


def inproj_acc_bound(rows_bf16, w, add, out_row):
    """The fp32 accumulation bound of ``inproj64``'s sum, absolute: n 2^-24 sum |terms|, n = E products + the added row."""
    E = w.shape[1]
    mag = rows_bf16[:, :E].double().abs() @ bf(w).double().abs().t() + add.double().abs()[out_row % add.shape[0]]
    return (E + 1) * 2.0 ** -24 * mag


def linear64(a_bf16, w_bf16, bias=None, res=None, dt=torch.float64, perm=None):
    """The plain bf16 GEMM: a . w^T (+ fp32 bias) (+ fp32 residual rows)."""
    y = _mm(a_bf16.to(dt), w_bf16.to(dt), perm)
    if bias is not None:
        y = y + bias.to(dt)
    if res is not None:
        y = y + res.to(dt)
    return y


def linear_acc_bound(a_bf16, w_bf16, bias=None, res=None):
    mag = a_bf16.double().abs() @ w_bf16.double().abs().t()
    n = a_bf16.shape[1]
    for t in (bias, res):
        if t is not None:
            mag, n = mag + t.double().abs(), n + 1
    return n * 2.0 ** -24 * mag


def attn_rounds_p(S, hd):
    """True where the bf16-MFMA kernel runs (P rounded to bf16 for P.V); S >= 256 or an odd head_dim take the widened fp32 core."""
    return S <= 128 and hd % 2 == 0


def attn64(q, k, v, n_seq, S, h, hd, scale, dt=torch.float64, perm=None):
    """q / k / v bf16 [n_seq * S, h * 32] (heads 32 columns apart) -> [n_seq * S, h * hd]: softmax with the max subtracted; the
    unnormalised exponentials rounded to bf16 for P.V (``attn_rounds_p``), the product divided by the sum of the UNROUNDED ones."""
    qf, kf, vf = (t.reshape(n_seq, S, h, 32)[..., :hd].permute(0, 2, 1, 3).to(dt) for t in (q, k, v))
    s = _mm(qf, kf, perm) * scale
    e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    p = round_bf16(e) if attn_rounds_p(S, hd) else e
    o = _mm(p, vf.transpose(-1, -2), perm) / e.sum(dim=-1, keepdim=True)
    return o.permute(0, 2, 1, 3).reshape(n_seq * S, h * hd)


def _ffn(xf, w1, b1, w2, b2, g, beta, eps, dt, perm):
    h = round_bf16(torch.relu(_mm(xf, bf(w1).to(dt), perm) + bf(b1).to(dt)))           # b1 rides in the GEMM: applied in bf16
    return _layer_norm(xf + _mm(h, bf(w2).to(dt), perm) + b2.to(dt), g, beta, eps, dt)


def ffn64(x, w1, b1, w2, b2, g, beta, eps, E, dt=torch.float64, perm=None):
    """x bf16 [M, 304] (E real columns) -> [M, E]: LayerNorm(x + bf16(relu(x bf16(w1)^T + bf16(b1))) bf16(w2)^T + b2) over E columns."""
    return _ffn(x[:, :E].to(dt), w1, b1, w2, b2, g, beta, eps, dt, perm)


def block64(attn, w0, add_rows, res_rows, g1, beta1, eps1, w1, b1, w2, b2, g2, beta2, eps2, E, dt=torch.float64, perm=None):
    """attn bf16 [M, 304], res_rows bf16 [M, >= E] (the residual rows, already gathered), add_rows fp32 [period, E] ->
    x1 = bf16(LN1(res + attn bf16(w0)^T + add_rows[r % period])), then the ffn statement on x1."""
    M = attn.shape[0]
    z = res_rows[:, :E].to(dt) + _mm(attn[:, :E].to(dt), bf(w0).to(dt), perm) + add_rows.to(dt)[torch.arange(M) % add_rows.shape[0], :E]
    x1 = round_bf16(_layer_norm(z, g1, beta1, eps1, dt))
    return _ffn(x1, w1, b1, w2, b2, g2, beta2, eps2, dt, perm)


def pool32_64(rows64):
    """fp64 [M, E] (M % 32 == 0) -> the means over 32-row blocks."""
    return rows64.view(rows64.shape[0] // 32, 32, rows64.shape[1]).mean(dim=1)


# ---------------------------------------------------------------------------------------------------
# the criterion
# ---------------------------------------------------------------------------------------------------
def ulp_scale(want64):
    """The bf16 ulp at max(|want|, mean |want| of the row), per element."""
    a = want64.abs()
    m = torch.maximum(a, a.mean(dim=-1, keepdim=True)).clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(m)) - 7)


def bf16_distance(got, want64):
    """(distance in ulps per element, mask of the elements that differ from bf16(want64)); got: any float tensor on want64's device."""
    g = got.to(torch.float64)
    return (g - want64).abs() / ulp_scale(want64), g != round_bf16(want64)


def assert_bf16_matches(got_bf16, want64, single_rounding, what):
    """got_bf16 against the fp64 statement.  single_rounding: None for a multi-rounding result (bound 0.5 + ALLOWANCE_ULPS), or the
    absolute fp32 accumulation bound per element (``inproj_acc_bound`` / ``linear_acc_bound``) of a single-rounding one.  Prints and
    returns (share of elements that differ from bf16(want64), worst distance in ulps)."""
    assert got_bf16.dtype == torch.bfloat16 and got_bf16.shape == want64.shape, (what, got_bf16.dtype, got_bf16.shape, want64.shape)
    assert want64.dtype == torch.float64 and want64.numel() > 0, what
    assert torch.isfinite(got_bf16).all(), '%s: non-finite values' % what
    dist, differs = bf16_distance(got_bf16, want64)
    if single_rounding is None:
        over = dist - (0.5 + ALLOWANCE_ULPS)
    else:
        over = dist - (0.5 + single_rounding.to(want64.device) / ulp_scale(want64))
    n_diff, n = int(differs.sum()), differs.numel()
    worst, i = float(dist.max()), int(over.argmax())
    print('%s: %d of %d elements (%.4f %%) differ from bf16(fp64), worst %.3f ulp' % (what, n_diff, n, 100.0 * n_diff / n, worst))
    assert float(over.max()) <= 0.0, '%s: element %d is %.3f ulp from the fp64 statement, %.3f over its bound (got %r, want %r)' % (
        what, i, float(dist.reshape(-1)[i]), float(over.max()), float(got_bf16.reshape(-1)[i]), float(want64.reshape(-1)[i]))
    assert n_diff <= SHARE_CAP * n, '%s: %d of %d elements (%.3f %%) differ from bf16(fp64); at most 1 %% may' % (what, n_diff, n, 100.0 * n_diff / n)
    return n_diff / n, worst


# ---------------------------------------------------------------------------------------------------
# cases.  Every ``*_inputs`` is cached: the tests of a case share one set of inputs and one fp64 reference and leave them unchanged.
# ---------------------------------------------------------------------------------------------------
def _ids(cases, fmt):
    return [pytest.param(*c, id=fmt % c) for c in cases]


# ---- attention: (S, n_seq, n_head, head_dim, out_cols or None for n_head * head_dim, ldo or None for out_cols) ----
ATTN_DENSE = [
    (32, 1, 1, 32, None, None), (32, 5, 3, 20, None, None), (64, 3, 10, 30, None, None), (64, 3, 10, 30, 304, None),
    (128, 2, 10, 32, None, None), (128, 2, 10, 30, 304, None), (32, 2, 1, 2, None, None),
    (64, 3, 10, 30, 304, 320),               # the output a column view of a wider buffer
    (32, 5, 3, 20, None, 72),
    (512, 1, 10, 30, 304, None),             # the widened fp32 core
    (64, 3, 10, 15, None, None),             # odd head_dim: the fp32-core fallback
]
ATTN_DENSE_PARAMS = [pytest.param(*c, id='S%d-n%d-h%d-hd%d-cols%s-ldo%s' % c) for c in ATTN_DENSE]


def attn_loop_cases(n_cu):
    """(S, n_seq, n_head, head_dim): (sequence, head) pairs that make some persistent workgroup run a second iteration --
    S = 128 (one pair per group, CUs x 3 workgroups): 3 CUs + 40 pairs; S = 32 (four pairs per group, CUs x 4 workgroups):
    16 CUs + 6 pairs (2 mod 4), two groups of a second iteration, the last of them half invalid."""
    out = []
    for S, pairs, hd in ((128, 3 * n_cu + 40, 30), (32, 16 * n_cu + 6, 32)):
        h = next(c for c in (10, 8, 7, 6, 5, 4, 3, 2, 1) if pairs % c == 0)
        out.append((S, pairs // h, h, hd))
    return out


@functools.lru_cache(maxsize=4)
def attn_inputs(S, n_seq, h, hd, seed=0):
    """-> (qkv bf16 [n_seq * S, 3 * h * 32] with zero pad columns, scale, want64 [n_seq * S, h * hd])."""
    x = torch.zeros(n_seq * S, 3 * h, 32)
    x[:, :, :hd] = rnd(n_seq * S, 3 * h, hd, seed=1000 + 7 * S + 3 * h + hd + seed, scale=2.0)
    qkv = bf(x.view(n_seq * S, 3 * h * 32))
    W, scale = h * 32, 1.0 / math.sqrt(hd)
    return qkv, scale, attn64(qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:], n_seq, S, h, hd, scale)


ATTN_ROWMAP = _ids([(S, hd) for S in (32, 64, 128) for hd in (30, 32)], 'S%d-hd%d')
ATTN_COUNTS = [None, 0, 1, 'half', 'all', 'over']            # n_seq_dev: None, 0, 1, n_seq // 2, n_seq, n_seq + 5


# ---- in_proj: (M or None for 128 CUs + 130, K, N, S); E: the weight's columns (the operand columns K - E .. K get zero weights) ----
INPROJ = [(1, 304, 960, 32), (127, 64, 320, 32), (129, 296, 640, 100), (385, 320, 960, 128), (None, 304, 960, 128)]
INPROJ_PARAMS = [pytest.param(*c, id='M%s-K%d-N%d-S%d' % c) for c in INPROJ]
INPROJ_E = {304: 300, 64: 60, 296: 290, 320: 313}
INPROJ_M_DEV = [0, 1, 128, 129, 'over']                      # 'over': M + 7


def inproj_m(M, n_cu):
    return 128 * n_cu + 130 if M is None else M


@functools.lru_cache(maxsize=2)
def inproj_inputs(M, K, N, S):
    """-> dict: table bf16 [V, K], ids int32 [M], w fp32 [N, E], adds {1: fp32 [1, N], S: fp32 [S, N]}, c_ids int32 [M] (injective into
    cap rows), cap."""
    V, E = 500, INPROJ_E[K]
    seed = 2000 + K + N + S + M % 1000
    d = dict(V=V, E=E, cap=M + 61)
    d['table'] = padded_bf16(rnd(V, E, seed=seed), K)
    d['ids'] = torch.randint(0, V, (M,), generator=gen(seed + 1), dtype=torch.int32)
    d['w'] = rnd(N, E, seed=seed + 2, scale=0.06)
    d['adds'] = {1: rnd(1, N, seed=seed + 3), S: rnd(S, N, seed=seed + 4)}
    d['c_ids'] = torch.randperm(d['cap'], generator=gen(seed + 5))[:M].to(torch.int32)
    return d


@functools.lru_cache(maxsize=1)
def _inproj_products(M, K, N, S):
    """rows . bf16(w)^T and |rows| . |bf16(w)|^T in fp64: shared by the case's periods and row orders."""
    d = inproj_inputs(M, K, N, S)
    x, w = d['table'][d['ids'].long()][:, :d['E']].double(), bf(d['w']).double()
    return x @ w.t(), x.abs() @ w.abs().t()


def inproj_want(M, K, N, S, period, scattered):
    """-> (want64 [M, N] = ``inproj64`` of the case, its accumulation bound ``inproj_acc_bound``) for result rows r = 0..M-1 (stored at
    c_ids[r] when scattered)."""
    d = inproj_inputs(M, K, N, S)
    prod, mag = _inproj_products(M, K, N, S)
    add = d['adds'][period].double()[(d['c_ids'].long() if scattered else torch.arange(M)) % period]
    return prod + add, (d['E'] + 1) * 2.0 ** -24 * (mag + add.abs())


# ---- fused ffn / block ----
FFN_E, FFN_F, FFN_M = (289, 292, 300, 303), (128, 384, 512), (1, 33, 129)
FFN_PARAMS = _ids([(E, F) for E in FFN_E for F in FFN_F], 'E%d-F%d')
FFN_BIG = (292, 512)                                         # at M = 128 CUs + 160: several tiles per workgroup
BLOCK_S, BLOCK_M, BLOCK_F = 32, 200, 512                     # M not a multiple of S (nor of 128)
BLOCK_PARAMS = _ids([(E, kind, per) for E in (292, 296, 300) for kind in (2, 3) for per in (1, BLOCK_S)], 'E%d-kind%d-period%d')
BLOCK_BIG = (300, 3, 1)                                      # residual kind 3 at M = 128 CUs + 160
M_DEV_ROWS, M_DEV = 288, (0, 32, 160, 288)                   # three tiles, the last one a quarter full


def big_m(n_cu):
    return 128 * n_cu + 160


@functools.lru_cache(maxsize=4)
def ffn_weights(E, F, seed=0):
    s = 3000 + E + F + seed
    return dict(w1=rnd(F, E, seed=s + 1, scale=0.06), b1=rnd(F, seed=s + 2), w2=rnd(E, F, seed=s + 3, scale=0.05), b2=rnd(E, seed=s + 4),
                g=rnd(E, seed=s + 5) + 1.5, beta=rnd(E, seed=s + 6), eps=1e-5)


@functools.lru_cache(maxsize=4)
def ffn_inputs(E, F, M):
    """-> (x bf16 [M, 304] with zero pad columns, weights dict, want64 [M, E])."""
    w = ffn_weights(E, F)
    x = padded_bf16(rnd(M, E, seed=3100 + E + F + M % 1000, scale=1.5), EP)
    return x, w, ffn64(x, w['w1'], w['b1'], w['w2'], w['b2'], w['g'], w['beta'], w['eps'], E)


@functools.lru_cache(maxsize=4)
def block_inputs(E, kind, period, M, F=BLOCK_F):
    """-> dict: attn bf16 [M, 304]; kind 2: table bf16 [V, 304] + res_ids int32 [M], kind 3: res bf16 [M, 304]; add_rows fp32
    [period, E] (out_proj's bias, + the positional rows); w0, g1, beta1, eps1; the ffn weights; want64 [M, E]."""
    s = 4000 + E + 10 * kind + period + M % 1000
    d = dict(ffn_weights(E, F, seed=1), V=300)
    d['attn'] = padded_bf16(rnd(M, E, seed=s), EP)
    d['w0'], d['g1'], d['beta1'], d['eps1'] = rnd(E, E, seed=s + 1, scale=0.06), rnd(E, seed=s + 2) + 1.5, rnd(E, seed=s + 3), 1e-5
    d['add_rows'] = rnd(period, E, seed=s + 4)
    if kind == 2:
        d['table'] = padded_bf16(rnd(d['V'], E, seed=s + 5), EP)
        d['res_ids'] = torch.randint(0, d['V'], (M,), generator=gen(s + 6), dtype=torch.int32)
        d['res_rows'] = d['table'][d['res_ids'].long()]
    else:
        d['res_rows'] = padded_bf16(rnd(M, E, seed=s + 5), EP)
    d['want'] = block_want(d, E)
    return d


def block_want(d, E, dt=torch.float64, perm=None):
    return block64(d['attn'], d['w0'], d['add_rows'], d['res_rows'], d['g1'], d['beta1'], d['eps1'], d['w1'], d['b1'], d['w2'], d['b2'],
                   d['g'], d['beta'], d['eps'], E, dt=dt, perm=perm)


# ---- the plain GEMM with the compacted path's arguments, the bf16 mean pool ----
LINEAR_M = (130, 4100)
POOL_S = (32, 128)


@functools.lru_cache(maxsize=2)
def linear_inputs(M, S=32):
    """The in_proj of the compacted path as two lime_linear_bf16 launches (K = N = 304: E = 300 zero padded)."""
    E, V, s = 300, 400, 5000 + M
    d = dict(E=E, V=V, S=S, cap=M + 45)
    d['table'] = padded_bf16(rnd(V, E, seed=s), EP)
    d['ids'] = torch.randint(1, V, (M,), generator=gen(s + 1), dtype=torch.int32)
    d['w'] = padded_bf16(rnd(E, E, seed=s + 2, scale=0.06), EP, rows=EP)
    d['res'] = torch.zeros(S, EP)
    d['res'][:, :E] = rnd(S, E, seed=s + 3)
    d['c_ids'] = torch.randperm(d['cap'], generator=gen(s + 4))[:M].to(torch.int32)
    return d
