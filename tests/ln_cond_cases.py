"""Ill-conditioned LayerNorm rows for every fp32 kernel that normalises, as data and CPU statements -- shared by
tests/test_ln_conditioning_cpu.py (which checks the inputs) and tests/test_ln_conditioning_gpu.py (which holds the kernels to them).

Every other kernel test draws zero-mean rows of unit scale, on which var = E[x^2] - mean^2 and var = E[(x - mean)^2] agree to a few
ulps.  They part as mean / std grows: the one-pass form loses mean^2 / var of the fp32 significand, the centred form does not.

Row classes (CLASSES; a launch holds all of them, BLOCK consecutive rows of a class at a time, so every tile mixes classes):
  r0 r4 r16 r64   uniform(-1, 1) + r * DEV: mean / std = r  (DEV = 0.577, the standard deviation of uniform(-1, 1))
  mixed           the same, consecutive rows cycling through the four r: statistics that leak between the rows of a tile show
  const3 const0   every column 3.0 / 0.0: variance 0, the result is beta
  tiny huge       uniform(-1, 1) * 1e-4 (variance 3e-9, below eps = 1e-5) and * 1e4

How a class reaches an entry: through the residual of the GEMM entries (dense, or table rows by res_ids + positional rows that are
constant along a row), through x (ffn_sp: x is its residual; gate_ln: x and scale -- half the rows carry scale 1, the other half
scale 2 on x / 2 behind a saturated gate), through res (oproj_sp, dropout_add_layernorm).  The products that are added to such a row
stay small (K = 64, activations * 0.1, weights * 0.3; rows of a constant class get a zero activation row, the tiny class a * 1e-5
one), so the row that is normalised keeps its class.  The no-residual form of lime_linear_f32 has no per-row operand besides the
product: there the offset is a constant bias (one launch per value: r * DEV and 3.0), the deviation is the product itself
(activations * 0.72: standard deviation DEV), and the rows of a launch are 'normal', 'huge' and, where they mean something
(nores_classes), 'zero' (constant result: beta) and 'tiny'.

Statements: ``want`` is fp64; ``ref32`` the same torch operations in fp32 on the CPU (F.linear + F.layer_norm: the reference
model's arithmetic) -- the yardstick.  Bound per class and output:  err <= max(B0, K_REF * err_ref32)  with helpers.rel_err, B0 the
bound the entry's own test module already asserts (imported there, not copied).

K_REF = 8.  The rule: the largest err / err_ref32 (classes where err_ref32 > 0) observed on an MI355X over the entries that ALREADY
centred before these tests existed, doubled and rounded up to a power of two, and nothing above 8.  Measured (the full table:
profiles/ln_conditioning.txt):
    lime_linear_f32, general family   5.32   (N = 320, res_ids + PE, r16: 1.907e-05 / 3.583e-06; 4.8 at r64)
    ffn_sp                            2.78   (tiny: 3.4e-07 / 1.2e-07, both far below B0; 1.4 at r64)
    oproj_sp                          1.35
    dropout_add_layernorm             1.69
    gate_ln, gate_ln_sage             1.00, 1.03
Every entry but the first doubles and rounds to at most 8.  The general family's 5.3 would double to 16, which the rule rejects; it is
not its LayerNorm: that kernel loads the residual row into its accumulators, so each of the K / 4 accumulation steps of the product
rounds at the residual's magnitude (37 at r64) where F.linear + residual rounds there once -- the split-product kernel with res_ids,
which adds the residual in its epilogue, sits at 1.0 with the same LayerNorm code.  K_REF is therefore the cap itself, 8: the largest
value the rule admits, 1.5 times what the general family needs, and a bound the one-pass form E[x^2] - mean^2 misses by 3 times
at r16 and by 10 to 16 times at r64.  The pp and sp families of lime_linear_f32 are held to this K_REF, not to one measured on themselves.

bf16 entries (ffn_bf16, encoder_block_bf16) are out of scope: bf16 rounding of an offset row leaves no significand for the
deviation (at r = 64 the row is 37 +- 1 with a bf16 spacing of 0.25), and their 6e-3 gate says nothing about the variance formula.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
DEV = 0.577
R = (0, 4, 16, 64)
CLASSES = ('r0', 'r4', 'r16', 'r64', 'mixed', 'const3', 'const0', 'tiny', 'huge')
BLOCK = 32                      # rows of one class in a run (the 32-row pooling block of lime_linear_f32's pool32)
K = 64

K_REF = 8                       # the docstring says where it comes from


def u(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * 2 - 1


def class_index(M, block=BLOCK):
    """int array [M]: the class of every row."""
    return (np.arange(M) // block) % len(CLASSES)


def class_rows(M, N, seed, block=BLOCK):
    """(rows [M, N] fp32, class index [M], per-row scale of the small operand that is added to the row [M] fp32)."""
    cls = class_index(M, block)
    base = u(M, N, seed=seed)
    off = torch.zeros(M)
    mul = torch.ones(M)
    small = torch.full((M,), 0.1)
    for i, name in enumerate(CLASSES):
        rows = torch.from_numpy(cls == i)
        if name.startswith('r'):
            off[rows] = int(name[1:]) * DEV
        elif name == 'mixed':
            idx = torch.nonzero(rows).flatten()
            off[idx] = torch.tensor([R[int(j) % 4] * DEV for j in idx])
        elif name.startswith('const'):
            mul[rows], off[rows], small[rows] = 0.0, float(name[5:]), 0.0
        elif name == 'tiny':
            mul[rows], small[rows] = 1e-4, 1e-5
        elif name == 'huge':
            mul[rows] = 1e4
    return (base * mul[:, None] + off[:, None]).float(), cls, small


def mixed_offsets(M, block=BLOCK):
    """mean / std the rows of the 'mixed' class were given, [M] (nan elsewhere)."""
    cls = class_index(M, block)
    out = np.full(M, np.nan)
    for j in np.nonzero(cls == CLASSES.index('mixed'))[0]:
        out[j] = R[j % 4]
    return out


def ln_params(N, seed):
    return 0.75 + 0.5 * torch.rand(N, generator=torch.Generator().manual_seed(seed)), u(N, seed=seed + 1)


def layer_norm(z, gamma, beta, eps=EPS):
    """(LayerNorm(z), rstd) in z's dtype."""
    gamma, beta = gamma.to(z.dtype), beta.to(z.dtype)
    return F.layer_norm(z, (z.shape[1],), gamma, beta, eps), 1.0 / torch.sqrt(z.var(dim=1, unbiased=False) + eps)


# ---------------------------------------------------------------------------------------------------
# lime_linear_f32 with ln
# ---------------------------------------------------------------------------------------------------
LINEAR_FORMS = ('dense', 'ids_pe', 'rstd', 'pool32')
PE_PERIOD = 4                   # divides both class cycles: a gathered table row knows the position its reader has in the period
NORES_BIAS = tuple(r * DEV for r in R) + (3.0,)
NORES_MUL = {'normal': 0.72, 'zero': 0.0, 'tiny': 0.72e-4, 'huge': 0.72e4}


def nores_classes(bias_value):
    """The row classes of the no-residual launch with this bias.  'zero' (the row is the bias: constant) where 300 copies of the
    bias add up exactly in fp32, as the constant rows of CLASSES do; 'tiny' only without an offset: 1e-4 u + 37 is 37 in fp32, for
    the yardstick too."""
    return ('normal', 'zero', 'tiny', 'huge') if bias_value == 0.0 else ('normal', 'zero') if bias_value == 3.0 else ('normal', 'huge')


def class_preserving_ids(M, seed, block=BLOCK):
    """ids [M] int32 into a table that holds class_rows(M, ...): row r reads a table row of r's class (and, in the mixed class, of
    r's offset): one with the same position in the cycle of len(CLASSES) * block rows."""
    cycle = len(CLASSES) * block
    g = torch.Generator().manual_seed(seed)
    r = torch.arange(M)
    pos = r % cycle
    n = (M - 1 - pos) // cycle + 1                        # table rows at this position of the cycle
    return (pos + cycle * (torch.rand(M, generator=g) * n).long().clamp(max=n - 1)).to(torch.int32)


def _bias_and_pe(rows, N, cls):
    """(bias, positional rows, table) of the gathered form: a constant bias of 0.25 and positional rows of 0.125 * position, both
    taken off the table rows beforehand (a table row and its reader share the position), so the sum is the class row again.  Not off
    the tiny rows: 1e-4 u - 0.375 would round u away; they keep the shift (a constant along the row: the variance stays 3e-9)."""
    pe = (0.125 * torch.arange(PE_PERIOD, dtype=torch.float32))[:, None].repeat(1, N)
    shift = 0.25 + pe[torch.arange(rows.shape[0]) % PE_PERIOD]
    shift[torch.from_numpy(cls == CLASSES.index('tiny'))] = 0.0
    return torch.full((N,), 0.25), pe, rows - shift


def linear_case(M, N, form, seed=0):
    """The operands of one residual form as CPU fp32 tensors + the class index."""
    rows, cls, small = class_rows(M, N, seed)
    c = dict(M=M, N=N, form=form, cls=cls, a=u(M, K, seed=seed + 1) * small[:, None], w=u(N, K, seed=seed + 2) * 0.3, bias=None,
             res=rows, res_ids=None, res_pe=None)
    c['gamma'], c['beta'] = ln_params(N, seed + 3)
    if form == 'ids_pe':
        c['bias'], c['res_pe'], c['res'] = _bias_and_pe(rows, N, cls)
        c['res_ids'] = class_preserving_ids(M, seed + 5)
    return c


def linear_nores_case(M, N, bias_value, seed=0):
    """No residual: z = a w^T + bias_value; rows of nores_classes(bias_value) in runs of BLOCK."""
    names = nores_classes(bias_value)
    cls = (np.arange(M) // BLOCK) % len(names)
    mul = torch.tensor([NORES_MUL[n] for n in names])[torch.from_numpy(cls)]
    c = dict(M=M, N=N, form='nores', cls=cls, names=names, a=u(M, K, seed=seed + 1) * mul[:, None], w=u(N, K, seed=seed + 2) * 0.3,
             bias=torch.full((N,), float(bias_value)), res=None, res_ids=None, res_pe=None)
    c['gamma'], c['beta'] = ln_params(N, seed + 3)
    return c


def linear_pre(c, dtype):
    """The row LayerNorm sees, in dtype: residual + F.linear."""
    z = F.linear(c['a'].to(dtype), c['w'].to(dtype), None if c['bias'] is None else c['bias'].to(dtype))
    if c['res'] is not None:
        if c['res_ids'] is not None:
            res = c['res'].to(dtype)[c['res_ids'].long()] + c['res_pe'].to(dtype)[torch.arange(c['M']) % PE_PERIOD]
        else:
            res = c['res'].to(dtype)
        z = res + z
    return z


def linear_statement(c, dtype):
    """{'y', 'rstd', 'pool'} in dtype; pool: the means of 32 consecutive result rows (M % 32 == 0)."""
    y, rstd = layer_norm(linear_pre(c, dtype), c['gamma'], c['beta'])
    out = {'y': y, 'rstd': rstd}
    if c['M'] % 32 == 0:
        out['pool'] = y.reshape(-1, 32, c['N']).mean(1)
    return out


# ---------------------------------------------------------------------------------------------------
# encoder_ffn_sp, encoder_oproj_sp (E = 300)
# ---------------------------------------------------------------------------------------------------
E = 300
SMALL_BLOCK = 4
FFN_F = 512


def ffn_case(M, seed=20):
    """x carries the class and is the residual.  w2 is small, so the feed-forward term leaves the class of the row alone."""
    rows, cls, _ = class_rows(M, E, seed, SMALL_BLOCK)
    c = dict(M=M, cls=cls, x=rows, w1=u(FFN_F, E, seed=seed + 1) * 0.3 * E ** -0.5, b1=u(FFN_F, seed=seed + 2) * 0.1,
             w2=u(E, FFN_F, seed=seed + 3) * 0.01 * FFN_F ** -0.5, b2=torch.zeros(E))
    c['gamma'], c['beta'] = ln_params(E, seed + 4)
    return c


def ffn_pre(c, dtype):
    x = c['x'].to(dtype)
    h = torch.relu(F.linear(x, c['w1'].to(dtype), c['b1'].to(dtype)))
    return x + F.linear(h, c['w2'].to(dtype), c['b2'].to(dtype))


def ffn_statement(c, dtype):
    return {'y': layer_norm(ffn_pre(c, dtype), c['gamma'], c['beta'])[0]}


def oproj_case(M, form, seed=30):
    rows, cls, small = class_rows(M, E, seed, SMALL_BLOCK)
    c = dict(M=M, N=E, form=form, cls=cls, a=u(M, E, seed=seed + 1) * small[:, None], w=u(E, E, seed=seed + 2) * 0.3 * E ** -0.5,
             bias=torch.zeros(E), res=rows, res_ids=None, res_pe=None)
    c['gamma'], c['beta'] = ln_params(E, seed + 3)
    if form == 'ids_pe':
        c['bias'], c['res_pe'], c['res'] = _bias_and_pe(rows, E, cls)
        c['res_ids'] = class_preserving_ids(M, seed + 5, SMALL_BLOCK)
    return c


def oproj_statement(c, dtype):
    return {'y': layer_norm(linear_pre(c, dtype), c['gamma'], c['beta'])[0]}


# ---------------------------------------------------------------------------------------------------
# dropout_add_layernorm: z = res + m * t, m the keep * scale multiplier of dropout_cases
# ---------------------------------------------------------------------------------------------------
def dropout_ln_case(M, width, seed=40):
    rows, cls, small = class_rows(M, width, seed, SMALL_BLOCK)
    c = dict(M=M, E=width, cls=cls, res=rows, t=u(M, width, seed=seed + 1) * small[:, None])
    c['gamma'], c['beta'] = ln_params(width, seed + 2)
    return c


def dropout_ln_statement(c, m, dtype):
    y, rstd = layer_norm(c['res'].to(dtype) + m.to(dtype) * c['t'].to(dtype), c['gamma'], c['beta'])
    return {'y': y, 'rstd': rstd}


# ---------------------------------------------------------------------------------------------------
# gate_ln, gate_ln_sage: LayerNorm(g * (s x) + (1 - g) x), g = sigmoid(s y + bias)
# ---------------------------------------------------------------------------------------------------
def gate_case(rows_n, D, seed=50):
    """Even runs of SMALL_BLOCK rows: scale 1 (the blend is x whatever the gate).  Odd runs: scale 2, x = row / 2, y = 40 (the gate is
    exactly 1 in fp32 and fp64 alike, the blend 2 x): the class arrives through x and scale."""
    rows, cls, _ = class_rows(rows_n, D, seed, 2 * SMALL_BLOCK)
    odd = torch.from_numpy((np.arange(rows_n) // SMALL_BLOCK) % 2 == 1)
    s = torch.where(odd, torch.tensor(2.0), torch.tensor(1.0))
    y = u(rows_n, D, seed=seed + 1)
    y[odd] = 40.0
    const = torch.from_numpy(np.isin(cls, [CLASSES.index('const3'), CLASSES.index('const0')]))
    y[const & ~odd] = -40.0          # (a constant row stays one: 1 - g is exactly 1 and g x is below half an ulp of x)
    c = dict(rows=rows_n, D=D, cls=cls, x=rows / s[:, None], y=y, s=s, bias=u(D, seed=seed + 2) * 0.3)
    c['gamma'], c['beta'] = ln_params(D, seed + 3)
    return c


def gate_pre(c, dtype):
    x, y, s, bias = (c[k].to(dtype) for k in ('x', 'y', 's', 'bias'))
    g = torch.sigmoid(s[:, None] * y + bias)
    return g * (s[:, None] * x) + (1 - g) * x


def gate_statement(c, dtype, H=None):
    """{'y'} and, with H (rows = groups * H), {'mean'}: the means of each group's H result rows (gate_ln_sage's aggregate)."""
    out = {'y': layer_norm(gate_pre(c, dtype), c['gamma'], c['beta'])[0]}
    if H:
        out['mean'] = out['y'].reshape(-1, H, c['D']).mean(1)
    return out


# d out / d scale of a row is a sum over its columns in which sum(dz) = 0 cancels: on a constant row nothing but rounding is left of
# it, and in the mixed class the rows with an offset set the error while the rows without set the magnitude it is judged by -- the
# fp32 yardstick itself is at 2.4e-4 there.  dscale is held on the other classes.
DSCALE_SKIP = ('mixed', 'const3')


def gate_bwd_statement(c, dout, dtype):
    """(dy, dx, dscale, dbias, dgamma, dbeta) of gate_ln under dout, by autograd in dtype."""
    leaves = [c[k].to(dtype).clone().requires_grad_() for k in ('y', 'x', 's', 'bias', 'gamma', 'beta')]
    y, x, s, bias, gamma, beta = leaves
    g = torch.sigmoid(s[:, None] * y + bias)
    out = F.layer_norm(g * (s[:, None] * x) + (1 - g) * x, (c['D'],), gamma, beta, EPS)
    out.backward(dout.to(dtype))
    return [t.grad for t in leaves]


def layernorm_bwd_ref32(z, gamma, beta, dy):
    """dropout_cases.layernorm_bwd_ref's (dz, dgamma, dbeta, dzsum) in fp32: the yardstick of the backward."""
    z = z.float().clone().requires_grad_()
    g, b = gamma.float().clone().requires_grad_(), beta.float().clone().requires_grad_()
    F.layer_norm(z, (z.shape[1],), g, b, EPS).backward(dy.float())
    return z.grad, g.grad, b.grad, z.grad.sum(0)


# ---------------------------------------------------------------------------------------------------
# per-class errors
# ---------------------------------------------------------------------------------------------------
def class_errors(got, want, cls, names=CLASSES, per_block=None):
    """{class: helpers.rel_err of that class's rows}; per_block: got / want hold one row per `per_block` rows (pool32)."""
    from helpers import rel_err
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if per_block:
        cls = cls[::per_block]
    out = {}
    for i, name in enumerate(names):
        rows = cls == i
        if rows.any():
            out[name] = rel_err(got[rows], want[rows])
    return out


def bound(b0, e32):
    return max(b0, K_REF * e32)


def realised_ratio(z, rows):
    """mean over `rows` of |row mean| / row std, fp64."""
    z = z.double()[torch.from_numpy(rows)]
    return float((z.mean(1).abs() / z.std(1, unbiased=False)).mean())
