"""Every fp32 kernel that normalises a row, on the ill-conditioned rows of ln_cond_cases.py (mean / std up to 64, constant rows,
variance below eps, rows * 1e4) against fp64, per row class:  err <= max(B0, K_REF * err_ref32)  -- B0 the bound the entry's own test
module asserts, err_ref32 the error of the same operations in torch fp32 on the CPU (ln_cond_cases.py says where K_REF comes from).
Each check prints its figures ('LNCOND ...') before it asserts."""
import numpy as np
import pytest
import torch

import dropout_cases as dc
import ln_cond_cases as lc
from test_backward_gpu import TIGHT as RSTD_TIGHT                  # rstd of the fused epilogue (test_layernorm_bwd_and_rstd)
from test_dropout_kernels_gpu import TIGHT as DROPOUT_LN_TIGHT     # dropout_add_layernorm: y and rstd
from test_ffn_sp_gpu import TIGHT as FFN_TIGHT
from test_kernels_gpu import TIGHT as MFMA_TIGHT                   # lime_linear_f32 on the fp32 kernels, gate_ln, gate_ln_sage
from test_oproj_sp_gpu import TIGHT as OPROJ_TIGHT
from test_split_gemm_gpu import TIGHT as SPLIT_TIGHT
from test_wide_heads_gpu import BWD                                # test_backward_gpu.py's bound on gradients against fp64 autograd

pytestmark = pytest.mark.gpu

# family -> (M, lime_set_split_gemm mode, B0): 4 = fp32 kernels whatever the fill rules say, 7 = split products for every form
FAMILIES = {'general': (1000, 1, MFMA_TIGHT), 'pp': (4096, 4, MFMA_TIGHT), 'sp': (4096, 7, SPLIT_TIGHT)}
LINEAR_CASES = [(fam, N, form) for fam in FAMILIES for N in (300, 320) for form in lc.LINEAR_FORMS
                if not (fam == 'general' and form == 'pool32')]     # pool32 needs M % 32 == 0 and the big-M kernels
LINEAR_CASES += [(fam, 260, 'dense') for fam in FAMILIES]           # 60 zero-padded columns behind the row
# no residual: the split-product kernel has no such LayerNorm instantiation (the plan gives it to pp under every mode)
NORES_CASES = [(fam, b) for fam in ('general', 'pp') for b in range(len(lc.NORES_BIAS))]


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from lime_cikm25_amd import ops as _ops
    from lime_cikm25_amd import _lib
    _lib.load()
    return _ops


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def statements(key, case, statement):
    """(want fp64, ref32) of a case: computed once, shared, never written to."""
    return cached(('st',) + key, lambda: (statement(case, torch.float64), statement(case, torch.float32)))


def hold(what, got, want, ref, cls, b0, names=lc.CLASSES, per_block=None, skip=()):
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape), (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what
    e_got = lc.class_errors(got, want, cls, names, per_block)
    e_ref = lc.class_errors(ref, want, cls, names, per_block)
    bad = []
    for name, e in e_got.items():
        if name in skip:
            continue
        bnd = lc.bound(b0, e_ref[name])
        print('LNCOND %-44s %-7s err %.3e ref32 %.3e bound %.3e' % (what, name, e, e_ref[name], bnd))
        if not e <= bnd:
            bad.append('%s %s: err %.3e > %.3e (ref32 %.3e)' % (what, name, e, bnd, e_ref[name]))
    assert not bad, '\n'.join(bad)


def hold_all(what, got, want, ref, b0):
    """One figure for a result whose rows are not rows of a class (column sums, group means)."""
    hold(what, got.reshape(1, -1), want.reshape(1, -1), ref.reshape(1, -1), np.zeros(1, dtype=int), b0, names=('all',))


def launch_linear(ops, c, mode, rstd=False, pool32=False, misaligned_out=False):
    """-> (plan, y, rstd or None): ops.linear on case c under split mode `mode`, restored afterwards."""
    from lime_cikm25_amd import _lib
    lib = _lib.load()
    d = lambda t: None if t is None else t.cuda()
    kw = dict(a=d(c['a']), w=d(c['w']), bias=d(c['bias']), ln=(d(c['gamma']), d(c['beta'])), ln_eps=lc.EPS)
    if c['res'] is not None:
        kw['res'] = d(c['res'])
        if c['res_ids'] is not None:
            kw.update(res_ids=d(c['res_ids']), res_pe=d(c['res_pe']), res_period=lc.PE_PERIOD)
    if rstd:
        kw['ln_rstd'] = torch.zeros(c['M'], dtype=torch.float32, device='cuda')
    if pool32:
        kw['pool32'] = True
    if misaligned_out:           # a result 4 bytes off a 16-byte boundary: only the general family takes it
        kw['out'] = torch.zeros(c['M'] * c['N'] + 8, dtype=torch.float32, device='cuda')[1:1 + c['M'] * c['N']].view(c['M'], c['N'])
    start = lib.lime_set_split_gemm(-1)
    try:
        lib.lime_set_split_gemm(mode)
        plan = ops.linear_plan(**kw)
        y = ops.linear(**kw)
        ran = lib.lime_last_linear_kernel().decode()
        torch.cuda.synchronize()
    finally:
        lib.lime_set_split_gemm(start)
    assert plan['kernel'] == ran, (plan, ran)
    return plan, y, kw.get('ln_rstd')


# ---------------------------------------------------------------------------------------------------
# lime_linear_f32 with ln
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fam,N,form', LINEAR_CASES, ids=['%s-n%d-%s' % c for c in LINEAR_CASES])
def test_linear_layernorm(ops, fam, N, form):
    M, mode, b0 = FAMILIES[fam]
    data_form = 'ids_pe' if form == 'ids_pe' else 'dense'
    c = cached(('lin', M, N, data_form), lambda: lc.linear_case(M, N, data_form))
    want, ref = statements(('lin', M, N, data_form), c, lc.linear_statement)
    plan, y, rstd = launch_linear(ops, c, mode, rstd=form == 'rstd', pool32=form == 'pool32')
    assert plan['family'] == fam, plan
    what = 'linear %s M%d N%d %s' % (fam, M, N, form)
    if form == 'pool32':
        hold(what + ' pool', y, want['pool'], ref['pool'], c['cls'], b0, per_block=32)
        return
    hold(what + ' y', y, want['y'], ref['y'], c['cls'], b0)
    if form == 'rstd':
        hold(what + ' rstd', rstd[:, None], want['rstd'][:, None], ref['rstd'][:, None], c['cls'], RSTD_TIGHT)
    const = torch.from_numpy(np.isin(c['cls'], [lc.CLASSES.index('const3'), lc.CLASSES.index('const0')]))
    # (with res_ids the row is 3.0 or 0.0 + 0.25 + an eighth of the position: every sum of such a row is exact in fp32 too)
    assert torch.equal(y.cpu()[const], c['beta'].expand(int(const.sum()), N)), 'a constant row does not give beta'


@pytest.mark.parametrize('fam,b', NORES_CASES, ids=['%s-bias%d' % c for c in NORES_CASES])
def test_linear_layernorm_without_residual(ops, fam, b):
    M, mode, b0 = FAMILIES[fam]
    N = 300
    c = cached(('nores', M, N, b), lambda: lc.linear_nores_case(M, N, lc.NORES_BIAS[b]))
    want, ref = statements(('nores', M, N, b), c, lc.linear_statement)
    plan, y, _ = launch_linear(ops, c, mode)
    assert plan['family'] == fam, plan
    hold('linear %s M%d nores bias %.3f y' % (fam, M, lc.NORES_BIAS[b]), y, want['y'], ref['y'], c['cls'], b0, names=c['names'])
    if 'zero' in c['names']:
        zero = torch.from_numpy(c['cls'] == c['names'].index('zero'))
        assert torch.equal(y.cpu()[zero], c['beta'].expand(int(zero.sum()), N)), 'a constant row does not give beta'


def test_every_ln_capable_family_is_reached_and_n324_is_refused(ops):
    """The cases above between them plan general, pp and sp (each test asserts its own); mid never takes a LayerNorm; the epilogue
    holds a row of at most 320 columns, so N = 324 is refused under every mode, not routed somewhere unnormalised."""
    from lime_cikm25_amd import _lib
    assert {fam for fam, _, _ in LINEAR_CASES} == {f for f in _lib.LINEAR_FAMILY.values() if f not in (None, 'mid')}
    for fam, (M, mode, _) in FAMILIES.items():
        c = lc.linear_case(M, 324, 'dense')
        with pytest.raises(_lib.LimeHipError, match='N <= 320'):
            launch_linear(ops, c, mode)


# ---------------------------------------------------------------------------------------------------
# encoder_ffn_sp, encoder_oproj_sp: one 128-row tile and a ragged tail
# ---------------------------------------------------------------------------------------------------
M_SMALL = 133


def test_ffn_sp(ops):
    c = cached(('ffn',), lambda: lc.ffn_case(M_SMALL))
    want, ref = statements(('ffn',), c, lc.ffn_statement)
    d = lambda k: c[k].cuda()
    w1p, w2p = ops.ffn_pack_sp(d('w1'), d('w2'))
    y = ops.encoder_ffn_sp(d('x'), w1p, w2p, d('b1'), d('b2'), (d('gamma'), d('beta')), lc.EPS)
    torch.cuda.synchronize()
    hold('ffn_sp M%d y' % M_SMALL, y, want['y'], ref['y'], c['cls'], FFN_TIGHT)


@pytest.mark.parametrize('form', ['dense', 'ids_pe'])
def test_oproj_sp(ops, form):
    c = cached(('oproj', form), lambda: lc.oproj_case(M_SMALL, form))
    want, ref = statements(('oproj', form), c, lc.oproj_statement)
    d = lambda k: c[k].cuda()
    res = dict(res=d('res'))
    if form == 'ids_pe':
        res.update(res_ids=d('res_ids'), res_pe=d('res_pe'), res_period=lc.PE_PERIOD)
    y = ops.encoder_oproj_sp(d('a'), ops.oproj_pack_sp(d('w')), d('bias'), (d('gamma'), d('beta')), lc.EPS, **res)
    torch.cuda.synchronize()
    hold('oproj_sp M%d %s y' % (M_SMALL, form), y, want['y'], ref['y'], c['cls'], OPROJ_TIGHT)


# ---------------------------------------------------------------------------------------------------
# dropout_add_layernorm: the 16-byte kernel (E = 300) and the scalar one (E = 301)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('width', [300, 301])
@pytest.mark.parametrize('p', [0.0, dc.P])
def test_dropout_add_layernorm(ops, width, p):
    seed, site = dc.SEED_SITES[0]
    c = cached(('daln', width), lambda: lc.dropout_ln_case(M_SMALL, width))
    m = dc.multiplier(p, seed, site, (M_SMALL, width))
    want, ref = lc.dropout_ln_statement(c, m, torch.float64), lc.dropout_ln_statement(c, m, torch.float32)
    d = lambda k: c[k].cuda()
    y, rstd = ops.dropout_add_layernorm(d('t'), d('res'), d('gamma'), d('beta'), lc.EPS, p, seed, site)
    torch.cuda.synchronize()
    what = 'dropout_add_layernorm E%d p%.1f' % (width, p)
    hold(what + ' y', y, want['y'], ref['y'], c['cls'], DROPOUT_LN_TIGHT)
    hold(what + ' rstd', rstd[:, None], want['rstd'][:, None], ref['rstd'][:, None], c['cls'], DROPOUT_LN_TIGHT)


# ---------------------------------------------------------------------------------------------------
# gate_ln, gate_ln_sage (sixteen waves a group below 4096 groups, four from there on), gate_ln_bwd
# ---------------------------------------------------------------------------------------------------
GATE_ROWS, GATE_D = 144, 400


def test_gate_ln(ops):
    c = cached(('gate', GATE_ROWS, GATE_D), lambda: lc.gate_case(GATE_ROWS, GATE_D))
    want, ref = statements(('gate', GATE_ROWS, GATE_D), c, lc.gate_statement)
    d = lambda k: c[k].cuda()
    y = ops.gate_ln(d('y'), d('x'), d('s'), d('bias'), d('gamma'), d('beta'), lc.EPS)
    torch.cuda.synchronize()
    hold('gate_ln rows%d D%d y' % (GATE_ROWS, GATE_D), y.view(GATE_ROWS, GATE_D), want['y'], ref['y'], c['cls'], MFMA_TIGHT)


@pytest.mark.parametrize('G,H,D', [(12, 12, 400), (4096, 2, 64)])
def test_gate_ln_sage(ops, G, H, D):
    c = cached(('gate', G * H, D), lambda: lc.gate_case(G * H, D))
    want, ref = cached(('st', 'sage', G, H, D), lambda: (lc.gate_statement(c, torch.float64, H), lc.gate_statement(c, torch.float32, H)))
    d = lambda k: c[k].cuda()
    y, mean = ops.gate_ln_sage(d('y'), d('x'), d('s'), d('bias'), d('gamma'), d('beta'), lc.EPS, G, H, D, 1, H)
    torch.cuda.synchronize()
    what = 'gate_ln_sage G%d H%d D%d' % (G, H, D)
    hold(what + ' y', y, want['y'], ref['y'], c['cls'], MFMA_TIGHT)
    hold_all(what + ' mean', mean.cpu(), want['mean'], ref['mean'], MFMA_TIGHT)


def test_gate_ln_bwd(ops):
    c = cached(('gate', GATE_ROWS, GATE_D), lambda: lc.gate_case(GATE_ROWS, GATE_D))
    dout = lc.u(GATE_ROWS, GATE_D, seed=60)
    want, ref = lc.gate_bwd_statement(c, dout, torch.float64), lc.gate_bwd_statement(c, dout, torch.float32)
    d = lambda k: c[k].cuda()
    got = ops.gate_ln_bwd(d('y'), d('x'), d('s'), d('bias'), d('gamma'), d('beta'), lc.EPS, dout.cuda())
    torch.cuda.synchronize()
    for name, g, w, r in zip(('dy', 'dx', 'dscale', 'dbias', 'dgamma', 'dbeta'), got, want, ref):
        g = g.cpu().view(w.shape)
        if name in ('dy', 'dx'):
            hold('gate_ln_bwd ' + name, g, w, r, c['cls'], BWD)
        elif name == 'dscale':
            hold('gate_ln_bwd ' + name, g[:, None], w[:, None], r[:, None], c['cls'], BWD, skip=lc.DSCALE_SKIP)
        else:
            hold_all('gate_ln_bwd ' + name, g, w, r, BWD)


# ---------------------------------------------------------------------------------------------------
# layernorm_bwd on the y and rstd the fused epilogue of each family itself produced (M = 4096, N = 300)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings('ignore:lime_linear_f32. LayerNorm epilogue on operands that are not 16-byte aligned')
@pytest.mark.parametrize('fam', list(FAMILIES))
def test_layernorm_bwd_on_the_forward_kernels_rstd(ops, fam):
    M, N = 4096, 300
    _, mode, b0 = FAMILIES[fam]
    c = cached(('lin', M, N, 'dense'), lambda: lc.linear_case(M, N, 'dense'))
    plan, y, rstd = launch_linear(ops, c, mode, rstd=True, misaligned_out=fam == 'general')
    assert plan['family'] == fam, plan
    dy = lc.u(M, N, seed=70)

    def make():
        z = lc.linear_pre(c, torch.float64)
        return dc.layernorm_bwd_ref(z, c['gamma'], c['beta'], dy)[2:], lc.layernorm_bwd_ref32(lc.linear_pre(c, torch.float32), c['gamma'], c['beta'], dy)
    want, ref = cached(('st', 'lnbwd'), make)
    got = ops.layernorm_bwd(dy.cuda(), y.contiguous(), c['gamma'].cuda(), c['beta'].cuda(), rstd)
    torch.cuda.synchronize()
    hold('layernorm_bwd after %s dz' % fam, got[0], want[0], ref[0], c['cls'], BWD)
    for name, g, w, r in zip(('dgamma', 'dbeta', 'dzsum'), got[1:], want[1:], ref[1:]):
        hold_all('layernorm_bwd after %s %s' % (fam, name), g.cpu(), w, r, BWD)
