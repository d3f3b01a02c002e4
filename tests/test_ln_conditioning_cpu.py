"""The inputs of tests/test_ln_conditioning_gpu.py, not the kernels: every row class is what ln_cond_cases.py says it is (realised
mean / std, zero variance, variance below eps), and on every class the yardstick itself -- the same operations in torch fp32 on the
CPU -- stays within a quarter of the bound the GPU test applies, so the bound has room for a correct kernel and none for a wrong
formula.  A class that failed this would be resized here, never given a wider bound there."""
import numpy as np
import pytest
import torch

import dropout_cases as dc
import ln_cond_cases as lc
import test_ln_conditioning_gpu as G
from test_kernels_gpu import TOL as NORTH_STAR


def quarter(what, want, ref, cls, b0, names=lc.CLASSES, per_block=None, skip=()):
    e_ref = lc.class_errors(ref, want, cls, names, per_block)
    assert e_ref, what
    for name, e in e_ref.items():
        if name in skip:
            continue
        assert 4 * e <= lc.bound(b0, e), '%s %s: ref32 %.3e against a bound of %.3e' % (what, name, e, lc.bound(b0, e))
        # (from K_REF = 4 on the line above holds by construction.)  A class on which fp32 itself is a quarter of the way to the
        # north star's 1e-3 says nothing about a kernel
        assert 4 * e <= NORTH_STAR, '%s %s: ref32 %.3e' % (what, name, e)


def quarter_all(what, want, ref, b0):
    quarter(what, want.reshape(1, -1), ref.reshape(1, -1), np.zeros(1, dtype=int), b0, names=('all',))


def check_classes(what, z, cls, block, names=lc.CLASSES, tol=0.05, const_exact=True):
    """z: the fp64 rows LayerNorm sees."""
    var = z.double().var(dim=1, unbiased=False)
    for i, name in enumerate(names):
        rows = cls == i
        assert rows.any(), (what, name)
        if name in ('r0', 'r4', 'r16', 'r64'):
            r, got = int(name[1:]), lc.realised_ratio(z, rows)
            assert abs(got - r) <= tol * r if r else got < 0.25, '%s %s: realised mean / std %.3f' % (what, name, got)
        elif name == 'mixed':
            offs = lc.mixed_offsets(len(cls), block)
            for r in lc.R:
                got = lc.realised_ratio(z, offs == r)
                assert abs(got - r) <= tol * r if r else got < 0.25, '%s mixed %d: realised mean / std %.3f' % (what, r, got)
        elif name.startswith('const') or name == 'zero':
            if const_exact:
                assert float(var[torch.from_numpy(rows)].max()) == 0.0, (what, name)
        elif name == 'tiny':
            assert float(var[torch.from_numpy(rows)].max()) < lc.EPS, (what, name)
        elif name == 'huge':
            assert float(var[torch.from_numpy(rows)].min()) > 1e6, (what, name)


def test_the_r_table_of_the_issue():
    assert lc.R == (0, 4, 16, 64) and lc.K_REF in (1, 2, 4, 8)
    assert abs(lc.DEV - (1.0 / 3.0) ** 0.5) < 1e-3


@pytest.mark.parametrize('M', sorted({m for m, _, _ in G.FAMILIES.values()}))
@pytest.mark.parametrize('N', sorted({n for _, n, _ in G.LINEAR_CASES}))
@pytest.mark.parametrize('form', ['dense', 'ids_pe'])
def test_linear_rows(M, N, form):
    c = lc.linear_case(M, N, form)
    check_classes('linear %d %d %s' % (M, N, form), lc.linear_pre(c, torch.float64), c['cls'], lc.BLOCK)
    if form == 'ids_pe':
        ids = c['res_ids'].long().numpy()
        assert (lc.class_index(M)[ids] == c['cls']).all() and ((ids % 4) == (np.arange(M) % 4)).all()
        assert len(set(ids.tolist())) > M // 2                       # a gather, not the identity
        assert (ids != np.arange(M)).any()
    want, ref = lc.linear_statement(c, torch.float64), lc.linear_statement(c, torch.float32)
    for fam, (m, _, b0) in G.FAMILIES.items():
        if m != M:
            continue
        quarter('linear y', want['y'], ref['y'], c['cls'], b0)
        quarter('linear rstd', want['rstd'][:, None], ref['rstd'][:, None], c['cls'], G.RSTD_TIGHT)
        if M % 32 == 0:
            quarter('linear pool', want['pool'], ref['pool'], c['cls'], b0, per_block=32)


@pytest.mark.parametrize('b', range(len(lc.NORES_BIAS)))
def test_linear_rows_without_residual(b):
    for M in sorted({m for m, _, _ in G.FAMILIES.values()}):
        c = lc.linear_nores_case(M, 300, lc.NORES_BIAS[b])
        z = lc.linear_pre(c, torch.float64)
        check_classes('nores', z, c['cls'], lc.BLOCK, names=c['names'])
        normal = c['cls'] == c['names'].index('normal')
        got, r = lc.realised_ratio(z, normal), lc.NORES_BIAS[b] / lc.DEV
        assert abs(got - r) <= 0.05 * r if r else got < 0.25, (b, got, r)
        want, ref = lc.linear_statement(c, torch.float64), lc.linear_statement(c, torch.float32)
        quarter('nores y', want['y'], ref['y'], c['cls'], G.MFMA_TIGHT, names=c['names'])


def test_ffn_and_oproj_rows():
    c = lc.ffn_case(G.M_SMALL)
    # the feed-forward term is not constant along a row: the constant classes are near-constant here, and judged by fp64 like the rest
    check_classes('ffn', lc.ffn_pre(c, torch.float64), c['cls'], lc.SMALL_BLOCK, const_exact=False)
    quarter('ffn y', lc.ffn_statement(c, torch.float64)['y'], lc.ffn_statement(c, torch.float32)['y'], c['cls'], G.FFN_TIGHT)
    for form in ('dense', 'ids_pe'):
        c = lc.oproj_case(G.M_SMALL, form)
        check_classes('oproj ' + form, lc.linear_pre(c, torch.float64), c['cls'], lc.SMALL_BLOCK)
        quarter('oproj y', lc.oproj_statement(c, torch.float64)['y'], lc.oproj_statement(c, torch.float32)['y'], c['cls'], G.OPROJ_TIGHT)


@pytest.mark.parametrize('width', [300, 301])
@pytest.mark.parametrize('p', [0.0, dc.P])
def test_dropout_add_layernorm_rows(width, p):
    seed, site = dc.SEED_SITES[0]
    c = lc.dropout_ln_case(G.M_SMALL, width)
    m = dc.multiplier(p, seed, site, (G.M_SMALL, width))
    check_classes('daln', c['res'].double() + m * c['t'].double(), c['cls'], lc.SMALL_BLOCK)
    want, ref = lc.dropout_ln_statement(c, m, torch.float64), lc.dropout_ln_statement(c, m, torch.float32)
    quarter('daln y', want['y'], ref['y'], c['cls'], G.DROPOUT_LN_TIGHT)
    quarter('daln rstd', want['rstd'][:, None], ref['rstd'][:, None], c['cls'], G.DROPOUT_LN_TIGHT)


@pytest.mark.parametrize('rows,D,H', [(G.GATE_ROWS, G.GATE_D, None), (12 * 12, 400, 12), (4096 * 2, 64, 2)])
def test_gate_rows(rows, D, H):
    c = lc.gate_case(rows, D)
    assert set(c['s'].tolist()) == {1.0, 2.0}
    for i in range(len(lc.CLASSES)):                                 # every class arrives under both scales
        assert set(c['s'][torch.from_numpy(c['cls'] == i)].tolist()) == {1.0, 2.0}
    check_classes('gate', lc.gate_pre(c, torch.float64), c['cls'], 2 * lc.SMALL_BLOCK, tol=0.05 if D >= 300 else 0.1)
    want, ref = lc.gate_statement(c, torch.float64, H), lc.gate_statement(c, torch.float32, H)
    quarter('gate y', want['y'], ref['y'], c['cls'], G.MFMA_TIGHT)
    if H:
        quarter_all('gate mean', want['mean'], ref['mean'], G.MFMA_TIGHT)


def test_backward_yardsticks():
    c = lc.gate_case(G.GATE_ROWS, G.GATE_D)
    dout = lc.u(G.GATE_ROWS, G.GATE_D, seed=60)
    want, ref = lc.gate_bwd_statement(c, dout, torch.float64), lc.gate_bwd_statement(c, dout, torch.float32)
    for name, w, r in zip(('dy', 'dx', 'dscale', 'dbias', 'dgamma', 'dbeta'), want, ref):
        if name in ('dy', 'dx'):
            quarter('gate_ln_bwd ' + name, w, r, c['cls'], G.BWD)
        elif name == 'dscale':
            quarter('gate_ln_bwd ' + name, w[:, None], r[:, None], c['cls'], G.BWD, skip=lc.DSCALE_SKIP)
        else:
            quarter_all('gate_ln_bwd ' + name, w, r, G.BWD)
    M, N = 4096, 300
    c = lc.linear_case(M, N, 'dense')
    dy = lc.u(M, N, seed=70)
    want = dc.layernorm_bwd_ref(lc.linear_pre(c, torch.float64), c['gamma'], c['beta'], dy)[2:]
    ref = lc.layernorm_bwd_ref32(lc.linear_pre(c, torch.float32), c['gamma'], c['beta'], dy)
    quarter('layernorm_bwd dz', want[0], ref[0], c['cls'], G.BWD)
    for name, w, r in zip(('dgamma', 'dbeta', 'dzsum'), want[1:], ref[1:]):
        quarter_all('layernorm_bwd ' + name, w, r, G.BWD)
