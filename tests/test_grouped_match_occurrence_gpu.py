"""lime_grouped_match_occurrence_f32 and lime_grouped_mlp_match_occurrence_f32 (csrc/grouped_match_f32.hip, csrc/grouped_mlp_match_f32.hip)
on the MI355X: pair p reads row index[p] of two news tables and row occ[p] of two occurrence tables and adds them while it loads its
operands.  Their statement is the plain kernel (lime_grouped_match_f32 / lime_grouped_mlp_match_f32) on rows composed with one torch
fp32 add, ``qa[index] + qt[occ]`` and ``ca[index] + ct[occ]`` (``na`` / ``nt`` under the MLP predictor), bit for bit (``torch.equal``
throughout); on top of that the independence of a pair's bits from the plan and from both tables' sizes and layouts, and the clamp of
an index or an occurrence id outside its table."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ALPHA, BETA = 0.3, 0.7
N_TABLE = 37
GROUPS = [0, 1, 64, 65, 130]              # pairs per group, in one call: empty, one, one full tile, one past it, three tiles
HS = [1, 7, 50, 128]                      # one per instantiation (16, 16, 64, 128 padded rows), none routed away: all are scratch-free
# (A, second width): the dot product's (A, D) -- CROWN-CROWN, a pooled user (H = 1: four zero columns) at D = 300, CROWN's Q on the
# content encoder's 900 columns -- and the MLP predictor's (A, Dh) with Dh = D // 2 of D = 300 and 900
SHAPES = {'dot': [(400, 400), (4, 300), (400, 900)], 'mlp': [(400, 150), (4, 150), (400, 450)]}
CASES = [(form, A, W) for form in ('dot', 'mlp') for A, W in SHAPES[form]]


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from lime_cikm25_amd import ops as _ops
    from lime_cikm25_amd import _lib
    _lib.load()
    return _ops


def make_ids(P, n, rng):
    """Row ids with repeats, a descending run from the last row, a run of one row and the last row of the table."""
    ids = rng.integers(0, n, size=P).astype(np.int32)
    run = min(P, n)
    ids[:run] = np.arange(n - 1, n - 1 - run, -1)
    if P > run + 8:
        ids[run:run + 8] = ids[run]
    ids[-1] = n - 1
    return ids


def make(H, A, W, sizes=GROUPS, n=N_TABLE, n_occ=100, seed=0):
    """kp [G H, A] and x [G H, W] (g or gu) per group; the news tables qa [n, A], va [n, W] and the occurrence tables qt [n_occ, A],
    vt [n_occ, W]; index, occ and remaining per pair; the MLP predictor's w_out [W] and b_out [1]."""
    rng = np.random.default_rng(seed)
    G, P = len(sizes), int(sum(sizes))
    u = lambda *s: rng.uniform(-1.0, 1.0, size=s).astype(np.float32)
    return dict(kp=u(G * H, A), x=u(G * H, W), qa=u(n, A), va=u(n, W), qt=u(n_occ, A), vt=u(n_occ, W), H=H,
                index=make_ids(P, n, rng), occ=make_ids(P, n_occ, rng), remaining=rng.uniform(-3.0, 3.0, size=P).astype(np.float32),
                offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), w_out=u(W), b_out=u(1))


def on_device(d):
    return {k: torch.from_numpy(v).cuda() for k, v in d.items() if k != 'H'}


def scale_of(A):
    return 1.0 / float(np.sqrt(np.float32(A)))


def run_occurrence(ops, form, t, H, tables=None, index=None, occ=None, n=None, n_occ=None):
    """The occurrence-composed entry on the device tensors t; ``tables`` = (qa, va, qt, vt) instead of t's."""
    qa, va, qt, vt = tables if tables is not None else (t['qa'], t['va'], t['qt'], t['vt'])
    index, occ = t['index'] if index is None else index, t['occ'] if occ is None else occ
    scale = scale_of(t['kp'].shape[1])
    if form == 'dot':
        return ops.grouped_match(t['kp'], t['x'], qa, va, t['remaining'], t['offsets'], H, scale, ALPHA, BETA, True, True, index=index, n=n,
                                 occ=occ, qt=qt, ct=vt, n_occ=n_occ)
    return ops.grouped_mlp_match(t['kp'], t['x'], qa, va, t['w_out'], t['b_out'], t['offsets'], H, scale, index=index, n=n, occ=occ, qt=qt,
                                 nt=vt, n_occ=n_occ)


def run_plain_on_composed(ops, form, t, H, index=None, occ=None):
    """The plain entry on rows composed with one torch fp32 add, a + t in that order."""
    i, o = (t['index'] if index is None else index).long(), (t['occ'] if occ is None else occ).long()
    qp, v = t['qa'][i] + t['qt'][o], t['va'][i] + t['vt'][o]
    scale = scale_of(t['kp'].shape[1])
    if form == 'dot':
        return ops.grouped_match(t['kp'], t['x'], qp, v, t['remaining'], t['offsets'], H, scale, ALPHA, BETA, True, True)
    return ops.grouped_mlp_match(t['kp'], t['x'], qp, v, t['w_out'], t['b_out'], t['offsets'], H, scale)


@pytest.mark.parametrize('n_occ', [4, 100])
@pytest.mark.parametrize('form,A,W', CASES)
@pytest.mark.parametrize('H', HS)
def test_bits_are_those_of_the_plain_kernel_on_the_composed_rows(ops, H, form, A, W, n_occ):
    t = on_device(make(H, A, W, n_occ=n_occ, seed=H + W + n_occ))
    got = run_occurrence(ops, form, t, H)
    want = run_plain_on_composed(ops, form, t, H)
    assert got.shape == (sum(GROUPS),) and torch.isfinite(got).all()
    assert torch.equal(got, want)


@pytest.mark.parametrize('form,A,W', [('dot', 400, 900), ('mlp', 400, 450)])
def test_a_pairs_bits_do_not_depend_on_the_plan_or_the_tables(ops, form, A, W):
    """The same pairs against larger tables that hold the same rows at other places, in another group order, in another order inside
    their group, behind a stranger group and under another P, G, n and n_occ."""
    H = 50
    d = make(H, A, W, seed=21)
    first = run_occurrence(ops, form, on_device(d), H).cpu().numpy()
    assert np.array_equal(first, run_occurrence(ops, form, on_device(d), H).cpu().numpy()), 'two runs differ'
    rng = np.random.default_rng(22)
    n2, n_occ2 = 97, 150
    place, place_occ = rng.permutation(n2)[:N_TABLE], rng.permutation(n_occ2)[:100]        # old row -> its row in the new tables
    stranger = make(H, A, W, sizes=[37], n=n2, n_occ=n_occ2, seed=23)
    tabs = {k: stranger[k].copy() for k in ('qa', 'va', 'qt', 'vt')}
    tabs['qa'][place], tabs['va'][place] = d['qa'], d['va']
    tabs['qt'][place_occ], tabs['vt'][place_occ] = d['qt'], d['vt']
    perm = [3, 1, 4, 0, 2]                                                 # new place -> old group
    sizes, rows = [37], []
    for i in perm:
        lo, hi = int(d['offsets'][i]), int(d['offsets'][i + 1])
        rows.append(rng.permutation(np.arange(lo, hi)))
        sizes.append(hi - lo)
    rows = np.concatenate(rows)
    grp = lambda name: np.concatenate([stranger[name]] + [d[name][i * H:(i + 1) * H] for i in perm])
    d2 = dict(tabs, kp=grp('kp'), x=grp('x'), H=H, w_out=d['w_out'], b_out=d['b_out'],
              index=np.concatenate([stranger['index'], place[d['index'][rows]].astype(np.int32)]),
              occ=np.concatenate([stranger['occ'], place_occ[d['occ'][rows]].astype(np.int32)]),
              remaining=np.concatenate([stranger['remaining'], d['remaining'][rows]]),
              offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    second = run_occurrence(ops, form, on_device(d2), H).cpu().numpy()
    assert second.shape[0] == first.shape[0] + 37
    assert np.array_equal(second[37:].view(np.int32), first[rows].view(np.int32))


@pytest.mark.parametrize('form,A,W', [('dot', 400, 900), ('mlp', 400, 450)])
def test_ids_outside_their_table_are_clamped_into_it(ops, form, A, W):
    """An index of n (and beyond) reads row n - 1 and a negative one row 0, and so does an occurrence id against n_occ -- on tables that
    lie inside larger allocations whose rows in front of and behind them hold NaN: a read outside a table would poison the pair."""
    H, n, n_occ = 7, N_TABLE, 100
    d = make(H, A, W, sizes=[5, 70], n_occ=n_occ, seed=31)
    top, low = np.iinfo(np.int32).max, np.iinfo(np.int32).min
    bad_i, bad_o = d['index'].copy(), d['occ'].copy()
    bad_i[0], bad_i[1], bad_i[2], bad_i[6], bad_i[74] = n, -1, top, low, n + 1000
    bad_o[0], bad_o[3], bad_o[4], bad_o[7], bad_o[73] = low, n_occ, -1, top, n_occ + 5         # (pair 0: both ids bad)
    fixed_i = np.clip(bad_i.astype(np.int64), 0, n - 1).astype(np.int32)
    fixed_o = np.clip(bad_o.astype(np.int64), 0, n_occ - 1).astype(np.int32)
    t = on_device(d)
    pad = 8                                                                # rows of NaN on either side (8 rows keep the 16-byte alignment)

    def inside_nan(x):
        big = torch.full((x.shape[0] + 2 * pad, x.shape[1]), float('nan'), device='cuda')
        big[pad:pad + x.shape[0]] = x
        return big[pad:pad + x.shape[0]]
    tables = tuple(inside_nan(t[k]) for k in ('qa', 'va', 'qt', 'vt'))
    dev = lambda a: torch.from_numpy(a).cuda()
    got = run_occurrence(ops, form, t, H, tables=tables, index=dev(bad_i), occ=dev(bad_o), n=n, n_occ=n_occ)
    want = run_occurrence(ops, form, t, H, tables=tables, index=dev(fixed_i), occ=dev(fixed_o), n=n, n_occ=n_occ)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)
    assert torch.equal(want, run_plain_on_composed(ops, form, t, H, index=dev(fixed_i), occ=dev(fixed_o)))
    # n and n_occ below the tables' rows: the clamp is against them, not against the allocation
    few = run_occurrence(ops, form, t, H, n=10, n_occ=3)
    assert torch.equal(few, run_plain_on_composed(ops, form, t, H, index=dev(np.minimum(d['index'], 9)), occ=dev(np.minimum(d['occ'], 2))))


def test_ops_check_the_occurrence_tables_on_the_host(ops):
    z = lambda *s: torch.zeros(*s, device='cuda')
    off = torch.tensor([0, 1], dtype=torch.int64, device='cuda')
    idx = torch.zeros(1, dtype=torch.int32, device='cuda')
    args = (z(4, 8), z(4, 8), z(3, 8), z(3, 8), None, off, 4, 1.0)
    with pytest.raises(ValueError, match='n_occ = 5'):
        ops.grouped_match(*args, index=idx, occ=idx, qt=z(2, 8), ct=z(2, 8), n_occ=5)
    with pytest.raises(ValueError, match='qt must be'):
        ops.grouped_match(*args, index=idx, occ=idx, qt=z(2, 4), ct=z(2, 8))
    with pytest.raises(ValueError, match='needs ct'):
        ops.grouped_match(*args, index=idx, occ=idx, qt=z(2, 8))
    with pytest.raises(ValueError, match='give index'):
        ops.grouped_match(*args, occ=idx, qt=z(2, 8), ct=z(2, 8))
    with pytest.raises(TypeError, match='occ'):
        ops.grouped_match(*args, index=idx, occ=idx.long(), qt=z(2, 8), ct=z(2, 8))
    mlp = (z(4, 8), z(4, 6), z(3, 8), z(3, 6), z(6), z(1), off, 4, 1.0)
    with pytest.raises(ValueError, match='nt must be'):
        ops.grouped_mlp_match(*mlp, index=idx, occ=idx, qt=z(2, 8), nt=z(2, 8))
    assert ops.grouped_mlp_match(*mlp, index=idx, occ=idx, qt=z(2, 8), nt=z(2, 6)).shape == (1,)
