"""lime_grouped_match_indexed_f32 (csrc/grouped_match_f32.hip) on the MI355X: pair p reads row index[p] of a qp table [n, A] and of a
cand table [n, D].  Its statement is lime_grouped_match_f32 on the gathered rows, bit for bit (``torch.equal``); on top of that the
float64 rule of tests/test_grouped_match_gpu.py (twice lime_interest_match_f32's own error plus one ulp of the largest |logit|), the
independence of a pair's bits from the table's size, the row's place in it, P and G, the clamp of an index outside the table, and the
statuses of the arguments it refuses before any launch."""
import numpy as np
import pytest
import torch

from test_grouped_match_gpu import ALPHA, BETA, reference, run_old

pytestmark = pytest.mark.gpu

N_TABLE = 40
GROUPS = [0, 1, 64, 65, 130]              # pairs per group, in one call: empty, one, one full tile, one past it, three tiles
SHAPES = [(400, 900), (4, 300), (400, 400)]          # (A, D): CROWN-CROWN, a pooled user (H = 1: four zero columns) at D = 300, NAML's width


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from lime_cikm25_amd import ops as _ops
    from lime_cikm25_amd import _lib
    _lib.load()
    return _ops


def make_index(P, n, seed):
    """An index with repeats, a descending run, a run of one row and the last row of the table."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n, size=P).astype(np.int32)
    run = min(P, n)
    idx[:run] = np.arange(n - 1, n - 1 - run, -1)                          # descending from the last row
    if P > run + 8:
        idx[run:run + 8] = idx[run]                                        # the same row eight times
    idx[-1] = n - 1
    return idx


def make(H, A, D, sizes=GROUPS, n=N_TABLE, seed=0):
    rng = np.random.default_rng(seed)
    G, P = len(sizes), int(sum(sizes))
    u = lambda *s: rng.uniform(-1.0, 1.0, size=s).astype(np.float32)
    return dict(kp=u(G * H, A), g=u(G * H, D), qp_table=u(n, A), cand_table=u(n, D), H=H, index=make_index(P, n, seed + 1),
                remaining=rng.uniform(-3.0, 3.0, size=P).astype(np.float32), offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))


def gathered(d):
    """The plain form's inputs: the tables' rows, one per pair."""
    out = {k: v for k, v in d.items() if k not in ('qp_table', 'cand_table', 'index')}
    out['qp'], out['cand'] = d['qp_table'][d['index']], d['cand_table'][d['index']]
    return out


def scale_of(A):
    return 1.0 / float(np.sqrt(np.float32(A)))


def run_indexed(ops, d, use_weight=True, use_penalty=True, n=None):
    t = {k: torch.from_numpy(v).cuda() for k, v in d.items() if k != 'H'}
    return ops.grouped_match(t['kp'], t['g'], t['qp_table'], t['cand_table'], t['remaining'], t['offsets'], d['H'], scale_of(d['kp'].shape[1]),
                             ALPHA, BETA, use_weight, use_penalty, index=t['index'], n=n)


def run_plain(ops, d, use_weight=True, use_penalty=True):
    t = {k: torch.from_numpy(v).cuda() for k, v in d.items() if k != 'H'}
    return ops.grouped_match(t['kp'], t['g'], t['qp'], t['cand'], t['remaining'], t['offsets'], d['H'], scale_of(d['kp'].shape[1]),
                             ALPHA, BETA, use_weight, use_penalty)


@pytest.mark.parametrize('A,D', SHAPES)
@pytest.mark.parametrize('H', [1, 7, 50, 128])
def test_bits_are_those_of_the_plain_kernel_on_the_gathered_rows(ops, H, A, D):
    d = make(H, A, D, seed=H + D)
    got = run_indexed(ops, d)
    want = run_plain(ops, gathered(d))
    assert got.shape == (sum(GROUPS),) and torch.isfinite(got).all()
    assert torch.equal(got, want)
    assert torch.equal(run_indexed(ops, d, False, False), run_plain(ops, gathered(d), False, False))


@pytest.mark.parametrize('A,D', SHAPES)
@pytest.mark.parametrize('H', [1, 7, 50, 128])
def test_sizes_against_float64(ops, H, A, D):
    """The rule of tests/test_grouped_match_gpu.py::test_sizes_against_float64, with both errors measured here, on these inputs."""
    d = make(H, A, D, seed=3 * H + A)
    flat = gathered(d)
    want = reference(flat, True, True)
    new = run_indexed(ops, d).cpu().numpy()
    old = run_old(ops, flat, True, True).cpu().numpy()
    assert np.isfinite(new).all()
    e_new, e_old = float(np.abs(new - want).max()), float(np.abs(old - want).max())
    ulp = float(np.spacing(np.float32(np.abs(want).max())))
    print('H %d A %d D %d: indexed grouped match max err %.3e, interest match max err %.3e, one ulp of max |logit| %.3e (bound %.3e)' % (
        H, A, D, e_new, e_old, ulp, 2 * e_old + ulp))
    assert e_new <= 2 * e_old + ulp


def test_a_pairs_bits_do_not_depend_on_the_layout(ops):
    """The same pairs against a larger table that holds the same rows at other places, in another group order, in another order inside
    their group, behind a stranger group and under another P and G."""
    H, A, D = 50, 400, 900
    d = make(H, A, D, seed=21)
    first = run_indexed(ops, d).cpu().numpy()
    assert np.array_equal(first, run_indexed(ops, d).cpu().numpy()), 'two runs differ'
    rng = np.random.default_rng(22)
    # a table of 97 rows: the 40 old rows scattered over it, strangers between them
    n2 = 97
    place = rng.permutation(n2)[:N_TABLE]                                  # old row -> its row in the new table
    stranger = make(H, A, D, sizes=[37], n=n2, seed=23)
    qp2, cand2 = stranger['qp_table'].copy(), stranger['cand_table'].copy()
    qp2[place], cand2[place] = d['qp_table'], d['cand_table']
    perm = [3, 1, 4, 0, 2]                                                 # new place -> old group
    sizes, rows = [37], []
    for i in perm:
        lo, hi = int(d['offsets'][i]), int(d['offsets'][i + 1])
        rows.append(rng.permutation(np.arange(lo, hi)))
        sizes.append(hi - lo)
    rows = np.concatenate(rows)
    grp = lambda name: np.concatenate([stranger[name]] + [d[name][i * H:(i + 1) * H] for i in perm])
    d2 = dict(kp=grp('kp'), g=grp('g'), qp_table=qp2, cand_table=cand2, H=H,
              index=np.concatenate([stranger['index'], place[d['index'][rows]].astype(np.int32)]),
              remaining=np.concatenate([stranger['remaining'], d['remaining'][rows]]),
              offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    second = run_indexed(ops, d2).cpu().numpy()
    assert second.shape[0] == first.shape[0] + 37
    assert np.array_equal(second[37:].view(np.int32), first[rows].view(np.int32))


def test_an_index_outside_the_table_is_clamped_into_it(ops):
    """The documented behaviour: an index of n (and beyond) reads row n - 1, a negative one row 0 -- on a table that lies inside a
    larger allocation whose rows in front of and behind it hold NaN: a read outside the table would poison the pair."""
    H, A, D, n = 7, 400, 900, N_TABLE
    d = make(H, A, D, sizes=[5, 70], seed=31)
    bad = d['index'].copy()
    bad[0], bad[1], bad[2], bad[6], bad[74] = n, -1, np.iinfo(np.int32).max, np.iinfo(np.int32).min, n + 1000
    fixed = np.clip(bad.astype(np.int64), 0, n - 1).astype(np.int32)
    t = {k: torch.from_numpy(v).cuda() for k, v in d.items() if k != 'H'}
    pad = 8                                                                # rows of NaN on either side (8 rows keep the 16-byte alignment)
    big_q = torch.full((n + 2 * pad, A), float('nan'), device='cuda')
    big_c = torch.full((n + 2 * pad, D), float('nan'), device='cuda')
    big_q[pad:pad + n], big_c[pad:pad + n] = t['qp_table'], t['cand_table']
    run = lambda idx: ops.grouped_match(t['kp'], t['g'], big_q[pad:pad + n], big_c[pad:pad + n], t['remaining'], t['offsets'], H, scale_of(A),
                                        ALPHA, BETA, True, True, index=torch.from_numpy(idx).cuda(), n=n)
    got, want = run(bad), run(fixed)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)
    d_fixed = dict(d, index=fixed)
    assert torch.equal(want, run_plain(ops, gathered(d_fixed)))
    # n below the tables' rows: the clamp is against n, not against the allocation
    few = ops.grouped_match(t['kp'], t['g'], t['qp_table'], t['cand_table'], t['remaining'], t['offsets'], H, scale_of(A), ALPHA, BETA, True, True,
                            index=t['index'], n=10)
    assert torch.equal(few, run_plain(ops, gathered(dict(d, index=np.minimum(d['index'], 9)))))


def test_bad_arguments_return_their_status_without_a_launch(ops):
    from lime_cikm25_amd import _lib
    lib = _lib.load()
    z = lambda *s: torch.zeros(*s, device='cuda')
    off = torch.tensor([0, 1], dtype=torch.int64, device='cuda')
    idx = torch.zeros(1, dtype=torch.int32, device='cuda')

    def call(H, A, D, n=1, P=1, qp=None, index=idx, use_weight=0):
        kp, g, cand, out = z(H, A), z(H, D), z(max(n, 1), D), torch.full((max(P, 1),), 7.0, device='cuda')
        qp = z(max(n, 1), A) if qp is None else qp
        st = lib.lime_grouped_match_indexed_f32(kp.data_ptr(), g.data_ptr(), qp.data_ptr() if isinstance(qp, torch.Tensor) else qp,
                                                cand.data_ptr(), None, off.data_ptr(), index.data_ptr() if index is not None else None, n,
                                                out.data_ptr(), 1, P, H, A, D, 1.0, 0.0, 0.0, use_weight, 0, None)
        torch.cuda.synchronize()
        return st, out

    for H, A, D in ((129, 8, 8), (4, 2052, 8), (4, 8, 2052), (4, 6, 8)):
        st, out = call(H, A, D)
        assert st == -2 and float(out[0]) == 7.0, (H, A, D, st)            # LIME_ERR_UNSUPPORTED, nothing written
    st, out = call(4, 8, 8, n=0)                                           # pairs that index an empty table
    assert st == -1 and float(out[0]) == 7.0
    assert b'empty table' in lib.lime_last_error_string()
    assert call(4, 8, 8, n=0, P=0)[0] == 0                                 # ... no pairs: nothing to read
    assert call(4, 8, 8, n=-1)[0] == -1
    assert call(4, 8, 8, index=None)[0] == -1                              # NULL index
    assert call(4, 8, 8, use_weight=1)[0] == -1                            # weight without remaining
    st, out = call(4, 8, 8, qp=z(8, 8).data_ptr() + 4)                     # a table off the 16-byte grid
    assert st == -1 and float(out[0]) == 7.0
    st, out = call(4, 8, 8)
    assert st == 0 and float(out[0]) == 0.0                                # the same call with good arguments does launch
    with pytest.raises(ValueError, match='n = 5'):
        ops.grouped_match(z(4, 8), z(4, 8), z(3, 8), z(3, 8), None, off, 4, 1.0, index=idx, n=5)
    with pytest.raises(TypeError, match='index'):
        ops.grouped_match(z(4, 8), z(4, 8), z(3, 8), z(3, 8), None, off, 4, 1.0, index=idx.long())
