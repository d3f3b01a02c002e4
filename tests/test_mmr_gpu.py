"""ops.mmr_rows (lime_mmr_rows_f32, csrc/mmr_rows_f32.hip) on the MI355X against ``recommend.mmr_select`` -- the host statement in
fp64, itself held against a literal per-round loop in test_mmr_cpu.py.

The kernel sums in fp32, so two checks (mmr_cases.py) stand in for bit equality on the clustered cases:
  1. greedy validity, every row: the kernel's OWN picks replayed through the fp64 statement -- each pick live, not repeated, and its
     fp64 v within tol of the round's best.  tol = 8 (E + 8) 2^-24: two cosines, each a dot product and two norms, under the worst-case
     fp32 summation bound (1.9e-4 at E = 400; the largest cosine error numpy's fp32 shows there is 1.3e-6).  Typical gaps between
     candidates are about 1e-2, so a wrong pick is far outside tol.
  2. exact equality of the picks on the rows whose fp64 minimum gap exceeds 2 tol, at E <= 400 and lam = 0.3; at least half of a
     case's rows must be such rows (asserted: a condition on the generator).
The exact cases of the CPU file -- one-hot rows, power-of-two spans: every v exact, the ties real -- are held bit for bit."""
import numpy as np
import pytest
import torch

from lime_cikm25_amd import recommend
from mmr_cases import check_exact, check_greedy, clustered, exact_groups, padded, tolerance

pytestmark = pytest.mark.gpu

# (M, E, R, k, lam): every M of {1, 2, 15, 16, 17, 64, 127, 128}, E of {4, 20, 400, 516}, R of {1, 3, 70}, k of {1, 10, M} and lam of
# {0, 0.3, 1} with the edge values of the others (16 entries: one row per lane group; 64: one wave's lanes; E = 20: a group's lanes
# partly idle; 516: not a multiple of the group's 64 floats per step)
CASES = [(1, 4, 1, 1, 0.3), (1, 516, 70, 1, 1.0), (2, 20, 3, 2, 0.3), (2, 4, 70, 1, 0.0), (15, 400, 3, 10, 0.3), (15, 4, 1, 15, 0.0),
         (16, 20, 70, 10, 0.3), (16, 516, 1, 16, 0.3), (17, 400, 1, 17, 0.3), (17, 4, 70, 10, 0.3), (17, 20, 3, 1, 1.0),
         (64, 400, 70, 10, 0.3), (64, 516, 3, 64, 0.0), (64, 4, 1, 1, 0.3), (127, 20, 1, 127, 0.3), (127, 516, 70, 10, 0.0),
         (127, 400, 3, 10, 0.3), (128, 400, 70, 10, 0.3), (128, 4, 3, 128, 0.3), (128, 516, 1, 128, 1.0), (128, 20, 70, 1, 0.0),
         (128, 400, 3, 128, 0.0), (128, 516, 3, 10, 0.3)]


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from lime_cikm25_amd import ops as _ops
    from lime_cikm25_amd import _lib
    _lib.load()
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(ops, scores, ids, table, lam, k):
    table = table if isinstance(table, torch.Tensor) else dev(table)
    picks = ops.mmr_rows(dev(scores), dev(ids), table, lam, k)
    assert picks.dtype == torch.int32 and tuple(picks.shape) == (scores.shape[0], k)
    return picks.cpu().numpy()


@pytest.mark.parametrize('case', range(len(CASES)), ids=['M%d-E%d-R%d-k%d-lam%g' % c for c in CASES])
def test_picks_are_greedy_and_equal_where_the_gap_is_clear(ops, case):
    M, E, R, k, lam = CASES[case]
    scores, ids, table = clustered(R, M, E, seed=100 + case)
    got, tol, what = run(ops, scores, ids, table, lam, k), tolerance(E), 'M %d E %d R %d k %d lam %g' % CASES[case]
    check_greedy(got, scores, ids, table, lam, tol, what)
    live = (ids >= 0) & (ids < table.shape[0]) & np.isfinite(scores)
    if lam == 1.0:                                                            # the plain order of the live entries, exactly
        for r in range(R):
            assert np.array_equal(got[r], padded(np.flatnonzero(live[r])[:k], k)), what
    if lam == 0.0:                                                            # `first` first
        assert np.array_equal(got[:, 0], [np.flatnonzero(l)[0] if l.any() else -1 for l in live]), what
    if k == M:                                                                # all of the live entries, then -1
        assert all(sorted(g[g >= 0].tolist()) == np.flatnonzero(l).tolist() for g, l in zip(got, live)), what
    if E <= 400 and lam == 0.3:
        want, gap = recommend.mmr_select(scores, ids, table, lam, k, return_gap=True)
        check_exact(got, want, gap, tol, what)


def test_the_exact_cases_bit_for_bit(ops):
    rows = 0
    for scores, ids, table, lam, k in exact_groups():
        assert np.array_equal(run(ops, scores, ids, table, lam, k), recommend.mmr_select(scores, ids, table, lam, k)), (rows, lam, k)
        rows += scores.shape[0]
    assert rows >= 1000


def test_a_row_does_not_feel_its_place_the_other_rows_or_the_run(ops):
    M, E, k, lam = 128, 400, 10, 0.3
    scores, ids, table = clustered(70, M, E, seed=7)
    t = dev(table)
    whole = run(ops, scores, ids, t, lam, k)
    assert np.array_equal(whole, run(ops, scores, ids, t, lam, k))            # two runs are equal
    for R, at in ((1, 0), (3, 2), (70, 41)):                                  # row 5 at three positions of three different R
        s, i = scores[:R].copy(), ids[:R].copy()
        s[at], i[at] = scores[5], ids[5]
        assert np.array_equal(run(ops, s, i, t, lam, k)[at], whole[5]), (R, at)


@pytest.mark.parametrize('E,lead,shift', [(20, 20, 0), (20, 20, 3), (400, 403, 0), (400, 800, 400), (8, 8, 1)])
def test_a_table_view_ending_at_its_buffers_end_reads_its_last_row_and_nothing_behind_it(ops, E, lead, shift):
    """The table is the tail of its buffer: the rows of leading dimension ``lead`` end where the buffer ends, ``shift`` floats into a
    16-byte unit -- the vector loads' form (aligned, lead % 4 == 0) and the scalar one.  Everything in front of the view is NaN."""
    M, k, lam, R = 17, 10, 0.3, 3
    scores, ids, table = clustered(R, M, E, seed=E + lead + shift, dead=0.0)
    n = table.shape[0]
    assert ids[0, 0] == n - 1
    front = 64 + shift
    buf = torch.full((front + (n - 1) * lead + E,), float('nan'), dtype=torch.float32, device='cuda')
    view = buf[front:].as_strided((n, E), (lead, 1))
    view.copy_(dev(table))
    assert view.data_ptr() + 4 * ((n - 1) * lead + E) == buf.data_ptr() + 4 * buf.numel()
    got = run(ops, scores, ids, view, lam, k)
    check_greedy(got, scores, ids, table, lam, tolerance(E), 'view E %d lead %d shift %d' % (E, lead, shift))
    want, gap = recommend.mmr_select(scores, ids, table, lam, k, return_gap=True)
    check_exact(got, want, gap, tolerance(E))


def test_ops_refuses_what_the_kernel_cannot_take(ops):
    s, i, t = torch.zeros(2, 8, device='cuda'), torch.zeros(2, 8, dtype=torch.int32, device='cuda'), torch.ones(4, 8, device='cuda')
    for bad in (lambda: ops.mmr_rows(s, i, t, 0.5, 9), lambda: ops.mmr_rows(s, i, t, 0.5, 0), lambda: ops.mmr_rows(s, i, t, 1.5, 2),
                lambda: ops.mmr_rows(s[:, :4], i[:, :4].contiguous(), t, 0.5, 2), lambda: ops.mmr_rows(s, i[:1], t, 0.5, 2)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.mmr_rows(s, i.long(), t, 0.5, 2)
    with pytest.raises(TypeError):
        ops.mmr_rows(s.cpu(), i, t, 0.5, 2)
    with pytest.raises(RuntimeError, match='lime_mmr_rows_f32'):              # the kernel's own limit: E % 4
        ops.mmr_rows(s, i, torch.ones(4, 6, device='cuda'), 0.5, 2)
    assert tuple(ops.mmr_rows(s[:0], i[:0], t, 0.5, 2).shape) == (0, 2)
