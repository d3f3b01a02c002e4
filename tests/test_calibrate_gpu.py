"""ops.calibrate_rows (lime_calibrate_rows_f32) and ops.slate_miscalibration (lime_slate_miscalibration), csrc/calibrate_rows.hip, on the
MI355X against ``recommend.calibrated_select`` / ``recommend.slate_miscalibration`` -- the host statements in fp64, themselves held
against literal loops in test_calibrate_cpu.py.

The selection runs in fp32, so two checks (calibrate_cases.py) stand in for bit equality:
  1. greedy validity, every row: the kernel's OWN picks replayed through the fp64 statement -- each pick live, not repeated, and its
     fp64 v within tol of the round's best; tol = ``calibrate_cases.tolerance(H, alpha)``, derived from the arithmetic (DESIGN.md
     "Calibrated slates"; 2.0e-5 at H = 50, 4.7e-5 at H = 128, alpha = 0.01, with logf ASSUMED within 4 ulp);
  2. exact equality of the picks on the rows whose fp64 minimum gap exceeds 2 tol; on the shapes flagged in
     ``calibrate_cases.GPU_SHAPES`` at least 3/4 of the rows must be such rows (a condition on the inputs that the CPU suite asserts
     from the fp64 statement alone).
The metric is fp64 on both sides: values within ``calibrate_cases.metric_bound``, statuses equal."""
import numpy as np
import pytest
import torch

from lime_cikm25_amd import recommend
from calibrate_cases import GPU_SHAPES, case, check_exact, check_greedy, host_select, metric_bound, padded, sure_rows, tie_case, tolerance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from lime_cikm25_amd import ops as _ops
    from lime_cikm25_amd import _lib
    _lib.load()
    return _ops


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(ops, c, lam, alpha, k):
    picks = ops.calibrate_rows(dev(c['scores']), dev(c['ids']), dev(c['keys']), c['n_keys'], dev(c['hist_keys']), dev(c['weights']), lam, alpha, k)
    assert picks.dtype == torch.int32 and tuple(picks.shape) == (c['scores'].shape[0], k)
    return picks.cpu().numpy()


def held(ops, c, lam, alpha, k, what, share):
    """Both checks of one case -> the device's picks."""
    got = run(ops, c, lam, alpha, k)
    tol = tolerance(c['hist_keys'].shape[1], alpha)
    check_greedy(got, c, lam, alpha, tol, what)
    want, gap = host_select(c, lam, alpha, k)
    if share:
        check_exact(got, want, gap, tol, what)
    else:
        sure = sure_rows(gap, tol)
        assert np.array_equal(got[sure], want[sure]), what
    return got


@pytest.mark.parametrize('shape', GPU_SHAPES, ids=lambda s: 'R%d-M%d-H%d-n%d-k%d-lam%g' % s[:6])
def test_picks_are_greedy_and_equal_where_the_gap_is_clear(ops, shape):
    R, M, H, n_keys, k, lam, alpha, weighted, seed, share = shape
    c = case(R, M, H, n_keys, seed, weighted)
    got = held(ops, c, lam, alpha, k, 'R %d M %d H %d n_keys %d k %d lam %g' % shape[:6], share)
    if lam == 1.0 or H == 0:                                                  # the plain order of the live entries, exactly
        live = (c['ids'] >= 0) & (c['ids'] < c['keys'].shape[0]) & np.isfinite(c['scores'])
        for r in range(R):
            assert np.array_equal(got[r], padded(np.flatnonzero(live[r])[:k], k))


def test_lam_one_reads_neither_keys_nor_history(ops):
    """Keys and history keys full of out-of-range values, weights full of NaN: lam = 1 returns the live entries in order all the same."""
    c = case(9, 65, 6, 17, seed=21)
    c['keys'] = np.full_like(c['keys'], 2 ** 30)
    c['hist_keys'] = np.full_like(c['hist_keys'], -2 ** 31)
    c['weights'] = np.full(c['hist_keys'].shape, np.nan, dtype=np.float32)
    got = run(ops, c, 1.0, 0.01, 10)
    live = (c['ids'] >= 0) & (c['ids'] < c['keys'].shape[0]) & np.isfinite(c['scores'])
    for r in range(9):
        assert np.array_equal(got[r], padded(np.flatnonzero(live[r])[:10], 10))
    assert np.array_equal(run(ops, c, 0.3, 0.01, 10), got)                    # and with them no row has a target


def test_masked_histories_bad_weights_and_keys_out_of_range(ops):
    c = case(40, 64, 12, 17, seed=22, weighted=True)
    c['hist_keys'][::5] = -1                                                  # a history all masked: no target
    c['hist_keys'][1::5, ::2] = 17 + np.arange(6)                             # history keys out of range: no clicks
    c['weights'][2::5, ::3] = np.array([np.nan, -1.0, np.inf, 0.0], dtype=np.float32)
    c['weights'][3::5] = 0.0                                                  # every slot removed: no target
    got = held(ops, c, 0.3, 0.01, 10, 'masked', share=True)
    plain = run(ops, c, 1.0, 0.01, 10)
    assert np.array_equal(got[::5], plain[::5]) and np.array_equal(got[3::5], plain[3::5]) and not np.array_equal(got, plain)


def test_rows_share_histories_by_their_position_modulo_hist_rows(ops):
    c = case(6, 64, 20, 17, seed=23, hist_rows=3)
    assert c['hist_keys'].shape[0] == 3
    got = held(ops, c, 0.3, 0.01, 10, 'hist_rows 3 under R 6', share=True)
    wide = dict(c, hist_keys=np.concatenate([c['hist_keys']] * 2))
    assert np.array_equal(run(ops, wide, 0.3, 0.01, 10), got)


@pytest.mark.parametrize('lam', [0.0, 0.3])
def test_structural_ties_come_out_in_rank_order_bit_for_bit(ops, lam):
    """Scores from four values and three groups: two entries of one group with equal score bits carry the same v bits on the device as
    they do on the host, and the lower rank wins; the classes themselves lie far apart, so the picks are the statement's."""
    c = tie_case(64, 48, 10, 3, seed=24)
    got = run(ops, c, lam, 0.01, 48)
    check_greedy(got, c, lam, 0.01, tolerance(10, 0.01), 'ties')
    want, gap = host_select(c, lam, 0.01, 48)
    ties = 0
    for r in range(64):
        took = [int(j) for j in got[r] if j >= 0]
        cls = [(int(c['keys'][c['ids'][r, j]]), float(c['scores'][r, j])) for j in took]
        first = {}
        for at, (j, kind) in enumerate(zip(took, cls)):
            if kind in first:
                ties += 1
                assert first[kind] < j, (r, kind, first[kind], j)             # equal (group, score): in rank order
            first[kind] = j
    assert ties > 500
    if lam > 0:
        sure = sure_rows(gap, tolerance(10, 0.01))
        assert 2 * int(sure.sum()) >= 64 and np.array_equal(got[sure], want[sure])


def test_a_row_depends_on_its_own_operands_alone(ops):
    """70,000 rows of M = 8, H = 4 (the grid strides): 500 distinct rows, tiled -- every copy of a row gives the same picks, the
    statement's on the sure rows; the same rows at R = 3, 5 and 257 and in a second run give the same bits."""
    base = case(500, 8, 4, 5, seed=25, weighted=True)
    reps = 140
    big = dict(base, scores=np.tile(base['scores'], (reps, 1)), ids=np.tile(base['ids'], (reps, 1)),
               hist_keys=np.tile(base['hist_keys'], (reps, 1)), weights=np.tile(base['weights'], (reps, 1)))
    got = run(ops, big, 0.3, 0.01, 4)
    assert got.shape == (70000, 4) and np.array_equal(got, np.tile(got[:500], (reps, 1)))
    assert np.array_equal(run(ops, big, 0.3, 0.01, 4), got)                   # across two runs
    tol = tolerance(4, 0.01)
    check_greedy(got[:500], base, 0.3, 0.01, tol, 'R 70000')
    want, gap = host_select(base, 0.3, 0.01, 4)
    check_exact(got[:500], want, gap, tol, 'R 70000')
    for R, at in ((3, (0, 1, 2)), (5, (0, 2, 4)), (257, (0, 128, 256))):      # three positions of three R
        rows = np.array([7, 77, 499])
        part = {key: (np.repeat(base[key][:1], R, axis=0) if key in ('scores', 'ids', 'hist_keys', 'weights') else base[key]) for key in base}
        for key in ('scores', 'ids', 'hist_keys', 'weights'):
            part[key] = part[key].copy()
            part[key][list(at)] = base[key][rows]
        assert np.array_equal(run(ops, part, 0.3, 0.01, 4)[list(at)], got[rows]), R
    empty = {key: (base[key][:0] if key in ('scores', 'ids') else base[key]) for key in base}
    assert run(ops, empty, 0.3, 0.01, 4).shape == (0, 4)                      # R = 0: no call


# ---- the metric ----------------------------------------------------------------------------------------------------------------------
def slates(seed, R, k, ldp, H, lists, weighted, n=60, n_keys=7):
    rng = np.random.default_rng(seed)
    lens = rng.choice([0, 1, 3, 9, 40, 150], size=R) if lists else None       # lists shorter than k, and empty
    P = int(lens.sum()) if lists else 140
    c = dict(k=k, offsets=np.r_[0, np.cumsum(lens)].astype(np.int64) if lists else None, news=rng.integers(-1, n + 2, size=max(P, 1)).astype(np.int32)[:P],
             keys=rng.integers(-1, n_keys + 1, size=n).astype(np.int32), n_keys=n_keys,
             positions=rng.integers(-1, 150, size=(R, ldp)).astype(np.int32), hist_keys=rng.integers(-1, n_keys, size=(R, H)).astype(np.int32),
             weights=rng.choice(np.array([0, 0.25, 0.5, 1.0, np.nan, -1.0], dtype=np.float32), size=(R, H)) if weighted else None)
    if lists:                                                                 # most slots filled where the list has rows
        c['positions'] = np.where(rng.random((R, ldp)) < 0.8, rng.integers(0, 150, size=(R, ldp)) % np.maximum(lens, 1)[:, None], c['positions']).astype(np.int32)
    c['hist_keys'][::7] = -1
    c['positions'][3::11] = -1
    return c


@pytest.mark.parametrize('k,ldp,H,lists,weighted,alpha', [(1, 1, 6, True, False, 0.01), (10, 13, 50, True, True, 0.01), (16, 16, 64, False, False, 0.1),
                                                         (17, 20, 65, True, True, 0.01), (128, 128, 128, False, True, 0.01),
                                                         (128, 130, 1, True, False, 0.1), (10, 10, 0, True, False, 0.01)])
def test_miscalibration_is_the_statement(ops, k, ldp, H, lists, weighted, alpha):
    c = slates(30 + k, 257, k, ldp, H, lists, weighted)
    a32 = float(np.float32(alpha))                                            # the entry reads alpha as the fp32 number the selection reads
    want_v, want_s = recommend.slate_miscalibration(c['positions'], k, c['offsets'], c['news'], c['keys'], c['n_keys'], c['hist_keys'],
                                                    c['weights'], a32)
    wide = dev(c['positions'])
    value, status = ops.slate_miscalibration(wide, k, dev(c['offsets']), dev(c['news']), dev(c['keys']), c['n_keys'], dev(c['hist_keys']),
                                             dev(c['weights']), alpha)
    assert value.dtype == torch.float64 and status.dtype == torch.int32 and tuple(value.shape) == (257,)
    assert np.array_equal(status.cpu().numpy(), want_s) and (sorted(set(want_s.tolist())) == [0, 1, 2] or H == 0)
    err = np.abs(value.cpu().numpy() - want_v).max()
    print('k %d H %d: max |device - host| = %.3g, bound %.3g' % (k, H, err, metric_bound(H, alpha)))
    assert err <= metric_bound(H, alpha) and (value.cpu().numpy()[want_s != 0] == 0).all()
    if ldp > 3:                                                               # a prefix of a wider positions, in place
        lo_v, lo_s = ops.slate_miscalibration(wide[:, :3], 3, dev(c['offsets']), dev(c['news']), dev(c['keys']), c['n_keys'], dev(c['hist_keys']),
                                              dev(c['weights']), alpha)
        own_v, own_s = ops.slate_miscalibration(wide[:, :3].contiguous(), 3, dev(c['offsets']), dev(c['news']), dev(c['keys']), c['n_keys'],
                                                dev(c['hist_keys']), dev(c['weights']), alpha)
        assert torch.equal(lo_v, own_v) and torch.equal(lo_s, own_s)
    again = ops.slate_miscalibration(wide, k, dev(c['offsets']), dev(c['news']), dev(c['keys']), c['n_keys'], dev(c['hist_keys']), dev(c['weights']), alpha)
    assert torch.equal(again[0], value) and torch.equal(again[1], status)     # across two runs
