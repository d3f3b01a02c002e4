"""Case builders shared by the calibration tests (test_calibrate_cpu.py, test_calibrate_gpu.py, test_recommend_calibrated_gpu.py): the
literal per-round loop that ``recommend.calibrated_select`` is held against -- it evaluates the FULL objective lam rel - (1 - lam)
KL(p || q~ with the candidate added) / ln(1 / alpha) for every candidate, so it holds the incremental-KL identity as well as the
code --; the literal miscalibration; histories with a few favourite groups; the tolerances, derived from the arithmetic (DESIGN.md
"Calibrated slates"); and the two checks every device result is held to: greedy validity and exact equality on well-separated rows."""
import math

import numpy as np

from mmr_cases import clustered

TIE = 1e-12          # the literal loop's "equal": its full KL and the statement's gain differ by fp64 rounding, far below this


def literal_target(hist_keys, weights, n_keys):
    """{group: p} of one history row in Python floats, slot by slot; {} without a target."""
    total, sums = 0.0, {}
    for h, g in enumerate(hist_keys):
        w = 1.0 if weights is None else float(weights[h])
        if 0 <= g < n_keys and math.isfinite(w) and w > 0:
            total += w
            sums[int(g)] = sums.get(int(g), 0.0) + w
    if not (total > 0 and math.isfinite(total)):
        return {}
    return {g: v / total for g, v in sums.items()}


def literal_kl(p, counts, T, alpha):
    """KL(p || (1 - alpha) counts / T + alpha p) over p's support, a term at a time."""
    return sum(pg * math.log(pg / ((1.0 - alpha) * counts.get(g, 0) / T + alpha * pg)) for g, pg in p.items() if pg > 0)


def literal_values(s, ids, keys, n_keys, hist_keys, weights, lam, alpha, taken):
    """{j: v[j]} over the live, untaken entries of the round after ``taken``: the FULL lam rel - (1 - lam) KL(p || q~ with j added) /
    ln(1 / alpha), one entry at a time, in Python floats."""
    n, M = len(keys), len(s)
    live = [j for j in range(M) if 0 <= ids[j] < n and math.isfinite(s[j])]
    if not live:
        return {}
    span = float(s[live[0]]) - float(s[live[-1]])
    p = literal_target(hist_keys, weights, n_keys)
    counts = {}
    for j in taken:
        g = int(keys[ids[j]])
        if 0 <= g < n_keys:
            counts[g] = counts.get(g, 0) + 1
    values = {}
    for j in live:
        if j in taken:
            continue
        rel = 0.0 if span == 0.0 else (float(s[j]) - float(s[live[-1]])) / span
        g = int(keys[ids[j]])
        with_j = dict(counts)
        if 0 <= g < n_keys:
            with_j[g] = with_j.get(g, 0) + 1
        values[j] = lam * rel - (1.0 - lam) * (literal_kl(p, with_j, len(taken) + 1, alpha) / math.log(1.0 / alpha) if p else 0.0)
    return values


def literal_calibrated(s, ids, keys, n_keys, hist_keys, weights, lam, alpha, k):
    """Calibrated greedy selection as the words state it, one entry and one round at a time -> the ranks in the order taken."""
    taken = []
    while len(taken) < k:
        best, best_v = None, None
        for j, v in sorted(literal_values(s, ids, keys, n_keys, hist_keys, weights, lam, alpha, taken).items()):
            if best is None or v > best_v + TIE:                             # a later entry needs MORE: the lower rank wins ties
                best, best_v = j, v
        if best is None:
            break
        taken.append(best)
    return taken


def literal_miscalibration(slot_keys, hist_keys, weights, n_keys, alpha):
    """(value, status) of one slate from the keys of its FILLED slots (-1: a filled slot without a group)."""
    p = literal_target(hist_keys, weights, n_keys)
    if not p:
        return 0.0, 1
    if len(slot_keys) == 0:
        return 0.0, 2
    counts = {}
    for g in slot_keys:
        counts[int(g)] = counts.get(int(g), 0) + 1
    return literal_kl(p, counts, len(slot_keys), alpha), 0


def padded(taken, k):
    return np.array(list(taken) + [-1] * (k - len(taken)), dtype=np.int32)


# ---- case builders ---------------------------------------------------------------------------------------------------------------------
WEIGHTS = np.array([0.0, 0.25, 0.5, 1.0], dtype=np.float32)


def histories(R, H, pool, seed, weighted=False, masked=0.2):
    """R histories of H slots drawn from 1 to 4 favourite groups (of ``pool``) each, ``masked`` of the slots -1; ``weighted``: weights
    from {0, 0.25, 0.5, 1} -> (hist_keys int32 [R, H], weights fp32 [R, H] or None)."""
    rng = np.random.default_rng(seed)
    hk = np.full((R, H), -1, dtype=np.int32)
    for r in range(R):
        fav = rng.choice(pool, size=min(len(pool), int(rng.integers(1, 5))), replace=False)
        hk[r] = rng.choice(fav, size=H, p=rng.dirichlet(np.ones(len(fav)) * 2.0)) if H else hk[r]
    hk[rng.random((R, H)) < masked] = -1
    return hk, (rng.choice(WEIGHTS, size=(R, H)).astype(np.float32) if weighted else None)


def case(R, M, H, n_keys, seed, weighted=False, n=None, hist_rows=None):
    """Shortlists as ``mmr_cases.clustered`` makes them (descending scores, dead entries of every kind), the news' keys -- from a
    pool of at most 12 of the n_keys groups, the last group among them, a few keys outside [0, n_keys) --, and histories over the same
    pool -> dict(scores, ids, keys, n_keys, hist_keys, weights)."""
    scores, ids, table = clustered(R, M, 4, seed, n=n)
    rng = np.random.default_rng(seed + 7919)
    pool = np.unique(np.r_[rng.choice(n_keys, size=min(n_keys, 12), replace=False), n_keys - 1])
    keys = rng.choice(pool, size=table.shape[0]).astype(np.int32)
    keys[rng.random(keys.shape[0]) < 0.05] = rng.choice([-1, n_keys, n_keys + 3])
    hk, w = histories(R if hist_rows is None else hist_rows, H, pool, seed + 1, weighted)
    return dict(scores=scores, ids=ids, keys=keys, n_keys=n_keys, hist_keys=hk, weights=w)


def tie_case(R, M, H, n_keys, seed):
    """Scores from four values and few groups: two entries of one group with equal score bits -- the structural tie -- are frequent."""
    c = case(R, M, H, n_keys, seed)
    rng = np.random.default_rng(seed + 31)
    live = np.isfinite(c['scores'])
    c['scores'] = np.where(live, -np.sort(-rng.choice(np.array([0.5, 1.0, 1.5, 3.0], dtype=np.float32), size=(R, M)), axis=1), c['scores'])
    return c


# ---- tolerances, from the arithmetic ---------------------------------------------------------------------------------------------------
LOGF_ULP = 4.0       # ASSUMED: the installation carries no HIP math accuracy table; 4 ulp is above every figure published for logf / log


def tolerance(H, alpha, log_ulp=LOGF_ULP):
    """A bound on the fp32 kernel's error in the DIFFERENCE of two v, in units of u = 2^-24 (DESIGN.md "Calibrated slates"):
    lam rel: 5 u (three roundings of rel, lam's own, the product).  p: a sum of up to H terms over a sum of up to H terms, 2 H u.
    q: its two terms carry 3.5 u and (2 H + 2) u, the sum one more: (2 H + 3) u relative.  Each log: q's relative error plus
    2 log_ulp u |ln q|, |ln q| <= ln(1 / (alpha p)); times p / ln(1 / alpha), with p ln(1 / (alpha p)) / ln(1 / alpha) <= kappa =
    1 + 1 / (e ln(1 / alpha)).  The gain's own difference, two products and the rounded 1 / ln(1 / alpha): 4 u.  The fma: 2 u."""
    u, L = 2.0 ** -24, math.log(1.0 / alpha)
    kappa = 1.0 + 1.0 / (math.e * L)
    dp = 2.0 * max(H, 1)
    gain = dp + 4.0 + 2.0 * (2.0 * log_ulp * kappa) + 2.0 * (dp + 3.0) / L
    return 2.0 * (max(5.0, gain) + 2.0) * u


def metric_bound(H, alpha, log_ulp=LOGF_ULP):
    """A bound on |device - host| of the fp64 miscalibration, u = 2^-53, each side allowed the same error: per term p (2 H u), the
    ratio's denominator ((2 H + 3) u) and division (u) inside a log of slope 1, the log's own 2 log_ulp u |ln|, the product u; the
    terms' absolute values sum to at most B = ln(1 / alpha) + ln(max(H, 1)), and the sequential sum adds H u B."""
    u = 2.0 ** -53
    B = math.log(1.0 / alpha) + math.log(max(H, 1))
    return 2.0 * u * ((3.0 * max(H, 1) + 2.0 * log_ulp + 1.0) * B + 4.0 * max(H, 1) + 4.0)


# ---- the checks ------------------------------------------------------------------------------------------------------------------------
def round_values(rel, at, pe, counts, T, lam, alpha):
    """The fp64 v of every entry in a round: ``at`` the entry's support group (-1: none), ``pe`` its p, ``counts`` per support group."""
    ce = np.where(at >= 0, counts[np.maximum(at, 0)], 0.0)
    has = pe > 0
    q1 = np.where(has, (1.0 - alpha) * (ce + 1.0) / T + alpha * pe, 1.0)
    q0 = np.where(has, (1.0 - alpha) * ce / T + alpha * pe, 1.0)
    return lam * rel + (1.0 - lam) * pe * (np.log(q1) - np.log(q0)) / math.log(1.0 / alpha)


def check_greedy(picks, c, lam, alpha, tol, what=''):
    """Greedy validity of the device's OWN picks, replayed through the fp64 statement: every pick is live and not repeated, its fp64 v
    is within ``tol`` of the best fp64 v among the live untaken entries of its round, and -1 stands only where none is left."""
    from lime_cikm25_amd.recommend import calibration_target
    scores, ids, keys = np.asarray(c['scores'], dtype=np.float64), c['ids'], np.asarray(c['keys']).astype(np.int64)
    hk, w = c['hist_keys'], c['weights']
    for r in range(scores.shape[0]):
        live = (ids[r] >= 0) & (ids[r] < keys.shape[0]) & np.isfinite(scores[r])
        idx = np.flatnonzero(live)
        rel = np.zeros(len(live))
        if idx.size and scores[r, idx[0]] != scores[r, idx[-1]]:
            rel[idx] = (scores[r, idx] - scores[r, idx[-1]]) / (scores[r, idx[0]] - scores[r, idx[-1]])
        hr = r % hk.shape[0] if hk.shape[1] else 0
        groups, p = calibration_target(hk[hr] if hk.shape[1] else [], c['n_keys'], None if w is None or not hk.shape[1] else w[hr])
        at, pe = np.full(len(live), -1, dtype=np.int64), np.zeros(len(live))
        if groups.size and idx.size:
            key = keys[ids[r, idx]]
            g = np.minimum(np.searchsorted(groups, key), groups.size - 1)
            at[idx] = np.where(groups[g] == key, g, -1)
            pe = np.where(at >= 0, p[np.maximum(at, 0)], 0.0)
        counts, open_ = np.zeros(max(groups.size, 1)), live.copy()
        for t, j in enumerate(picks[r]):
            if j < 0:
                assert not open_.any() and (picks[r, t:] == -1).all(), '%s row %d round %d: -1 with live entries left' % (what, r, t)
                break
            assert 0 <= j < len(live) and open_[j], '%s row %d round %d: pick %d is dead or repeated' % (what, r, t, j)
            v = round_values(rel, at, pe, counts, t + 1.0, lam, alpha)
            assert v[j] >= v[open_].max() - tol, '%s row %d round %d: v[%d] = %.9g, best %.9g, tol %.3g' % (what, r, t, j, v[j],
                                                                                                           v[open_].max(), tol)
            open_[j] = False
            if at[j] >= 0:
                counts[at[j]] += 1.0


def sure_rows(gap, tol):
    return gap > 2.0 * tol


def check_exact(picks, want, gap, tol, what=''):
    """Exact equality with ``calibrated_select``'s picks on the rows whose fp64 minimum gap exceeds 2 tol; at least 3/4 of the rows
    must be such rows (a condition on the inputs, asserted on the CPU for every case the device tests use) -> the rows compared."""
    sure = sure_rows(gap, tol)
    assert 4 * int(sure.sum()) >= 3 * len(gap), '%s: only %d of %d rows have a minimum gap above 2 tol = %.3g' % (what, sure.sum(), len(gap), 2 * tol)
    assert np.array_equal(picks[sure], want[sure]), '%s: rows %s differ' % (what, np.flatnonzero(sure & (picks != want).any(axis=1))[:8])
    return int(sure.sum())


def host_select(c, lam, alpha, k):
    from lime_cikm25_amd.recommend import calibrated_select
    return calibrated_select(c['scores'], c['ids'], c['keys'], c['n_keys'], c['hist_keys'], c['weights'], lam, alpha, k, return_gap=True)


# The shapes of tests/test_calibrate_gpu.py, here so that the CPU suite asserts their share of sure rows from the fp64 statement alone:
# (R, M, H, n_keys, k, lam, alpha, weighted, seed, share) -- ``share``: at least 3/4 of the rows are sure rows.  Not so at lam = 0, where
# v is the gain alone and every entry of a group ties with every other whatever its score, nor where k = M walks into the tail.
GPU_SHAPES = [
    (200, 64, 50, 17, 10, 0.5, 0.01, False, 1, True), (200, 128, 50, 270, 10, 0.7, 0.01, True, 2, True),
    (200, 12, 6, 5, 5, 0.3, 0.01, False, 3, True), (200, 64, 128, 17, 16, 0.5, 0.01, True, 4, True),
    (5, 1, 1, 1, 1, 0.3, 0.01, False, 5, True), (5, 2, 6, 17, 2, 0.0, 0.1, True, 6, False), (257, 63, 64, 17, 10, 0.3, 0.1, False, 7, True),
    (3, 65, 65, 8192, 65, 0.3, 0.01, True, 8, False), (5, 128, 128, 17, 128, 0.0, 0.01, False, 9, False),
    (1, 64, 0, 17, 1, 0.3, 0.01, False, 10, True), (257, 65, 6, 8192, 10, 1.0, 0.01, True, 11, True), (3, 128, 1, 1, 10, 0.0, 0.1, False, 12, False),
]
