"""Case builders shared by the MMR tests (test_mmr_cpu.py, test_mmr_gpu.py, test_recommend_mmr_gpu.py): the literal per-round loop
that ``recommend.mmr_select`` is held against; exact cases -- one-hot or zero table rows, scores whose differences are powers of two,
lam a multiple of 1/4, so every cosine is 0 or 1, every v is exact in fp32 and in fp64 and ties are real --; clustered shortlists for
the rounding checks; and the two checks every device result is held to: greedy validity and exact equality on well-separated rows."""
import math

import numpy as np

EXACT_SCORES = np.array([-1.0, 0.0, 1.0, 1.0, 0.0, -np.inf, np.nan, np.inf], dtype=np.float32)    # finite spans: 1 or 2
EXACT_LAMS = (0.0, 0.25, 0.5, 0.75, 1.0)


def literal_mmr(s, ids, table, lam, k):
    """MMR as the words state it, one entry and one round at a time, in Python floats -> the ranks in the order taken."""
    n, M = len(table), len(s)
    live = [j for j in range(M) if 0 <= ids[j] < n and math.isfinite(s[j])]
    if not live:
        return []
    first, last = live[0], live[-1]
    span = float(s[first]) - float(s[last])

    def cos(j, i):
        a, b = [float(x) for x in table[ids[j]]], [float(x) for x in table[ids[i]]]
        na, nb = math.sqrt(sum(x * x for x in a)), math.sqrt(sum(x * x for x in b))
        return 0.0 if na == 0.0 or nb == 0.0 else sum(x * y for x, y in zip(a, b)) / (na * nb)
    taken = []
    while len(taken) < k:
        best, best_v = None, None
        for j in live:
            if j in taken:
                continue
            rel = 0.0 if span == 0.0 else (float(s[j]) - float(s[last])) / span
            pen = max([0.0] + [cos(j, i) for i in taken])
            v = lam * rel - (1.0 - lam) * pen
            if best is None or v > best_v:                                    # a later entry needs MORE: the lower rank wins ties
                best, best_v = j, v
        if best is None:
            break
        taken.append(best)
    return taken


def padded(taken, k):
    return np.array(list(taken) + [-1] * (k - len(taken)), dtype=np.int32)


def exact_groups(seed=0, groups=64, rows=16):
    """``groups`` x ``rows`` (about 1,000) small exact cases; a group shares M <= 12, k <= M, lam, and a table of n <= 6 one-hot or zero
    rows of E = 4 or 8 columns -- one launch on the device -> [(scores fp32 [rows, M], ids int32 [rows, M], table fp32 [n, E], lam, k)].
    Scores in any order, ids from -1 up to n + 1 (the last two out of range)."""
    rng = np.random.default_rng(seed)
    out = []
    for g in range(groups):
        M = int(rng.integers(1, 13))
        k = M if g % 8 == 0 else int(rng.integers(1, M + 1))
        n, E = int(rng.integers(1, 7)), int(rng.choice([4, 8]))
        table = np.zeros((n, E), dtype=np.float32)
        hot = rng.integers(-1, min(E, 3), size=n)                             # -1: a zero row; few distinct columns: many cosines of 1
        table[np.flatnonzero(hot >= 0), hot[hot >= 0]] = rng.choice([1.0, 2.0, 0.5], size=int((hot >= 0).sum()))
        scores = rng.choice(EXACT_SCORES, size=(rows, M)).astype(np.float32)
        ids = rng.integers(-1, n + 2, size=(rows, M)).astype(np.int32)
        out.append((scores, ids, table, EXACT_LAMS[g % len(EXACT_LAMS)], k))
    return out


def clustered(R, M, E, seed, n=None, dead=0.1):
    """R shortlists of M entries over a table of ``n`` (default 3 M + 5) rows that are 8 centres plus noise, so penalties matter:
    scores descending, distinct ids, and ``dead`` of the entries dead -- empty slots (-1 / -inf) at the tail, ids of n and beyond, a
    -inf or NaN score in the middle -> (scores fp32 [R, M], ids int32 [R, M], table fp32 [n, E])."""
    rng = np.random.default_rng(seed)
    n = 3 * M + 5 if n is None else n
    centres = rng.standard_normal((8, E))
    table = (centres[rng.integers(0, 8, size=n)] + 0.35 * rng.standard_normal((n, E))).astype(np.float32)
    scores = -np.sort(-rng.uniform(0.0, 4.0, size=(R, M)).astype(np.float32), axis=1)
    ids = np.stack([rng.permutation(n)[:M] for _ in range(R)]).astype(np.int32)
    for r in range(R):
        tail = int(rng.integers(0, max(1, int(2 * dead * M)) + 1)) if M > 2 else 0
        if tail:
            scores[r, M - tail:], ids[r, M - tail:] = -np.inf, -1
        for j in np.flatnonzero(rng.random(M) < dead / 2):
            kind = int(rng.integers(0, 3))
            if M > 2 and kind == 0:
                ids[r, j] = n + int(rng.integers(0, 3))
            elif M > 2 and kind == 1:
                scores[r, j] = np.nan if j % 2 else -np.inf
    if np.isfinite(scores[0, 0]) and ids[0, 0] >= 0:                          # the table's last row is read
        ids[0, ids[0] == n - 1] = ids[0, 0]
        ids[0, 0] = n - 1
    return scores, ids, table


def tolerance(E):
    """8 (E + 8) 2^-24: two cosines, each a dot product and two norms of E terms, under the worst-case fp32 summation bound."""
    return 8.0 * (E + 8) * 2.0 ** -24


def check_greedy(picks, scores, ids, table, lam, tol, what=''):
    """Greedy validity of the device's OWN picks, replayed through the fp64 statement: every pick is live and not repeated, its fp64 v
    is within ``tol`` of the best fp64 v among the live untaken entries of its round, and -1 stands only where none is left."""
    scores64, table64 = np.asarray(scores, dtype=np.float64), np.asarray(table, dtype=np.float64)
    n = table64.shape[0]
    for r in range(scores64.shape[0]):
        live = (ids[r] >= 0) & (ids[r] < n) & np.isfinite(scores64[r])
        at = np.flatnonzero(live)
        rel = np.zeros(len(live))
        if at.size and scores64[r, at[0]] != scores64[r, at[-1]]:
            rel[at] = (scores64[r, at] - scores64[r, at[-1]]) / (scores64[r, at[0]] - scores64[r, at[-1]])
        unit = np.zeros((len(live), table64.shape[1]))
        x = table64[ids[r, at]]
        norm = np.sqrt((x * x).sum(axis=1, keepdims=True))
        unit[at] = np.divide(x, norm, out=np.zeros_like(x), where=norm > 0)
        pen, open_ = np.zeros(len(live)), live.copy()
        for t, p in enumerate(picks[r]):
            if p < 0:
                assert not open_.any() and (picks[r, t:] == -1).all(), '%s row %d round %d: -1 with live entries left' % (what, r, t)
                break
            assert 0 <= p < len(live) and open_[p], '%s row %d round %d: pick %d is dead or repeated' % (what, r, t, p)
            v = lam * rel - (1.0 - lam) * pen
            assert v[p] >= v[open_].max() - tol, '%s row %d round %d: v[%d] = %.9g, best %.9g, tol %.3g' % (what, r, t, p, v[p],
                                                                                                           v[open_].max(), tol)
            open_[p] = False
            pen = np.maximum(pen, unit @ unit[p])


def check_exact(picks, want, gap, tol, what=''):
    """Exact equality with ``mmr_select``'s picks on the rows whose fp64 minimum gap exceeds 2 tol; at least half of the rows must be
    such rows (a condition on the inputs) -> the number of rows compared."""
    sure = gap > 2.0 * tol
    assert 2 * int(sure.sum()) >= len(gap), '%s: only %d of %d rows have a minimum gap above 2 tol = %.3g' % (what, sure.sum(), len(gap), 2 * tol)
    assert np.array_equal(picks[sure], want[sure]), '%s: rows %s differ' % (what, np.flatnonzero(sure & (picks != want).any(axis=1))[:8])
    return int(sure.sum())
