"""Case builders shared by the topic-quota tests (test_topk_quota_cpu.py, test_topk_quota_gpu.py): score rows built to hit the edges of
the order -- many ties, +-0.0, NaN, -inf --, group keys, drop masks, and the literal sequential walk that ``recommend.quota_topk`` is
held against."""
import numpy as np

CHUNK, TOPK_MAX = 4096, 128


def edge_rows(U, C, seed):
    """U rows of C scores, cycling through: few distinct small integers (many ties); +-0.0 mixed with a few values; random with
    blocks of -inf and a NaN; NaN / -inf / inf / zeros / a number; plain random."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((U, C), dtype=np.float32)
    for u in range(U):
        kind = u % 5
        if kind == 0:
            rows[u] = rng.integers(-2, 3, size=C).astype(np.float32)
        elif kind == 1:
            rows[u] = rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], dtype=np.float32), size=C)
        elif kind == 2:
            rows[u] = rng.standard_normal(C).astype(np.float32)
            rows[u, : C // 3] = -np.inf
            rows[u, C // 2] = np.nan
        elif kind == 3:
            rows[u] = rng.choice(np.array([np.nan, -np.inf, np.inf, 0.0, -0.0, 2.0], dtype=np.float32), size=C)
        else:
            rows[u] = rng.standard_normal(C).astype(np.float32)
    return rows


def group_keys(C, n_groups, seed):
    """int32 [C]: skewed over n_groups groups (group 0 holds about half), so a small quota binds."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, n_groups, size=C)
    keys[rng.random(C) < 0.5] = 0
    return keys.astype(np.int32)


def drop_mask(R, C, seed, p=0.3):
    return np.random.default_rng(seed).random((R, C)) < p


def crowded(C=2 * CHUNK, crowd=300, seed=5):
    """One row of C scores in which group 0 owns the `crowd` best scores of EVERY chunk of 4096 (the rest spread over groups 1 .. 6,
    all below): a kernel that cuts a chunk to its plain best 128 before it filters has nothing but group 0 left."""
    rng = np.random.default_rng(seed)
    scores = rng.uniform(0.0, 1.0, size=(1, C)).astype(np.float32)
    keys = rng.integers(1, 7, size=C).astype(np.int32)
    for c0 in range(0, C, CHUNK):
        at = c0 + rng.permutation(min(CHUNK, C - c0))[:crowd]
        scores[0, at] = rng.uniform(2.0, 3.0, size=at.size).astype(np.float32)
        keys[at] = 0
    return scores, keys


def sequential_walk(row, keys, k, quota, drop=None):
    """The walk as the words state it, one entry at a time -> the taken positions.  Order: descending score, +0.0 == -0.0, equal
    scores lower position first, a NaN behind every number, NaNs in position order (a plain comparison sort on that key)."""
    def rank(j):
        v = row[j]
        return (1, 0.0, j) if np.isnan(v) else (0, -(float(v) + 0.0), j)
    taken, count = [], {}
    for j in sorted(range(len(row)), key=rank):
        if keys[j] < 0 or (drop is not None and drop[j]):
            continue
        if count.get(int(keys[j]), 0) >= quota:
            continue
        count[int(keys[j])] = count.get(int(keys[j]), 0) + 1
        taken.append(j)
        if len(taken) == k:
            break
    return taken


def same(got, want, what=''):
    """(positions, scores) equal, the scores bit for bit (the sign of a zero, a NaN's payload)."""
    pos, top = (np.asarray(x.cpu().numpy() if hasattr(x, 'cpu') else x) for x in got)
    assert pos.dtype == np.int32 and top.dtype == np.float32 and pos.shape == top.shape == want[0].shape, what
    assert np.array_equal(pos, want[0]), what
    assert np.array_equal(top.view(np.int32), want[1].view(np.int32)), what
