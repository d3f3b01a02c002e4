"""The host side of pool recommendation (Model.score_pool / Model.recommend): the grouping plan.  Pure numpy, no GPU.

Under the eval shape the candidate enters the user side only through its topic (layers.py:66-81 reads the candidate's topic row and
nothing else of it), so everything up to the operands of the match is computed once per (user, candidate topic) GROUP and the pool is
walked in topic order: ``pool_plan`` sorts the pool by topic key and gives the CSR of the topics' segments, ``group_offsets`` lays the
segments out user-major for the users of one pass."""
import collections

import numpy as np

PoolPlan = collections.namedtuple('PoolPlan', 'order segments category subCategory')
PoolPlan.__doc__ = """order int64 [C]: pool positions in group order (stable: position order inside a group); segments int64 [T + 1]:
group t owns order[segments[t]:segments[t + 1]]; category / subCategory int64 [T]: the topic of group t (what the user side reads)."""


def _topics(who, category, subCategory, by):
    """The topic arguments of ``who`` (pool_plan / topic_table) as int64 [n], n >= 1, refused as both refuse them."""
    cat, sub = (np.asarray(a).reshape(-1).astype(np.int64) for a in (category, subCategory))
    if cat.shape[0] < 1 or sub.shape[0] != cat.shape[0]:
        raise ValueError('%s needs category and subCategory of one length >= 1, got %d and %d' % (who, cat.shape[0], sub.shape[0]))
    if by not in ('topic', 'category', None):
        raise ValueError("by must be 'topic', 'category' or None, got %r" % (by,))
    if by is not None and (cat.min() < 0 or sub.min() < 0):
        raise ValueError('negative topic ids')
    return cat, sub


def _topic_key(cat, sub, by, width):
    """One integer per news that two news share exactly when they fall into one group; ``width``: above every subCategory."""
    return cat * width + sub if by == 'topic' else cat


def pool_plan(category, subCategory, by='topic', topics=None):
    """Group a pool of C news by what the user side reads of a candidate.

    ``by``: 'topic' -- (category, subCategory), the CROWN user encoder; 'category' -- the category alone (ATT / MHSA: no subcategory
    enters their candidate-aware attention; a group's ``subCategory`` is its first member's and is not read); None -- the
    candidate-aware attention is off, the user side does not read the candidate at all: ONE group.
    ``topics``: optional list of (category, subCategory) keys (of categories for 'category') that fixes the groups and their order,
    e.g. every topic of the corpus, so that plans of different pools line up; a topic without a candidate stays as an EMPTY group, a
    candidate whose topic is not listed is a ValueError.  Default: the pool's own topics, ascending."""
    cat, sub = _topics('pool_plan', category, subCategory, by)
    C = cat.shape[0]
    if by is None:
        if topics is not None:
            raise ValueError('by=None makes one group: topics cannot be given')
        return PoolPlan(np.arange(C, dtype=np.int64), np.array([0, C], dtype=np.int64), cat[:1].copy(), sub[:1].copy())
    width = int(sub.max()) + 1
    if topics is not None:
        tk = np.asarray(topics, dtype=np.int64).reshape(len(topics), -1)
        if tk.shape[1] != (2 if by == 'topic' else 1) or (tk < 0).any():
            raise ValueError('topics must be non-negative (category, subCategory) pairs for by=\'topic\', categories for by=\'category\'')
        width = max(width, int(tk[:, -1].max()) + 1) if by == 'topic' else width
    key = _topic_key(cat, sub, by, width)
    if topics is None:
        order = np.argsort(key, kind='stable')
        skey = key[order]
        first = np.flatnonzero(np.concatenate([[True], skey[1:] != skey[:-1]]))
        segments = np.concatenate([first, [C]]).astype(np.int64)
        return PoolPlan(order.astype(np.int64), segments, cat[order[first]], sub[order[first]])
    gkey = _topic_key(tk[:, 0], tk[:, -1], by, width)
    if len(set(gkey.tolist())) != len(gkey):
        raise ValueError('topics holds a key twice')
    slot = {int(k): t for t, k in enumerate(gkey)}
    try:
        group = np.array([slot[int(k)] for k in key], dtype=np.int64)
    except KeyError as e:
        raise ValueError('a candidate\'s topic (key %s) is not in topics' % e) from None
    order = np.argsort(group, kind='stable')
    segments = np.concatenate([[0], np.cumsum(np.bincount(group, minlength=len(gkey)))]).astype(np.int64)
    g_sub = tk[:, 1] if by == 'topic' else np.zeros(len(gkey), dtype=np.int64)
    return PoolPlan(order.astype(np.int64), segments, tk[:, 0].copy(), g_sub)


def group_offsets(segments, n_users):
    """The CSR of one pass's groups over its pairs, user-major: the pairs of a pass are [n_users, C] in plan order (pair u C + j is user
    u with pool position order[j]), group u T + t owns pairs u C + segments[t] .. u C + segments[t + 1] - 1 -> int64 [n_users T + 1]."""
    seg = np.asarray(segments, dtype=np.int64).reshape(-1)
    if seg.shape[0] < 2 or seg[0] != 0 or (np.diff(seg) < 0).any():
        raise ValueError('segments must start at 0 and not decrease')
    if n_users < 0:
        raise ValueError('n_users must not be negative')
    C = int(seg[-1])
    starts = (np.arange(n_users, dtype=np.int64)[:, None] * C + seg[None, :-1]).reshape(-1)
    return np.concatenate([starts, [n_users * C]]).astype(np.int64)


def users_per_pass(n_users, C, n_groups, H, pairs_per_pass):
    """Users of one pass: as many as keep both the candidate rows (users x C) and the refined history rows (users x groups x H) within
    ``pairs_per_pass`` rows -- one user at the least, then evened out over the passes."""
    if pairs_per_pass < 1:
        raise ValueError('pairs_per_pass must be positive')
    per = max(1, min(n_users, pairs_per_pass // max(C, 1), pairs_per_pass // max(n_groups * H, 1)))
    n_pass = (n_users + per - 1) // per if n_users else 1
    return max(1, (n_users + n_pass - 1) // n_pass)


# ---- candidate lists (Model.score_lists / Model.recommend_lists): every user has a list of its own -------------------------------------
MAX_TOPICS = 8192                     # lime_list_plan's table of bins

ListPlan = collections.namedtuple('ListPlan', 'order group_offsets slot_key n_distinct')
ListPlan.__doc__ = """order int64 [P]: the pairs in group order -- user u's stay in rows offsets[u] .. offsets[u + 1] - 1, sorted by slot,
stable in list order; group_offsets int64 [U S + 1]: group u S + s (user u, its s-th key ascending) owns order[group_offsets[u S + s]:
group_offsets[u S + s + 1]]; slot_key int32 [U S]: the key of each slot (an unused slot: the key of the user's slot 0; an empty list:
key 0); n_distinct int32 [U]: the distinct keys of each list."""


def topic_table(category, subCategory, by):
    """Dense topic ids for a corpus of n_news news -> (topic_of_news int32 [n_news], category int64 [T_all], subCategory int64 [T_all]).
    ``by`` as in ``pool_plan``: 'topic' -- the (category, subCategory) pair; 'category' -- the category alone (a topic's subCategory is
    its first news' and is not read); None -- one id, 0, for every news.  The ids ascend in ``pool_plan``'s key order, so two news
    share an id exactly when ``pool_plan`` puts them into one group."""
    cat, sub = _topics('topic_table', category, subCategory, by)
    if by is None:
        return np.zeros(cat.shape[0], dtype=np.int32), cat[:1].copy(), sub[:1].copy()
    key = _topic_key(cat, sub, by, int(sub.max()) + 1)
    _, first, topic = np.unique(key, return_index=True, return_inverse=True)
    return topic.reshape(-1).astype(np.int32), cat[first], sub[first]


def list_plan(keys, offsets, slots=None):
    """Group the pairs of U candidate lists by (user, key): the host statement of ``ops.list_plan`` (lime_list_plan).

    ``keys`` int [P]: the topic id of every pair (>= 0); ``offsets`` int64 [U + 1]: the CSR of the lists.  A user's distinct keys take
    slots 0 .. n_distinct[u] - 1 in ascending key order; ``slots`` = S slots per user (default max(1, n_distinct.max()); fewer than
    n_distinct.max() is a ValueError); groups are user-major, the slots behind a user's last key are empty groups -> ListPlan."""
    keys = np.asarray(keys).reshape(-1).astype(np.int64)
    off = np.asarray(offsets).reshape(-1).astype(np.int64)
    P = keys.shape[0]
    if off.shape[0] < 1 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != P:
        raise ValueError('offsets must start at 0, not decrease and end at P = %d' % P)
    if P and keys.min() < 0:
        raise ValueError('negative keys')
    U = off.shape[0] - 1
    lens = np.diff(off)
    user = np.repeat(np.arange(U, dtype=np.int64), lens)
    order = np.lexsort((np.arange(P), keys, user)).astype(np.int64)           # by user, then key, then list order
    su, sk = user[order], keys[order]
    new = np.ones(P, dtype=bool)
    new[1:] = (su[1:] != su[:-1]) | (sk[1:] != sk[:-1])                       # the first row of every (user, key) group
    n_distinct = np.bincount(su[new], minlength=U).astype(np.int32)
    need = max(1, int(n_distinct.max())) if U else 1
    S = need if slots is None else int(slots)
    if S < need:
        raise ValueError('slots = %d, but a list holds %d distinct keys' % (S, need))
    rows = np.flatnonzero(new)
    slot = np.arange(rows.shape[0]) - np.repeat(np.cumsum(n_distinct) - n_distinct, n_distinct)
    group_offsets = np.empty(U * S + 1, dtype=np.int64)
    group_offsets[:-1] = np.repeat(off[1:], S)                                # an unused slot: empty, at the end of the user's rows
    group_offsets[-1] = P
    group_offsets[su[rows] * S + slot] = rows
    slot_key = np.zeros((U, S), dtype=np.int32)
    has = n_distinct > 0
    slot_key[has] = sk[off[:-1][has]][:, None]                                # the user's first (smallest) key
    slot_key.reshape(-1)[su[rows] * S + slot] = sk[rows]
    return ListPlan(order, group_offsets, slot_key.reshape(-1), n_distinct)


def list_passes(offsets, n_distinct, H, pairs_per_pass):
    """Consecutive users per pass of Model.score_lists -> list of (u0, u1, S_pass): a pass keeps its pairs and its users x S_pass x H
    refined rows within ``pairs_per_pass`` each, S_pass = max(1, the largest n_distinct of its users); one user a pass at the least."""
    if pairs_per_pass < 1:
        raise ValueError('pairs_per_pass must be positive')
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    nd = np.asarray(n_distinct, dtype=np.int64).reshape(-1)
    U, passes, u0 = off.shape[0] - 1, [], 0
    while u0 < U:
        u1, S = u0 + 1, max(1, int(nd[u0]))
        while u1 < U:
            S1 = max(S, int(nd[u1]))
            if off[u1 + 1] - off[u0] > pairs_per_pass or (u1 + 1 - u0) * S1 * H > pairs_per_pass:
                break
            u1, S = u1 + 1, S1
        passes.append((u0, u1, S))
        u0 = u1
    return passes


# ---- topic quotas (Model.recommend* with max_per_topic): at most `quota` entries of one group among the k --------------------------------
def walk_order(scores):
    """The positions of a row of scores in ``recommend``'s order: descending score; +0.0 == -0.0; equal scores lower position first;
    a NaN behind every number, NaNs in position order."""
    row = np.asarray(scores, dtype=np.float32).reshape(-1)
    nan = np.isnan(row)
    value = np.where(nan, 0.0, row).astype(np.float64) + 0.0                 # -0.0 + 0.0 = +0.0: the zeros tie
    order = np.argsort(-value, kind='stable')
    return order[np.argsort(nan[order], kind='stable')]


def quota_topk(scores, keys, k, quota, drop=None):
    """The host statement of ``ops.topk_rows_quota`` (lime_topk_rows_quota_f32) -> (positions int32 [U, k], scores fp32 [U, k]).

    ``scores`` [U, C]; ``keys`` int [C]: column j belongs to group keys[j]; ``drop``: None or bool / uint8 [R, C], row u masked by
    drop[u % R].  Per row: walk the columns in ``walk_order``; take a column unless ``quota`` columns of its group were taken before
    it; stop at k.  A dropped column -- its drop entry set, or its key negative -- takes no part.  The outputs hold the taken
    columns in that order and their scores (the input's bits); the slots behind the last one hold -1 / -inf.
    Stated through the first of the two facts that the kernel rests on -- the result is the k best of the union, over the groups, of
    each group's ``quota`` best --: rank every column within its group, keep the ranks below ``quota``, cut at k."""
    scores = np.asarray(scores, dtype=np.float32)
    if scores.ndim != 2:
        raise ValueError('scores must be [U, C], got %s' % (scores.shape,))
    U, C = scores.shape
    keys = np.asarray(keys).reshape(-1).astype(np.int64)
    k, quota = int(k), int(quota)
    if keys.shape[0] != C or k < 1 or quota < 1:
        raise ValueError('quota_topk needs C = %d keys, k >= 1 and quota >= 1, got %d keys, k = %d, quota = %d' % (C, keys.shape[0], k, quota))
    if drop is not None:
        drop = np.asarray(drop).astype(bool).reshape(-1, C)
    pos = np.full((U, k), -1, dtype=np.int32)
    top = np.full((U, k), -np.inf, dtype=np.float32)
    for u in range(U):
        order = walk_order(scores[u])
        live = keys[order] >= 0
        if drop is not None:
            live &= ~drop[u % drop.shape[0]][order]
        order = order[live]
        g = keys[order]
        by_group = np.argsort(g, kind='stable')                               # groups together, each in walk order
        gs = g[by_group]
        head = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1]]) if gs.size else np.zeros(0, dtype=np.int64)
        rank = np.empty(gs.size, dtype=np.int64)
        rank[by_group] = np.arange(gs.size) - np.repeat(head, np.diff(np.r_[head, gs.size]))
        taken = order[rank < quota][:k]
        pos[u, :taken.size] = taken
        top[u, :taken.size] = scores[u, taken]
    return pos, top


def quota_topk_segments(scores, offsets, keys, k, quota, drop=None):
    """``quota_topk`` over the segments of a CSR: the host statement of ``ops.topk_segments_quota`` (lime_topk_segments_quota_f32).
    ``scores`` [P], ``offsets`` int64 [U + 1], ``keys`` int [P], ``drop`` None or [P]; positions count WITHIN the segment."""
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    off = np.asarray(offsets).reshape(-1).astype(np.int64)
    keys = np.asarray(keys).reshape(-1)
    U, k = off.shape[0] - 1, int(k)
    pos = np.full((U, k), -1, dtype=np.int32)
    top = np.full((U, k), -np.inf, dtype=np.float32)
    drop = None if drop is None else np.asarray(drop).reshape(-1)
    for u in range(U):
        a, b = off[u], off[u + 1]
        if b > a:
            pos[u], top[u] = (r[0] for r in quota_topk(scores[None, a:b], keys[a:b], k, quota, None if drop is None else drop[None, a:b]))
    return pos, top


# ---- diverse slates (Model.recommend* with mmr_lambda): maximal marginal relevance over a shortlist -------------------------------------
def mmr_select(scores, ids, table, lam, k, return_gap=False):
    """The host statement of ``ops.mmr_rows`` (lime_mmr_rows_f32), in fp64 -> picks int32 [R, k]: the shortlist ranks in the order
    taken, -1 behind the last one.

    ``scores`` [R, M]: a row's shortlist, best first, as the top-k kernels return it; ``ids`` int [R, M]: the row of ``table``
    [n, E] behind each entry, -1 for an empty slot.  An entry is DEAD if its id is < 0 or >= n, or its score is not finite (an
    excluded candidate carries -inf): it is never taken and never read from ``table``.  With ``first`` / ``last`` the first and last
    live entries of the row: rel[j] = (s[j] - s[last]) / (s[first] - s[last]), 0 for every j when the two scores are equal;
    cos(j, i): the cosine of rows ids[j] and ids[i], 0 when either norm is 0.  Each round takes the live, untaken j that maximises
    v[j] = lam rel[j] - (1 - lam) pen[j], pen[j] = max(0, max over the taken i of cos(j, i)) -- 0 while nothing is taken, and a
    negative cosine earns nothing --, the lower rank on equal v; until k are taken or no live entry is left.

    Hence: lam = 1 takes the live entries in rank order (of a sorted shortlist: the plain top-k); lam = 0 takes ``first`` first
    (every v is 0, the lowest rank wins); k >= the number of live entries returns all of them.
    ``return_gap``: -> (picks, gap fp64 [R]): per row the smallest difference between a round's best and second-best v (inf where no
    round had two candidates) -- a row whose gap is well above the rounding of another arithmetic has ONE right answer in it."""
    scores = np.asarray(scores, dtype=np.float64)
    ids = np.asarray(ids).astype(np.int64)
    table = np.asarray(table, dtype=np.float64)
    lam, k = float(lam), int(k)
    if scores.ndim != 2 or ids.shape != scores.shape or table.ndim != 2:
        raise ValueError('mmr_select needs scores and ids [R, M] and table [n, E], got %s, %s and %s' % (scores.shape, ids.shape, table.shape))
    if k < 1 or not 0.0 <= lam <= 1.0:
        raise ValueError('mmr_select needs k >= 1 and 0 <= lam <= 1, got k = %d, lam = %r' % (k, lam))
    R, M = scores.shape
    picks = np.full((R, k), -1, dtype=np.int32)
    gaps = np.full(R, np.inf)
    for r in range(R):
        live = np.flatnonzero((ids[r] >= 0) & (ids[r] < table.shape[0]) & np.isfinite(scores[r]))
        if live.size == 0:
            continue
        s = scores[r, live]
        span = s[0] - s[-1]
        rel = (s - s[-1]) / span if span != 0 else np.zeros(live.size)
        x = table[ids[r, live]]
        norm = np.sqrt((x * x).sum(axis=1))
        unit = np.divide(x, norm[:, None], out=np.zeros_like(x), where=norm[:, None] > 0)
        pen = np.zeros(live.size)
        open_ = np.ones(live.size, dtype=bool)
        for t in range(min(k, live.size)):
            v = np.where(open_, lam * rel - (1.0 - lam) * pen, -np.inf)
            best = int(np.argmax(v))                                          # the first of equal maxima: the lower rank
            if open_.sum() > 1:
                gaps[r] = min(gaps[r], v[best] - np.delete(v, best).max())
            picks[r, t] = live[best]
            open_[best] = False
            pen = np.maximum(pen, unit @ unit[best])
    return (picks, gaps) if return_gap else picks


# ---- calibrated slates (Model.recommend* with calibrate_lambda): the slate's topic mix follows the reader's own -------------------------
CALIBRATE_ALPHA = 0.01                # the share of the target mixed into the slate's distribution (Steck's smoothing)


def calibration_target(hist_keys, n_keys, weights=None):
    """The target of one history row -> (groups int64 [S] ascending, p fp64 [S]); S = 0: no target.  ``hist_keys`` [H]: the group of
    every history slot, an entry outside [0, n_keys) is no click; ``weights`` [H] or None (1 each): a weight that is not finite or
    not > 0 removes the slot.  W is the weight sum over the live slots (not finite, or 0: no target) and p[g] the weight sum of the
    live slots of group g, taken in slot order, divided by W."""
    hk = np.asarray(hist_keys).reshape(-1).astype(np.int64)
    w = np.ones(hk.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.shape[0] != hk.shape[0]:
        raise ValueError('a weight per history slot: %d weights, %d slots' % (w.shape[0], hk.shape[0]))
    live = (hk >= 0) & (hk < int(n_keys)) & np.isfinite(w) & (w > 0)
    none = (np.zeros(0, dtype=np.int64), np.zeros(0))
    if not live.any():
        return none
    wl = w[live]
    W = float(np.cumsum(wl)[-1])                                              # slot order, one addition after the other
    if not (np.isfinite(W) and W > 0):
        return none
    groups, inverse = np.unique(hk[live], return_inverse=True)
    return groups, np.bincount(inverse.reshape(-1), weights=wl) / W           # (bincount adds in slot order)


def _history_rows(who, hist_keys, weights):
    hk = np.asarray(hist_keys).astype(np.int64)
    if hk.ndim != 2:
        raise ValueError('%s needs hist_keys [hist_rows, H], got %s' % (who, hk.shape))
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    if w is not None and w.shape != hk.shape:
        raise ValueError('%s needs weights shaped like hist_keys %s, got %s' % (who, hk.shape, w.shape))
    if hk.shape[1] > 0 and hk.shape[0] < 1:
        raise ValueError('%s needs at least one history row' % who)
    return hk, w


def calibrated_select(scores, ids, keys, n_keys, hist_keys, weights=None, lam=0.5, alpha=CALIBRATE_ALPHA, k=10, return_gap=False):
    """The host statement of ``ops.calibrate_rows`` (lime_calibrate_rows_f32), in fp64 -> picks int32 [R, k]: the shortlist ranks in
    the order taken, -1 behind the last one.  Calibrated re-ranking (Steck, RecSys 2018) by the greedy rule.

    ``scores`` [R, M] and ``ids`` int [R, M]: a row's shortlist, best first, and the news id of each entry; ``keys`` int [n]: the
    group of every news (a key outside [0, n_keys) is no group); ``hist_keys`` int [hist_rows, H] and ``weights`` [hist_rows, H] or
    None: row r's TARGET p is ``calibration_target`` of history row r % hist_rows.  An entry is DEAD exactly as in ``mmr_select``:
    its id is < 0 or >= n, or its score is not finite; rel[j] is ``mmr_select``'s too: (s[j] - s[last]) / (s[first] - s[last]) over
    the live entries, 0 everywhere when the span is 0.  Round t has t entries taken, c[g] of them in group g.  With T = t + 1 and
    q(c) = (1 - alpha) c / T + alpha p[g], entry j of group g has
        gain[j] = p[g] (ln q(c[g] + 1) - ln q(c[g])) / ln(1 / alpha)        if p[g] > 0, else 0
    (0 too when the row has no target or j has no group), and the round takes the live, untaken j of the largest
    v[j] = lam rel[j] + (1 - lam) gain[j], the lower rank on equal v; until k are taken or none is left.

    Adding j changes only its own group's term of KL(p || q~), q~[g] = (1 - alpha) c[g] / T + alpha p[g] the slate of size T with j
    in it, so the largest gain is the smallest KL: Steck's greedy in O(M) a round.  ln(1 / alpha) is the largest value the bracket
    times p can take (p = 1, T = 1, c = 0), so gain lies in [0, 1] like rel and lam means what it means for MMR.
    Hence: lam = 1 takes the live entries in rank order (of a sorted shortlist); a row without a target does the same; k >= the
    number of live entries returns all of them; a round does not read k, so a PREFIX of the picks at k is the picks at a smaller k;
    and two entries of one group with equal scores have the same v by construction, so they come out in rank order.
    ``return_gap``: -> (picks, gap fp64 [R]): per row the smallest difference, over the rounds, between the best v and the best v
    among the open entries whose (group, score) differ from the winner's (a group outside the target's support counts as no group:
    its gain is 0 by construction too); inf where no round had such an entry."""
    scores = np.asarray(scores, dtype=np.float64)
    ids = np.asarray(ids).astype(np.int64)
    keys = np.asarray(keys).reshape(-1).astype(np.int64)
    lam, alpha, k, n_keys = float(lam), float(alpha), int(k), int(n_keys)
    if scores.ndim != 2 or ids.shape != scores.shape or keys.shape[0] < 1 or n_keys < 1:
        raise ValueError('calibrated_select needs scores and ids [R, M], keys [n] with n >= 1 and n_keys >= 1, got %s, %s, %s and %d'
                         % (scores.shape, ids.shape, keys.shape, n_keys))
    if k < 1 or not 0.0 <= lam <= 1.0 or not 0.0 < alpha < 1.0:
        raise ValueError('calibrated_select needs k >= 1, 0 <= lam <= 1 and 0 < alpha < 1, got k = %d, lam = %r, alpha = %r' % (k, lam, alpha))
    hk, w = _history_rows('calibrated_select', hist_keys, weights)
    R, M = scores.shape
    picks = np.full((R, k), -1, dtype=np.int32)
    gaps = np.full(R, np.inf)
    scale = np.log(1.0 / alpha)
    targets = {}
    for r in range(R):
        live = np.flatnonzero((ids[r] >= 0) & (ids[r] < keys.shape[0]) & np.isfinite(scores[r]))
        if live.size == 0:
            continue
        s = scores[r, live]
        span = s[0] - s[-1]
        rel = (s - s[-1]) / span if span != 0 else np.zeros(live.size)
        hr = r % hk.shape[0] if hk.shape[1] else -1
        if hr not in targets:
            targets[hr] = calibration_target(hk[hr], n_keys, None if w is None else w[hr]) if hr >= 0 else calibration_target([], n_keys)
        groups, p = targets[hr]
        key = keys[ids[r, live]]
        at, pe = np.full(live.size, -1, dtype=np.int64), np.zeros(live.size)  # the entry's support group (-1: none) and its p
        if groups.size:
            at = np.minimum(np.searchsorted(groups, key), groups.size - 1)
            at = np.where(groups[at] == key, at, -1)
            pe = np.where(at >= 0, p[np.maximum(at, 0)], 0.0)
        counts = np.zeros(max(groups.size, 1))
        open_ = np.ones(live.size, dtype=bool)
        for t in range(min(k, live.size)):
            T = t + 1.0
            ce = np.where(at >= 0, counts[np.maximum(at, 0)], 0.0)
            has = pe > 0
            q1 = np.where(has, (1.0 - alpha) * (ce + 1.0) / T + alpha * pe, 1.0)
            q0 = np.where(has, (1.0 - alpha) * ce / T + alpha * pe, 1.0)
            gain = pe * (np.log(q1) - np.log(q0)) / scale
            v = np.where(open_, lam * rel + (1.0 - lam) * gain, -np.inf)
            best = int(np.argmax(v))                                          # the first of equal maxima: the lower rank
            other = open_ & ~((at == at[best]) & (s == s[best]))
            if other.any():
                gaps[r] = min(gaps[r], v[best] - v[other].max())
            picks[r, t] = live[best]
            open_[best] = False
            if at[best] >= 0:
                counts[at[best]] += 1.0
    return (picks, gaps) if return_gap else picks


def slate_miscalibration(positions, k, offsets, news, keys, n_keys, hist_keys, weights=None, alpha=CALIBRATE_ALPHA):
    """The host statement of ``ops.slate_miscalibration`` (lime_slate_miscalibration), in fp64 -> (value fp64 [R], status int32 [R]):
    how far the topic mix of a finished slate is from its reader's, KL(p || q~).

    ``positions`` / ``k`` / ``offsets`` / ``news`` as in ``slate_metrics``, and "filled" is its rule: the position lies inside the
    list (the pool) and the news id behind it inside [0, n), n = len(keys).  ``keys`` int [n], ``hist_keys`` / ``weights``: as in
    ``calibrated_select`` -- slate r reads history row r % hist_rows.  With c[g] the FILLED slots of group g and F their number,
        value = sum over the target's support of p[g] ln(p[g] / ((1 - alpha) c[g] / F + alpha p[g]))
    status: 1 no target; else 2 no filled slot; else 0.  The value is 0 where the status is not 0."""
    pos = np.asarray(positions).astype(np.int64)
    k, n_keys, alpha = int(k), int(n_keys), float(alpha)
    if pos.ndim != 2 or not 1 <= k <= pos.shape[1]:
        raise ValueError('slate_miscalibration needs positions [R, ldp] and 1 <= k <= ldp, got %s and k = %d' % (pos.shape, k))
    if not 0.0 < alpha < 1.0 or n_keys < 1:
        raise ValueError('slate_miscalibration needs 0 < alpha < 1 and n_keys >= 1, got alpha = %r, n_keys = %d' % (alpha, n_keys))
    R = pos.shape[0]
    pos = pos[:, :k]
    news = np.asarray(news).reshape(-1).astype(np.int64)
    keys = np.asarray(keys).reshape(-1).astype(np.int64)
    P, n = news.shape[0], keys.shape[0]
    hk, w = _history_rows('slate_miscalibration', hist_keys, weights)
    if offsets is None:
        beg, length = np.zeros(R, dtype=np.int64), np.full(R, P, dtype=np.int64)
    else:
        off = np.clip(np.asarray(offsets).reshape(-1).astype(np.int64), 0, P)
        if off.shape[0] != R + 1:
            raise ValueError('offsets must have R + 1 = %d entries, got %d' % (R + 1, off.shape[0]))
        beg = off[:-1]
        length = np.maximum(off[1:], beg) - beg
    inside = (pos >= 0) & (pos < length[:, None])
    nid = news[np.where(inside, beg[:, None] + pos, 0)] if P else np.zeros_like(pos)
    filled = inside & (nid >= 0) & (nid < n)
    key = np.where(filled, keys[np.where(filled, nid, 0)], -1) if n else np.full(pos.shape, -1)
    value, status = np.zeros(R), np.zeros(R, dtype=np.int32)
    for r in range(R):
        groups, p = calibration_target(hk[r % hk.shape[0]], n_keys, None if w is None else w[r % hk.shape[0]]) if hk.shape[1] else ((), ())
        F = int(filled[r].sum())
        if len(groups) == 0:
            status[r] = 1
        elif F == 0:
            status[r] = 2
        else:
            c = (key[r][None, :] == groups[:, None]).sum(axis=1)
            on = p > 0
            value[r] = float((p[on] * np.log(p[on] / ((1.0 - alpha) * c[on] / F + alpha * p[on]))).sum())
    return value, status


# ---- what a slate is worth (util.evaluate_slates_on_device): accuracy against the labels, diversity of the slots ------------------------
SLATE_COLUMNS = ('ndcg', 'rr', 'hit', 'recall', 'ild', 'topics', 'filled', 'value')


def slate_metrics(positions, k, offsets, news, labels=None, skip=None, value=None, table=None, keys=None, n=None, n_keys=None):
    """The host statement of ``ops.slate_metrics`` (lime_slate_metrics_f32), in fp64 -> (per_slate fp64 [R, 8], status int32 [R],
    sums fp64 [8], counts int64 [3]).

    ``positions`` int [R, >= k]: slot j < k of slate r.  With ``offsets`` [R + 1] a position counts inside the slate's own list, rows
    offsets[r] .. offsets[r + 1] - 1 of the [P] arrays ``news`` / ``labels`` / ``value`` (the impression's rows); with ``offsets``
    None inside one pool of P rows that all slates share.  ``news`` [P]: the news id of a row -- the row of ``table`` [n, E] and of
    ``keys`` [n] (a key outside [0, n_keys) is no key).  A slot is FILLED when its position lies inside the list (the pool) and the
    news id behind it inside [0, n); every other slot (-1) is empty: it earns nothing and still occupies its slot.

    status: 1 skipped (``skip`` [R]), no ``labels`` or no rows; else 3 a label outside {0, 1} among the impression's rows; else 2 one
    class only among them; else 0.  With Ppos the positives among the impression's rows and disc[p] = 1 / log2(p + 2), the columns:
    0 nDCG@k = (sum over the filled slots j with label 1 of disc[j]) / (sum_{p < min(k, Ppos)} disc[p]); 1 RR@k = 1 / (1 + the first
    slot that holds a positive) or 0; 2 hit@k; 3 recall@k = hits / Ppos -- zeros unless status is 0; 4 ILD = 1 - the mean over the
    pairs a < b of filled slots of cos(table[news_a], table[news_b]), cos 0 when either norm is 0, defined with >= 2 filled slots;
    5 the distinct keys among the filled slots; 6 the filled slots; 7 the mean of ``value`` over them.  A column whose input is None
    or that is not defined for the slate is 0.  Sums in slot order, one addition after the other (the kernel's order for columns
    0-3 and 7).  counts: the slates with status 0 (they feed the sums of columns 0-3), the slates not skipped with >= 2 filled slots
    (column 4), with >= 1 (columns 5-7)."""
    pos = np.asarray(positions).astype(np.int64)
    k = int(k)
    if pos.ndim != 2 or not 1 <= k <= pos.shape[1]:
        raise ValueError('slate_metrics needs positions [R, ldp] and 1 <= k <= ldp, got %s and k = %d' % (pos.shape, k))
    if labels is not None and offsets is None:
        raise ValueError('labels need offsets: a pool has no impression to count the positives of')
    R = pos.shape[0]
    pos = pos[:, :k]
    news = np.asarray(news).reshape(-1).astype(np.int64)
    P = news.shape[0]
    table = None if table is None else np.asarray(table, dtype=np.float64)
    keys = None if keys is None else np.asarray(keys).reshape(-1).astype(np.int64)
    if n is None:
        n = table.shape[0] if table is not None else keys.shape[0] if keys is not None else (int(news.max()) + 1 if P else 1)
    if offsets is None:
        beg, length = np.zeros(R, dtype=np.int64), np.full(R, P, dtype=np.int64)
    else:
        off = np.clip(np.asarray(offsets).reshape(-1).astype(np.int64), 0, P)
        if off.shape[0] != R + 1:
            raise ValueError('offsets must have R + 1 = %d entries, got %d' % (R + 1, off.shape[0]))
        beg = off[:-1]
        length = np.maximum(off[1:], beg) - beg
    inside = (pos >= 0) & (pos < length[:, None])
    row = np.where(inside, beg[:, None] + pos, 0)
    nid = news[row] if P else np.zeros_like(row)
    filled = inside & (nid >= 0) & (nid < n)
    nid = np.where(filled, nid, 0)
    m = filled.sum(axis=1)
    skipped = np.zeros(R, dtype=bool) if skip is None else np.asarray(skip).reshape(-1).astype(bool)
    per = np.zeros((R, 8), dtype=np.float64)
    status = np.ones(R, dtype=np.int32)
    disc = 1.0 / np.log2(np.arange(k) + 2.0)
    if labels is not None:
        lab = np.asarray(labels).reshape(-1).astype(np.int64)
        seg = np.repeat(np.arange(R), length)
        rows = np.concatenate([np.arange(b, b + c) for b, c in zip(beg, length)]) if R else np.zeros(0, dtype=np.int64)
        n_pos = np.bincount(seg, weights=lab[rows] != 0, minlength=R).astype(np.int64)
        bad = np.bincount(seg, weights=(lab[rows] < 0) | (lab[rows] > 1), minlength=R) > 0
        status = np.where(skipped | (length == 0), 1, np.where(bad, 3, np.where((n_pos == 0) | (n_pos == length), 2, 0))).astype(np.int32)
        ok = status == 0
        gain = filled & (lab[row] != 0) if P else np.zeros_like(filled)
        dcg, ideal, hits = np.zeros(R), np.zeros(R), np.zeros(R, dtype=np.int64)
        first = np.full(R, -1, dtype=np.int64)
        for j in range(k):                                                    # slot order, one addition after the other
            dcg = np.where(gain[:, j], dcg + disc[j], dcg)
            ideal = np.where(j < n_pos, ideal + disc[j], ideal)
            hits += gain[:, j]
            first = np.where((first < 0) & gain[:, j], j, first)
        per[ok, 0] = dcg[ok] / ideal[ok]
        per[ok, 1] = np.where(first[ok] >= 0, 1.0 / (1.0 + np.maximum(first[ok], 0)), 0.0)
        per[ok, 2] = hits[ok] > 0
        per[ok, 3] = hits[ok] / n_pos[ok].astype(np.float64)
    if table is not None:
        step = max(1, (1 << 22) // max(1, k * table.shape[1]))
        upper = np.triu(np.ones((k, k), dtype=bool), 1)
        for r0 in range(0, R, step):
            f = filled[r0:r0 + step]
            x = table[nid[r0:r0 + step]] * f[:, :, None]                      # [rows, k, E]; an empty slot: zeros
            norm = np.sqrt((x * x).sum(axis=2))
            unit = np.divide(x, norm[:, :, None], out=np.zeros_like(x), where=norm[:, :, None] > 0)
            cos = unit @ unit.transpose(0, 2, 1)
            pairs = m[r0:r0 + step] * (m[r0:r0 + step] - 1) // 2
            total = (cos * upper).sum(axis=(1, 2))
            per[r0:r0 + step, 4] = np.where(pairs > 0, 1.0 - total / np.maximum(pairs, 1), 0.0)
    if keys is not None:
        key = np.where(filled, keys[nid], -1)
        if n_keys is not None:
            key = np.where(key < int(n_keys), key, -1)
        for j in range(k):
            seen = (key[:, :j] == key[:, j:j + 1]).any(axis=1) if j else np.zeros(R, dtype=bool)
            per[:, 5] += (key[:, j] >= 0) & ~seen
    per[:, 6] = m
    if value is not None:
        val = np.asarray(value, dtype=np.float32).reshape(-1).astype(np.float64)
        picked = np.where(filled, val[row], 0.0) if P else np.zeros(filled.shape)
        total = np.zeros(R)
        for j in range(k):
            total = np.where(filled[:, j], total + picked[:, j], total)
        per[:, 7] = np.where(m > 0, total / np.maximum(m, 1), 0.0)
    sets = (status == 0, ~skipped & (m >= 2), ~skipped & (m >= 1))
    counts = np.array([s.sum() for s in sets], dtype=np.int64)
    sums = np.array([per[sets[0 if c < 4 else 1 if c == 4 else 2], c].sum() for c in range(8)], dtype=np.float64)
    return per, status, sums, counts


# ---- explanations (Model.explain_lists / Model.explain): the score of a pair as a sum over the reader's history slots -------------------
EXPLAIN_BY = ('contribution', 'attention')
EXPLAIN_MAX_TOP = 16                  # lime_grouped_match_explain_f32's slots per pair
PairExplanation = collections.namedtuple('PairExplanation', 'logits base weight attn contrib top_slot top_value')


def lifetime_weight(remaining, alpha, beta, use_weight, use_penalty):
    """The remaining-lifetime weight (util.py:23-49) in fp64: 1 with ``use_weight`` off; sigmoid(alpha r), times beta where r < 0,
    with the expired penalty; sigmoid(alpha |r|) without."""
    r = np.asarray(remaining, dtype=np.float64)
    if not use_weight:
        return np.ones_like(r)
    with np.errstate(over='ignore'):
        if use_penalty:
            w = 1.0 / (1.0 + np.exp(-float(alpha) * r))
            return np.where(r >= 0, w, float(beta) * w)
        return 1.0 / (1.0 + np.exp(-float(alpha) * np.abs(r)))


def top_slots(values, eligible, m):
    """The selection rule of an explanation -> (top_slot int32 [P, m], top_value [P, m] in ``values``' dtype): per row of ``values``
    [P, H] the m slots of largest value among those ``eligible`` (bool [P, H]) -- larger value first; equal values (+0.0 == -0.0)
    lower slot first; a NaN behind every number (``walk_order``'s rule, in the values' own precision) --, and the value at each.
    Fewer than m eligible slots: the tail holds -1 / 0."""
    values = np.asarray(values)
    eligible = np.asarray(eligible).astype(bool)
    P, H = values.shape
    m = int(m)
    slot = np.full((P, m), -1, dtype=np.int32)
    top = np.zeros((P, m), dtype=values.dtype)
    for p in range(P):
        nan = np.isnan(values[p])
        order = np.argsort(-(np.where(nan, 0, values[p]) + 0.0), kind='stable')             # -0.0 + 0.0 = +0.0: the zeros tie
        order = order[np.argsort(nan[order], kind='stable')]
        order = order[eligible[p][order]][:m]
        slot[p, :order.size] = order
        top[p, :order.size] = values[p, order]
    return slot, top


def explain_pairs(kp, g, qp, cand, remaining, offsets, H, scale, alpha=0.0, beta=0.0, use_weight=False, use_penalty=False, mask=None,
                  hist_div=1, m=3, by='contribution', index=None, occ=None, qt=None, ct=None):
    """The host statement of ``ops.grouped_match_explain`` (lime_grouped_match_explain_f32), in fp64 -> PairExplanation.

    kp [G H, A], g [G H, D] per group; offsets [G + 1]: the pairs of group i are rows offsets[i] .. offsets[i + 1] - 1 (every offset
    clamped into [0, P]).  The pair's own operands: rows qp[p], cand[p]; with ``index`` [P] rows index[p] of the tables qp, cand
    (clamped into the tables); with ``occ`` [P], ``qt`` and ``ct`` besides, those rows plus rows occ[p] of qt, ct (clamped).  Per pair:
        s[h] = kp[i, h] . qp * scale     attn = softmax_h(s) -- UNMASKED --     m[h] = g[i, h] . cand
        base = sum_h attn[h] m[h]     weight = w(remaining[p]) (``lifetime_weight``)     logits = base weight
        contrib[h] = attn[h] m[h] weight                    so that       sum_h contrib[h] = logits
    and top_slot / top_value [P, m]: ``top_slots`` of contrib (``by`` 'contribution') or attn ('attention') among the slots h with
    mask[i // hist_div, h] set (mask [ceil(G / hist_div), H]; None: all).  A pair outside every group holds zeros and slots -1."""
    if by not in EXPLAIN_BY:
        raise ValueError("by must be 'contribution' or 'attention', got %r" % (by,))
    H, m, hist_div = int(H), int(m), int(hist_div)
    if not 1 <= m <= min(EXPLAIN_MAX_TOP, H) or hist_div < 1:
        raise ValueError('explain_pairs names 1 <= m <= min(%d, H = %d) slots with hist_div >= 1, got m = %d, hist_div = %d'
                         % (EXPLAIN_MAX_TOP, H, m, hist_div))
    f64 = lambda t: np.asarray(t, dtype=np.float64)
    kp, g, qp, cand = f64(kp), f64(g), f64(qp), f64(cand)
    if (occ is None) != (qt is None) or (occ is None) != (ct is None) or (occ is not None and index is None):
        raise ValueError('the occurrence-composed form takes index, occ, qt and ct together')
    if index is not None:
        at = np.clip(np.asarray(index).reshape(-1).astype(np.int64), 0, qp.shape[0] - 1)
        qp, cand = qp[at], cand[at]
        if occ is not None:
            z = np.clip(np.asarray(occ).reshape(-1).astype(np.int64), 0, f64(qt).shape[0] - 1)
            qp, cand = qp + f64(qt)[z], cand + f64(ct)[z]
    P, G = qp.shape[0], kp.shape[0] // H
    off = np.clip(np.asarray(offsets).reshape(-1).astype(np.int64), 0, P)
    weight = lifetime_weight(np.zeros(P) if remaining is None else f64(remaining).reshape(-1), alpha, beta, use_weight, use_penalty)
    attn, contrib, base = np.zeros((P, H)), np.zeros((P, H)), np.zeros(P)
    eligible = np.zeros((P, H), dtype=bool)
    mask = None if mask is None else np.asarray(mask).reshape(-1, H) != 0
    for i in range(G):
        lo, hi = off[i], max(off[i], off[i + 1])
        if hi == lo:
            continue
        s = qp[lo:hi] @ kp[i * H:(i + 1) * H].T * float(scale)                                  # [n, H]
        e = np.exp(s - s.max(axis=1, keepdims=True))
        attn[lo:hi] = e / e.sum(axis=1, keepdims=True)
        terms = attn[lo:hi] * (cand[lo:hi] @ g[i * H:(i + 1) * H].T)
        base[lo:hi] = terms.sum(axis=1)
        contrib[lo:hi] = terms * weight[lo:hi, None]
        eligible[lo:hi] = True if mask is None else mask[i // hist_div]
    slot, top = top_slots(contrib if by == 'contribution' else attn, eligible, m)
    return PairExplanation(base * weight, base, weight, attn, contrib, slot, top)
