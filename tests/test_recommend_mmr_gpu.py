"""Model.recommend / recommend_schedule / recommend_lists with ``mmr_lambda`` on the MI355X against the host composition: the entry's
OWN scores (score_pool / score_schedule / score_lists), the shortlist by ``recommend.quota_topk`` or a stable sort, then
``recommend.mmr_select`` over the similarity table -- held to the two checks of tests/test_mmr_gpu.py (greedy validity of the device's
picks within tol = 8 (E + 8) 2^-24 on every row; exact equality on the rows whose fp64 minimum gap exceeds 2 tol, at least half of
them) and to the score bits of the positions returned.  Tiny models as tests/test_recommend_quota_gpu.py builds them: LIME-CROWN-CROWN
'add', LIME-NAML-ATT 'gated' (the similarity table is a column view of the cache) and the baseline NAML-ATT; a corpus of 400 news, a
pool of 300, three users (one history empty), k = 5, shortlist 32.

A schedule's slot is compared bit for bit with ``recommend`` at the shifted freshness where ``score_schedule`` gives ``score_pool``'s
bits (the baseline and 'gated' on every route, 'add' on the shared user side, LIME_SCHEDULE_MATCH=0); on the factorised route of 'add'
the scores agree to rounding only, so there the slot is held to the composition over ``score_schedule``'s own scores."""
import numpy as np
import pytest
import torch

from lime_cikm25_amd import DeviceCorpus, Model, make_config, model as model_module, recommend, synth
from mmr_cases import check_exact, check_greedy, tolerance
from user_cases import _TINY

pytestmark = pytest.mark.gpu

U, UL, H, C, N_NEWS, K, M, Q = 3, 4, 5, 300, 400, 5, 32, 2
TOPICS = [(1, 3), (1, 7), (1, 9), (2, 5), (2, 6), (4, 9), (4, 1), (4, 2), (5, 2), (7, 7), (7, 8), (9, 1), (9, 2), (9, 3)]
LENS = [0, 1, 4, 40]
OFFSETS = [10.0, 3000.0, 0.0]
MODELS = {'lime_crown_crown_add': dict(content_encoder='CROWN', fusion_method='add'),
          'lime_naml_att_gated': dict(content_encoder='NAML', user_encoder='ATT', fusion_method='gated'),
          'baseline_naml_att': dict(news_encoder='NAML', user_encoder='ATT')}
_BUILT = {}


def build(name):
    if name in _BUILT:
        return _BUILT[name]
    assert torch.cuda.is_available(), 'these tests need the GPU'
    cfg = make_config(**{**_TINY, 'max_history_num': H, **MODELS[name]})
    corpus = synth.synth_corpus(cfg, n_news=N_NEWS, n_train=1, n_dev=1, seed=41)
    rng = np.random.default_rng(42)
    topic_of = np.minimum(rng.integers(0, len(TOPICS), size=N_NEWS), rng.integers(0, len(TOPICS), size=N_NEWS))
    pool = rng.permutation(np.arange(1, N_NEWS))[:C].astype(np.int32)
    corpus.news_category[1:] = np.array([TOPICS[t][0] for t in topic_of[1:]], dtype=np.int32)
    corpus.news_subCategory[1:] = np.array([TOPICS[t][1] for t in topic_of[1:]], dtype=np.int32)
    dc = DeviceCorpus(corpus)
    outside = np.setdiff1d(np.arange(1, N_NEWS), pool)
    hist = np.zeros((UL, H), dtype=np.int32)
    hist[0] = np.concatenate([pool[:3], rng.choice(outside, size=H - 3)])
    hist[1, :2] = [pool[4], outside[0]]
    hist[3] = pool[10:10 + H]
    mask = np.arange(H)[None, :] < np.array([H, 2, 0, H])[:, None]
    ufr = np.where(mask, np.exp(rng.uniform(np.log(60.0), np.log(30 * 86400.0), size=(UL, H))), 0.0).astype(np.float32)
    ult = np.where(mask, np.exp(rng.uniform(np.log(600.0), np.log(14 * 86400.0), size=(UL, H))), 0.0).astype(np.float32)
    cfr = np.exp(rng.uniform(np.log(60.0), np.log(3 * 86400.0), size=C)).astype(np.float32)
    delta = rng.uniform(-8.0, 8.0, size=(UL, C))
    delta[:, 0::6] = -5000.0
    delta[:, 1::6] = 5000.0
    clt = (cfr[None, :].astype(np.float64) + delta).astype(np.float32)
    torch.manual_seed(0)
    model = Model(cfg)
    model.initialize()
    synth.fill_state_dict(model, seed=43)
    model = model.cuda().eval()
    cache = model.build_news_cache(dc)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    side = lambda n: dict(news_cache=cache, corpus=dc, hist_index=t(hist[:n]), hist_mask=t(mask[:n]), user_freshness=t(ufr[:n]),
                          user_lifetime=t(ult[:n]))
    pool_args = dict(side(U), cand_index=t(pool), cand_freshness=t(cfr), cand_lifetime=t(clt[:U]))
    # the lists: 0, 1, 4 and 40 candidates; user 3's 40 begin with the five news of its own history
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    at = np.concatenate([[7], np.arange(20, 24), np.arange(10, 50)])
    user = np.repeat(np.arange(UL), LENS)
    list_args = dict(side(UL), cand_offsets=t(off), cand_index=t(pool[at]), cand_freshness=t(cfr[at]), cand_lifetime=t(clt[user, at]))
    keys = recommend.topic_table(corpus.news_category, corpus.news_subCategory, 'category')[0]
    in_hist = lambda u, news: np.array([int(n) in set(hist[u][mask[u]].tolist()) for n in news])
    gone_pool = np.stack([in_hist(u, pool) for u in range(U)])
    gone_list = np.concatenate([in_hist(u, pool[at][off[u]:off[u + 1]]) for u in range(UL)]).astype(bool)
    content = cache.cpu().numpy()
    if 'gated' in name:
        assert content.shape[1] % 2 == 0
        content = content[:, :content.shape[1] // 2]                          # the content columns of a 'gated' cache
    _BUILT[name] = (model, pool_args, list_args, keys, pool, pool[at], off, gone_pool, gone_list, content)
    return _BUILT[name]


def bits(t):
    return (t.cpu().numpy() if hasattr(t, 'cpu') else np.asarray(t)).view(np.int32)


def shortlist_of(scores, news, keys, gone, quota, m=M):
    """The host's shortlist of every row of scores [R, n]: ``recommend``'s order cut at ``m`` (a stable sort) or the quota walk; an
    excluded entry takes no part -> (positions [R, m], scores [R, m], ids [R, m]), -1 / -inf / -1 where there is none."""
    R = scores.shape[0]
    if quota:
        pos, top = recommend.quota_topk(scores, keys[news], m, Q, gone)
    else:
        pos, top = np.full((R, m), -1, dtype=np.int32), np.full((R, m), -np.inf, dtype=np.float32)
        for r in range(R):
            order = recommend.walk_order(scores[r])[:m]
            pos[r, :order.size], top[r, :order.size] = order, scores[r, order]
            if gone is not None:
                pos[r, :order.size][gone[r % gone.shape[0]][order]] = -1
    ids = np.where(pos >= 0, news[np.clip(pos, 0, None)], -1).astype(np.int32)
    return pos, top, ids


def hold(got, short, table, lam, k, what, exact=True):
    """A device slate (positions, scores) [R, k] against the host composition over the shortlist ``short``: the positions are
    shortlist entries, the scores their bits, and the picks behind them pass ``check_greedy`` and ``check_exact``."""
    pos, top = got[0].cpu().numpy(), got[1].cpu().numpy()
    spos, stop, ids = short
    R = spos.shape[0]
    assert pos.dtype == np.int32 and top.dtype == np.float32 and pos.shape == top.shape == (R, k), what
    picks = np.full((R, k), -1, dtype=np.int32)
    for r in range(R):
        rank = {int(p): j for j, p in enumerate(spos[r]) if p >= 0}
        for j in range(k):
            if pos[r, j] >= 0:
                assert int(pos[r, j]) in rank, '%s row %d: position %d is not in the shortlist' % (what, r, pos[r, j])
                picks[r, j] = rank[int(pos[r, j])]
                assert bits(top[r, j:j + 1]) == bits(stop[r, picks[r, j]:picks[r, j] + 1]), what
            else:
                assert np.isneginf(top[r, j]), what
    tol = tolerance(table.shape[1])
    check_greedy(picks, stop, ids, table, lam, tol, what)
    want, gap = recommend.mmr_select(stop, ids, table, lam, k, return_gap=True)
    print('%s: E %d tol %.3g, fp64 minimum gaps %s, %d of %d picks equal' % (what, table.shape[1], tol, np.array2string(gap, precision=3),
                                                                            int((picks == want).sum()), picks.size))
    if exact:
        check_exact(picks, want, gap, tol, what)
    return picks


@pytest.mark.parametrize('name', list(MODELS))
def test_lambda_one_is_the_call_without_it(name):
    model, pool_args, list_args, *_ = build(name)
    for kw in (dict(), dict(max_per_topic=Q), dict(exclude_history=True, max_per_topic=Q)):
        for call, args in ((model.recommend, pool_args), (model.recommend_lists, list_args)):
            a, b = call(**args, k=K, **kw), call(**args, k=K, mmr_lambda=1.0, shortlist=M, **kw)
            assert torch.equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])), (name, kw)


@pytest.mark.parametrize('name', list(MODELS))
@pytest.mark.parametrize('quota', [False, True])
@pytest.mark.parametrize('exclude', [False, True])
def test_recommend_is_mmr_select_over_the_shortlist_of_score_pool(name, quota, exclude):
    model, pool_args, _, keys, pool, _, _, gone, _, content = build(name)
    what = '%s quota %s exclude %s' % (name, quota, exclude)
    scores = model.score_pool(**pool_args, exclude_history=exclude).cpu().numpy()
    kw = dict(k=K, mmr_lambda=0.5, shortlist=M, exclude_history=exclude, max_per_topic=Q if quota else None)
    got = model.recommend(**pool_args, **kw)
    short = shortlist_of(scores, pool, keys, gone if exclude else None, quota)
    hold(got, short, content, 0.5, K, what)
    pos = got[0].cpu().numpy()
    assert (pos >= 0).all() and all(len(set(p.tolist())) == K for p in pos)
    if exclude:                                                               # nothing the user has read, shortlisted or taken
        assert gone.sum(axis=1).tolist() == [3, 1, 0] and not gone[np.arange(U)[:, None], pos].any()
        assert not quota or not gone[np.arange(U)[:, None], np.clip(short[0], 0, None)][short[0] >= 0].any()
    if quota:
        assert all(np.bincount(keys[pool][p]).max() <= Q for p in pos)
    again = model.recommend(**pool_args, **kw)
    assert torch.equal(again[0], got[0]) and np.array_equal(bits(again[1]), bits(got[1]))
    default = model.recommend(**pool_args, **{**kw, 'shortlist': None})       # the default shortlist: min(128, max(k, 64)) = 64
    hold(default, shortlist_of(scores, pool, keys, gone if exclude else None, quota, m=64), content, 0.5, K, what + ' shortlist 64', exact=False)


def test_an_excluded_shortlist_entry_is_never_taken():
    """A pool of ten news that the shortlist holds whole: user 0 has read three of them and user 1 one, so the shortlist itself carries
    excluded entries (-inf, no id) -- the slates are the seven, nine and ten others, then -1."""
    model, pool_args, _, keys, pool, _, _, gone, _, content = build('baseline_naml_att')
    args = dict(pool_args, cand_index=pool_args['cand_index'][:10].contiguous(), cand_freshness=pool_args['cand_freshness'][:10].contiguous(),
                cand_lifetime=pool_args['cand_lifetime'][:, :10].contiguous())
    scores = model.score_pool(**args, exclude_history=True).cpu().numpy()
    assert np.isneginf(scores).sum(axis=1).tolist() == [3, 1, 0]
    got = model.recommend(**args, k=10, mmr_lambda=0.5, shortlist=10, exclude_history=True)
    short = shortlist_of(scores, pool[:10], keys, gone[:, :10], False, m=10)
    assert (short[2] < 0).sum(axis=1).tolist() == [3, 1, 0]                   # the shortlist's excluded entries
    hold(got, short, content, 0.5, 10, 'excluded in the shortlist', exact=False)
    pos = got[0].cpu().numpy()
    assert (pos >= 0).sum(axis=1).tolist() == [7, 9, 10] and (pos[0, 7:] == -1).all() and torch.isneginf(got[1][0, 7:]).all()
    assert not gone[:, :10][np.arange(U)[:, None], np.clip(pos, 0, None)][pos >= 0].any()


@pytest.mark.parametrize('name', list(MODELS))
def test_every_slot_of_a_schedule_is_recommend_at_the_shifted_freshness(name, monkeypatch):
    model, pool_args, _, keys, pool, _, _, gone, _, content = build(name)
    S = len(OFFSETS)
    slots = torch.tensor(OFFSETS, dtype=torch.float32, device='cuda')
    kw = dict(k=K, mmr_lambda=0.5, shortlist=M, max_per_topic=Q, exclude_history=True)
    pos, top = model.recommend_schedule(**pool_args, slot_offsets=slots, **kw)
    assert pos.shape == top.shape == (S, U, K) and pos.dtype == torch.int32 and top.dtype == torch.float32
    scores = model.score_schedule(**pool_args, slot_offsets=slots, exclude_history=True).cpu().numpy()
    for s in range(S):
        # (greedy validity alone: the user without a history scores whole topics alike, and a slot can tie two of its three rows)
        hold((pos[s], top[s]), shortlist_of(scores[s], pool, keys, gone, True), content, 0.5, K, '%s slot %d' % (name, s), exact=False)
    if model.schedule_route(S, H) == 'factorised' and not model.plain:       # the route that gives score_pool's bits
        monkeypatch.setattr(model_module, 'SCHEDULE_MATCH', False)
        pos, top = model.recommend_schedule(**pool_args, slot_offsets=slots, **kw)
    for s, offset in enumerate(OFFSETS):
        pos0, top0 = model.recommend(**dict(pool_args, cand_freshness=pool_args['cand_freshness'] + offset), **kw)
        assert torch.equal(pos[s], pos0) and np.array_equal(bits(top[s]), bits(top0)), '%s slot %d' % (name, s)


@pytest.mark.parametrize('name', list(MODELS))
@pytest.mark.parametrize('quota', [False, True])
def test_recommend_lists_counts_within_the_list(name, quota):
    model, _, list_args, keys, _, news, off, _, gone, content = build(name)
    what = '%s lists quota %s' % (name, quota)
    scores = model.score_lists(**list_args, exclude_history=True).cpu().numpy()
    got = model.recommend_lists(**list_args, k=K, mmr_lambda=0.5, shortlist=M, exclude_history=True, max_per_topic=Q if quota else None)
    pos = got[0].cpu().numpy()
    assert pos.shape == (UL, K) and (pos[0] == -1).all() and torch.isneginf(got[1][0]).all()      # the empty list
    assert pos[1].tolist() == [0] + [-1] * (K - 1)
    if not quota:
        assert sorted(pos[2, :4].tolist()) == [0, 1, 2, 3] and pos[2, 4] == -1                    # its four, then -1
    shorts = []
    for u in range(1, UL):                                                    # each list is a one-row pool of its own
        a, b = off[u], off[u + 1]
        shorts.append(shortlist_of(scores[None, a:b], news[a:b], keys, gone[None, a:b], quota))
        live = pos[u][pos[u] >= 0]
        assert (live < b - a).all() and not gone[a + live].any()
    hold((got[0][1:], got[1][1:]), tuple(np.concatenate([s[i] for s in shorts]) for i in range(3)), content, 0.5, K, what)
    assert gone.sum() == 5 and (pos[3] >= 0).all()


def test_a_callers_similarity_table_changes_the_slate_as_mmr_select_says():
    model, pool_args, _, keys, pool, _, _, _, _, content = build('baseline_naml_att')
    rng = np.random.default_rng(5)
    table = (rng.standard_normal((4, 8))[rng.integers(0, 4, size=N_NEWS)] + 0.2 * rng.standard_normal((N_NEWS, 8))).astype(np.float32)
    scores = model.score_pool(**pool_args).cpu().numpy()
    short = shortlist_of(scores, pool, keys, None, False)
    got = model.recommend(**pool_args, k=K, mmr_lambda=0.5, shortlist=M, similarity=torch.from_numpy(table).cuda())
    picks = hold(got, short, table, 0.5, K, 'similarity [n, 8]')
    own = recommend.mmr_select(short[1], short[2], content, 0.5, K)
    assert not np.array_equal(picks, own), 'the caller\'s table chose the slate the content would have chosen: the case shows nothing'
