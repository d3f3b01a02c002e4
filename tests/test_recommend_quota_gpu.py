"""Model.recommend / recommend_schedule / recommend_lists with ``max_per_topic`` on the MI355X: the slates equal
``recommend.quota_topk`` -- the host statement of the quota walk -- over the entry's OWN scores (score_pool / score_schedule /
score_lists) and the corpus' group keys, positions and score bits.  Small models as tests/test_recommend_gpu.py builds them
(LIME-CROWN-CROWN and the baseline NAML-ATT), a corpus of 400 news over six categories (fourteen topics), a pool of 300, four users
with H = 5 (one history empty; the pool entries use the first three), k = 10, max_per_topic = 2.

A schedule's slot s is held against ``recommend`` at ``cand_freshness + slot_offsets[s]`` bit for bit where ``score_schedule`` gives
``score_pool``'s bits -- the baseline on every route, a LIME model on the shared user side (LIME_SCHEDULE_MATCH=0) --; on the factorised
route of a LIME model the scores agree to fp32 rounding only (tests/test_schedule_model_gpu.py), so there the slot is held against the
walk over ``score_schedule``'s own scores."""
import numpy as np
import pytest
import torch

from lime_cikm25_amd import DeviceCorpus, Model, make_config, model as model_module, recommend, synth
from quota_cases import same
from user_cases import _TINY

pytestmark = pytest.mark.gpu

U, UL, H, C, N_NEWS, K, Q = 3, 4, 5, 300, 400, 10, 2
TOPICS = [(1, 3), (1, 7), (1, 9), (2, 5), (2, 6), (4, 9), (4, 1), (4, 2), (5, 2), (7, 7), (7, 8), (9, 1), (9, 2), (9, 3)]
LENS = [0, 1, 7, 130]
OFFSETS = [10.0, 3000.0, 0.0]
MODELS = {'lime_crown_crown': dict(content_encoder='CROWN'), 'baseline_naml_att': dict(news_encoder='NAML', user_encoder='ATT')}
_BUILT = {}


def build(name):
    if name in _BUILT:
        return _BUILT[name]
    assert torch.cuda.is_available(), 'these tests need the GPU'
    cfg = make_config(**{**_TINY, 'max_history_num': H, **MODELS[name]})
    corpus = synth.synth_corpus(cfg, n_news=N_NEWS, n_train=1, n_dev=1, seed=41)
    rng = np.random.default_rng(42)
    topic_of = np.minimum(rng.integers(0, len(TOPICS), size=N_NEWS), rng.integers(0, len(TOPICS), size=N_NEWS))   # skewed: early topics crowd
    pool = rng.permutation(np.arange(1, N_NEWS))[:C].astype(np.int32)
    topic_of[pool[150:150 + 2 * len(TOPICS)]] = np.repeat(np.arange(len(TOPICS)), 2)     # every topic is in the pool (and in user 3's list)
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
    # the lists: 0, 1, 7 and 130 candidates; user 3's 130 begin with the five news of its own history
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    at = np.concatenate([[7], np.arange(20, 27), np.arange(10, 140)])
    user = np.repeat(np.arange(UL), LENS)
    list_args = dict(side(UL), cand_offsets=t(off), cand_index=t(pool[at]), cand_freshness=t(cfr[at]), cand_lifetime=t(clt[user, at]))
    keys = {by: recommend.topic_table(corpus.news_category, corpus.news_subCategory, by)[0] for by in ('category', 'topic')}
    in_hist = lambda u, news: np.array([int(n) in set(hist[u][mask[u]].tolist()) for n in news])
    gone_pool = np.stack([in_hist(u, pool) for u in range(U)])
    gone_list = np.concatenate([in_hist(u, pool[at][off[u]:off[u + 1]]) for u in range(UL)]).astype(bool)
    _BUILT[name] = (model, pool_args, list_args, keys, pool, pool[at], off, gone_pool, gone_list)
    return _BUILT[name]


def test_the_fixture_makes_the_quota_bind():
    model, pool_args, _, keys, pool, *_ = build('lime_crown_crown')
    assert len(set(keys['category'][pool].tolist())) == 6 and len(set(keys['topic'][pool].tolist())) == len(TOPICS)
    plain = model.recommend(**pool_args, k=K)[0].cpu().numpy()
    assert max(np.bincount(keys['category'][pool][plain[u]]).max() for u in range(U)) > Q, 'no slate is crowded: the quota would not be felt'


@pytest.mark.parametrize('name', list(MODELS))
@pytest.mark.parametrize('quota_by', ['category', 'topic'])
@pytest.mark.parametrize('exclude', [False, True])
def test_recommend_is_the_quota_walk_over_score_pool(name, quota_by, exclude):
    model, pool_args, _, keys, pool, _, _, gone, _ = build(name)
    scores = model.score_pool(**pool_args, exclude_history=exclude).cpu().numpy()
    pos, top = model.recommend(**pool_args, k=K, max_per_topic=Q, quota_by=quota_by, exclude_history=exclude)
    g = keys[quota_by][pool]
    same((pos, top), recommend.quota_topk(scores, g, K, Q, gone if exclude else None), '%s %s' % (name, quota_by))
    pos = pos.cpu().numpy()
    assert gone.sum(axis=1).tolist() == [3, 1, 0]
    for u in range(U):
        assert (pos[u] >= 0).all() and len(set(pos[u].tolist())) == K
        assert np.bincount(g[pos[u]]).max() <= Q                              # no group more than twice
        if exclude:
            assert not gone[u][pos[u]].any()                                  # nothing the user has read
    again = model.recommend(**pool_args, k=K, max_per_topic=Q, quota_by=quota_by, exclude_history=exclude)
    assert torch.equal(again[0].cpu(), torch.from_numpy(pos)) and torch.equal(again[1].view(torch.int32), top.view(torch.int32))


@pytest.mark.parametrize('name', list(MODELS))
def test_a_quota_changes_the_slate_only_where_it_binds(name):
    model, pool_args, _, keys, pool, *_ = build(name)
    plain = model.recommend(**pool_args, k=K)
    loose = model.recommend(**pool_args, k=K, max_per_topic=K)
    assert torch.equal(plain[0], loose[0]) and torch.equal(plain[1].view(torch.int32), loose[1].view(torch.int32))
    tight = model.recommend(**pool_args, k=K, max_per_topic=1, quota_by='category')     # six categories: six news, then nothing
    assert (tight[0][:, :6] >= 0).all() and (tight[0][:, 6:] == -1).all() and torch.isneginf(tight[1][:, 6:]).all()


@pytest.mark.parametrize('name', list(MODELS))
@pytest.mark.parametrize('exclude', [False, True])
def test_every_slot_of_a_schedule_is_recommend_at_the_shifted_freshness(name, exclude, monkeypatch):
    model, pool_args, _, keys, pool, _, _, gone, _ = build(name)
    S = len(OFFSETS)
    slots = torch.tensor(OFFSETS, dtype=torch.float32, device='cuda')
    kw = dict(k=K, max_per_topic=Q, quota_by='topic', exclude_history=exclude)
    pos, top = model.recommend_schedule(**pool_args, slot_offsets=slots, **kw)
    assert pos.shape == top.shape == (S, U, K) and pos.dtype == torch.int32 and top.dtype == torch.float32
    scores = model.score_schedule(**pool_args, slot_offsets=slots, exclude_history=exclude).cpu().numpy()
    g = keys['topic'][pool]
    for s in range(S):
        same((pos[s], top[s]), recommend.quota_topk(scores[s], g, K, Q, gone if exclude else None), '%s slot %d' % (name, s))
    if name == 'lime_crown_crown':                                            # the route that gives score_pool's bits
        assert model.schedule_route(S, H) == 'factorised'
        monkeypatch.setattr(model_module, 'SCHEDULE_MATCH', False)
        pos, top = model.recommend_schedule(**pool_args, slot_offsets=slots, **kw)
    for s, offset in enumerate(OFFSETS):
        pos0, top0 = model.recommend(**dict(pool_args, cand_freshness=pool_args['cand_freshness'] + offset), **kw)
        assert torch.equal(pos[s], pos0) and torch.equal(top[s].view(torch.int32), top0.view(torch.int32)), '%s slot %d' % (name, s)


@pytest.mark.parametrize('name', list(MODELS))
@pytest.mark.parametrize('quota_by', ['category', 'topic'])
@pytest.mark.parametrize('exclude', [False, True])
def test_recommend_lists_is_the_quota_walk_over_score_lists(name, quota_by, exclude):
    model, _, list_args, keys, _, news, off, _, gone = build(name)
    scores = model.score_lists(**list_args, exclude_history=exclude).cpu().numpy()
    pos, top = model.recommend_lists(**list_args, k=K, max_per_topic=Q, quota_by=quota_by, exclude_history=exclude)
    g = keys[quota_by][news]
    same((pos, top), recommend.quota_topk_segments(scores, off, g, K, Q, gone if exclude else None), '%s %s' % (name, quota_by))
    pos = pos.cpu().numpy()
    assert gone.sum() == 5 and (pos[0] == -1).all() and pos[1].tolist() == [0] + [-1] * (K - 1)
    for u in range(UL):
        live = pos[u][pos[u] >= 0]
        assert len(live) == 0 or np.bincount(g[off[u] + live]).max() <= Q
        assert not exclude or not gone[off[u] + live].any()
    assert (pos[3] >= 0).all()


@pytest.mark.parametrize('name', list(MODELS))
def test_no_quota_is_the_call_without_the_argument(name):
    model, pool_args, list_args, *_ = build(name)
    slots = torch.tensor(OFFSETS, dtype=torch.float32, device='cuda')
    for exclude in (False, True):
        for call, args in ((model.recommend, pool_args), (model.recommend_lists, list_args),
                           (lambda **kw: model.recommend_schedule(slot_offsets=slots, **kw), pool_args)):
            a = call(**args, k=K, exclude_history=exclude)
            b = call(**args, k=K, exclude_history=exclude, max_per_topic=None, quota_by='topic')
            assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
