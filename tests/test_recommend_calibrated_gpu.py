"""Model.recommend / recommend_schedule / recommend_lists with ``calibrate_lambda`` on the MI355X against the host composition: the
entry's OWN scores (score_pool / score_schedule / score_lists), the shortlist by ``recommend.quota_topk`` or a stable sort, the history
keys from the corpus' topic table, then ``recommend.calibrated_select`` -- held to the two checks of tests/test_calibrate_gpu.py (greedy
validity of the device's picks within ``calibrate_cases.tolerance`` on every row; exact equality on the rows whose fp64 minimum gap
exceeds 2 tol) and to the score bits of the positions returned.  Tiny models as tests/test_recommend_mmr_gpu.py builds them (LIME over
CROWN with 'add', and the baseline NAML + ATT); a corpus of 120 news in 6 categories, U = 4 users with H = 6 (one history empty, one
half masked), a pool of 40, lists of 0 / 3 / 15 / 15 rows, S = 3 slots, k = 5, shortlist 16.

The sweep: ``calibration='category'`` adds 'miscalibration' and 'n_calibration', held to ``recommend.slate_miscalibration`` over the
same slates; without it the key set is what it was; and on scores that one category dominates the calibrated setting's miscalibration
is lower than the plain one's."""
import numpy as np
import pytest
import torch

from lime_cikm25_amd import DeviceBehaviors, DeviceCorpus, Model, evaluate as E, make_config, model as model_module, recommend, serving, synth
from lime_cikm25_amd import util as Ut
from calibrate_cases import check_greedy, metric_bound, sure_rows, tolerance
from slate_cases import dev_split
from user_cases import _TINY

pytestmark = pytest.mark.gpu

U, H, C, N_NEWS, K, M, Q, LAM, ALPHA = 4, 6, 40, 120, 5, 16, 2, 0.1, recommend.CALIBRATE_ALPHA
LENS = [0, 3, 15, 15]
OFFSETS = [10.0, 3000.0, 0.0]
MODELS = {'lime_crown_crown_add': dict(content_encoder='CROWN', fusion_method='add'),
          'baseline_naml_att': dict(news_encoder='NAML', user_encoder='ATT')}
_BUILT = {}


def build(name):
    if name in _BUILT:
        return _BUILT[name]
    assert torch.cuda.is_available(), 'these tests need the GPU'
    cfg = make_config(**{**_TINY, 'max_history_num': H, **MODELS[name]})
    corpus = synth.synth_corpus(cfg, n_news=N_NEWS, n_train=1, n_dev=1, seed=41)
    rng = np.random.default_rng(42)
    corpus.news_category[1:] = rng.integers(1, 7, size=N_NEWS - 1).astype(np.int32)
    corpus.news_subCategory[1:] = rng.integers(1, 4, size=N_NEWS - 1).astype(np.int32)
    dc = DeviceCorpus(corpus)
    pool = rng.permutation(np.arange(1, N_NEWS))[:C].astype(np.int32)
    outside = np.setdiff1d(np.arange(1, N_NEWS), pool)
    hist = np.zeros((U, H), dtype=np.int32)
    hist[0] = np.concatenate([pool[:3], rng.choice(outside, size=H - 3)])     # three of the pool: excluded under exclude_history
    hist[1] = rng.choice(outside, size=H)
    hist[3] = pool[10:10 + H]
    mask = np.arange(H)[None, :] < np.array([H, 3, 0, H])[:, None]            # user 1 half masked, user 2 without a history
    ufr = np.where(mask, np.exp(rng.uniform(np.log(60.0), np.log(30 * 86400.0), size=(U, H))), 0.0).astype(np.float32)
    ult = np.where(mask, np.exp(rng.uniform(np.log(600.0), np.log(14 * 86400.0), size=(U, H))), 0.0).astype(np.float32)
    cfr = np.exp(rng.uniform(np.log(60.0), np.log(3 * 86400.0), size=C)).astype(np.float32)
    clt = (cfr[None, :].astype(np.float64) + rng.uniform(-8.0, 8.0, size=(U, C))).astype(np.float32)
    torch.manual_seed(0)
    model = Model(cfg)
    model.initialize()
    synth.fill_state_dict(model, seed=43)
    model = model.cuda().eval()
    cache = model.build_news_cache(dc)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    side = dict(news_cache=cache, corpus=dc, hist_index=t(hist), hist_mask=t(mask), user_freshness=t(ufr), user_lifetime=t(ult))
    pool_args = dict(side, cand_index=t(pool), cand_freshness=t(cfr), cand_lifetime=t(clt))
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    at = np.concatenate([np.arange(20, 23), np.arange(0, 15), np.arange(10, 25)])
    user = np.repeat(np.arange(U), LENS)
    list_args = dict(side, cand_offsets=t(off), cand_index=t(pool[at]), cand_freshness=t(cfr[at]), cand_lifetime=t(clt[user, at]))
    keys = {by: recommend.topic_table(corpus.news_category, corpus.news_subCategory, by)[0] for by in ('category', 'topic')}
    in_hist = lambda u, news: np.array([int(n) in set(hist[u][mask[u]].tolist()) for n in news])
    gone_pool = np.stack([in_hist(u, pool) for u in range(U)])
    gone_list = np.concatenate([in_hist(u, pool[at][off[u]:off[u + 1]]) for u in range(U)]).astype(bool)
    _BUILT[name] = (model, pool_args, list_args, keys, pool, pool[at], off, gone_pool, gone_list, hist, mask)
    return _BUILT[name]


def bits(t):
    return (t.cpu().numpy() if hasattr(t, 'cpu') else np.asarray(t)).view(np.int32)


def shortlist_of(scores, news, keys, gone, quota, m=M):
    """The host's shortlist of every row of scores [R, n]: ``recommend``'s order cut at ``m`` (a stable sort) or the quota walk; an
    excluded entry takes no part -> (positions [R, m], scores [R, m], ids [R, m]), -1 / -inf / -1 where there is none."""
    R = scores.shape[0]
    m = min(m, 128)
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


def hold(got, short, keys, hist_keys, weights, lam, k, what, alpha=ALPHA):
    """A device slate (positions, scores) [R, k] against the host composition over the shortlist ``short``: the positions are
    shortlist entries, the scores their bits, and the picks behind them are greedy within tol and the statement's on the sure rows."""
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
    n_keys = int(keys.max()) + 1
    c = dict(scores=stop, ids=ids, keys=keys, n_keys=n_keys, hist_keys=hist_keys, weights=weights)
    tol = tolerance(hist_keys.shape[1], alpha)
    check_greedy(picks, c, lam, alpha, tol, what)
    want, gap = recommend.calibrated_select(stop, ids, keys, n_keys, hist_keys, weights, lam, alpha, k, return_gap=True)
    sure = sure_rows(gap, tol)
    print('%s: tol %.3g, fp64 minimum gaps %s, %d of %d rows sure' % (what, tol, np.array2string(gap, precision=3), int(sure.sum()), R))
    assert np.array_equal(picks[sure], want[sure]), what
    return picks, want, sure


def hist_keys_of(keys, hist, mask):
    return np.where(mask, keys[hist], -1).astype(np.int32)


@pytest.mark.parametrize('name', list(MODELS))
def test_lambda_one_and_none_are_the_call_without_it(name):
    model, pool_args, list_args, *_ = build(name)
    slots = torch.tensor(OFFSETS, dtype=torch.float32, device='cuda')
    for kw in (dict(), dict(max_per_topic=Q), dict(exclude_history=True, max_per_topic=Q)):
        for call, args in ((model.recommend, pool_args), (model.recommend_lists, list_args),
                           (model.recommend_schedule, dict(pool_args, slot_offsets=slots))):
            a = call(**args, k=K, **kw)
            b = call(**args, k=K, calibrate_lambda=1.0, shortlist=M, **kw)
            c = call(**args, k=K, calibrate_lambda=None, calibrate_by='category', calibrate_alpha=ALPHA, calibrate_weights=None, **kw)
            assert torch.equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])), (name, kw)
            assert torch.equal(a[0], c[0]) and np.array_equal(bits(a[1]), bits(c[1])), (name, kw)


@pytest.mark.parametrize('name', list(MODELS))
@pytest.mark.parametrize('quota,exclude,by,weighted', [(False, False, 'category', False), (True, False, 'topic', False),
                                                       (False, True, 'category', True), (True, True, 'category', True)])
def test_recommend_is_calibrated_select_over_the_shortlist_of_score_pool(name, quota, exclude, by, weighted):
    model, pool_args, _, keys, pool, _, _, gone, _, hist, mask = build(name)
    what = '%s quota %s exclude %s by %s weighted %s' % (name, quota, exclude, by, weighted)
    weights = np.random.default_rng(3).choice(np.array([0.0, 0.25, 0.5, 1.0], dtype=np.float32), size=(U, H)) if weighted else None
    scores = model.score_pool(**pool_args, exclude_history=exclude).cpu().numpy()
    kw = dict(k=K, calibrate_lambda=LAM, calibrate_by=by, shortlist=M, exclude_history=exclude, max_per_topic=Q if quota else None,
              calibrate_weights=None if weights is None else torch.from_numpy(weights).cuda())
    got = model.recommend(**pool_args, **kw)
    short = shortlist_of(scores, pool, keys['category'], gone if exclude else None, quota)
    picks, want, sure = hold(got, short, keys[by], hist_keys_of(keys[by], hist, mask), weights, LAM, K, what)
    pos = got[0].cpu().numpy()
    assert (pos >= 0).all() and all(len(set(p.tolist())) == K for p in pos)
    assert np.array_equal(picks[2], np.arange(K))                             # the user without a history: the plain slate
    if exclude:
        assert gone.sum(axis=1).tolist() == [3, 0, 0, H] and not gone[np.arange(U)[:, None], pos].any()
    if quota:
        assert all(np.bincount(keys['category'][pool][p]).max() <= Q for p in pos)
    again = model.recommend(**pool_args, **kw)
    assert torch.equal(again[0], got[0]) and np.array_equal(bits(again[1]), bits(got[1]))
    default = model.recommend(**pool_args, **{**kw, 'shortlist': None})       # the default shortlist: min(128, max(k, 64)) = 64 > C
    hold(default, shortlist_of(scores, pool, keys['category'], gone if exclude else None, quota, m=64), keys[by],
         hist_keys_of(keys[by], hist, mask), weights, LAM, K, what + ' shortlist 64')
    other = model.recommend(**pool_args, **{**kw, 'calibrate_alpha': 0.1})
    hold(other, short, keys[by], hist_keys_of(keys[by], hist, mask), weights, LAM, K, what + ' alpha 0.1', alpha=0.1)


def test_calibration_moves_the_slate_towards_the_history():
    """lam = 0 is the calibration alone: some slate differs from the plain one, and the slates are nearer to their histories."""
    model, pool_args, _, keys, pool, _, _, _, _, hist, mask = build('baseline_naml_att')
    plain = model.recommend(**pool_args, k=K)[0].cpu().numpy()
    cal = model.recommend(**pool_args, k=K, calibrate_lambda=0.0, shortlist=M)[0].cpu().numpy()
    hk = hist_keys_of(keys['category'], hist, mask)
    miss = lambda p: recommend.slate_miscalibration(p, K, None, pool, keys['category'], int(keys['category'].max()) + 1, hk)
    (v_plain, s_plain), (v_cal, s_cal) = miss(plain), miss(cal)
    assert s_plain.tolist() == s_cal.tolist() == [0, 0, 1, 0] and not np.array_equal(plain, cal) and np.array_equal(plain[2], cal[2])
    print('miscalibration plain %s calibrated %s' % (v_plain, v_cal))
    assert v_cal.sum() < v_plain.sum()


@pytest.mark.parametrize('name', list(MODELS))
def test_every_slot_of_a_schedule_is_recommend_at_the_shifted_freshness(name, monkeypatch):
    model, pool_args, _, keys, pool, _, _, gone, _, hist, mask = build(name)
    S = len(OFFSETS)
    slots = torch.tensor(OFFSETS, dtype=torch.float32, device='cuda')
    kw = dict(k=K, calibrate_lambda=LAM, shortlist=M, max_per_topic=Q, exclude_history=True)
    pos, top = model.recommend_schedule(**pool_args, slot_offsets=slots, **kw)
    assert pos.shape == top.shape == (S, U, K) and pos.dtype == torch.int32 and top.dtype == torch.float32
    scores = model.score_schedule(**pool_args, slot_offsets=slots, exclude_history=True).cpu().numpy()
    hk = hist_keys_of(keys['category'], hist, mask)
    for s in range(S):                                                        # row s U + u reads user u's history
        hold((pos[s], top[s]), shortlist_of(scores[s], pool, keys['category'], gone, True), keys['category'], hk, None, LAM, K,
             '%s slot %d' % (name, s))
    if model.schedule_route(S, H) == 'factorised' and not model.plain:       # the route that gives score_pool's bits
        monkeypatch.setattr(model_module, 'SCHEDULE_MATCH', False)
        pos, top = model.recommend_schedule(**pool_args, slot_offsets=slots, **kw)
    for s, offset in enumerate(OFFSETS):
        pos0, top0 = model.recommend(**dict(pool_args, cand_freshness=pool_args['cand_freshness'] + offset), **kw)
        assert torch.equal(pos[s], pos0) and np.array_equal(bits(top[s]), bits(top0)), '%s slot %d' % (name, s)


@pytest.mark.parametrize('name', list(MODELS))
@pytest.mark.parametrize('quota', [False, True])
def test_recommend_lists_counts_within_the_list(name, quota):
    model, _, list_args, keys, _, news, off, _, gone, hist, mask = build(name)
    what = '%s lists quota %s' % (name, quota)
    scores = model.score_lists(**list_args, exclude_history=True).cpu().numpy()
    got = model.recommend_lists(**list_args, k=K, calibrate_lambda=LAM, shortlist=M, exclude_history=True, max_per_topic=Q if quota else None)
    pos = got[0].cpu().numpy()
    assert pos.shape == (U, K) and (pos[0] == -1).all() and torch.isneginf(got[1][0]).all()       # the empty list
    if not quota:
        assert sorted(pos[1, :3].tolist()) == [0, 1, 2] and (pos[1, 3:] == -1).all()              # its three, then -1
    shorts = []
    for u in range(1, U):                                                     # each list is a one-row pool of its own
        a, b = off[u], off[u + 1]
        shorts.append(shortlist_of(scores[None, a:b], news[a:b], keys['category'], gone[None, a:b], quota))
        live = pos[u][pos[u] >= 0]
        assert (live < b - a).all() and not gone[a + live].any()
    hk = hist_keys_of(keys['category'], hist, mask)
    hold((got[0][1:], got[1][1:]), tuple(np.concatenate([s[i] for s in shorts]) for i in range(3)), keys['category'], hk[1:], None, LAM, K, what)


# ---- the sweep -----------------------------------------------------------------------------------------------------------------------
_SPLIT = {}


def split():
    if not _SPLIT:
        corpus, model, indices, labels = dev_split('naml_att', seed=71, one_class=True)
        _SPLIT['s'] = (model, DeviceBehaviors.from_devtest(DeviceCorpus(corpus), corpus, 'dev'), indices, labels)
    return _SPLIT['s']


def test_the_sweep_measures_miscalibration_as_the_statement_does():
    model, dev, indices, labels = split()
    cache = model.build_news_cache(dev.corpus)
    scores = model.score_behaviors(dev, torch.arange(dev.num, device='cuda'), cache, n_src=min(dev.num, dev.hist_index.shape[1] + model.config.batch_size)).float()
    settings = [{}, {'calibrate_lambda': 0.0, 'shortlist': 8}, {'calibrate_lambda': 0.2, 'calibrate_by': 'topic', 'calibrate_alpha': 0.1},
                {'max_per_topic': 1, 'calibrate_lambda': 0.0, 'shortlist': 8}]
    today = Ut.sweep_slate_settings(model, dev, cache, scores, indices, labels, settings, K)
    assert all(set(r) == set(Ut.SLATE_RESULT_KEYS) | {'n_relevance', 'n_diversity', 'n_slates'} for r in today)    # today's keys
    offsets, _, skip = E.impression_layout(indices, labels)
    first = np.minimum(offsets[:-1], dev.num - 1)
    hist, mask = dev.hist_index.cpu().numpy()[first], dev.hist_mask.cpu().numpy()[first].astype(bool)
    cand = dev.cand_index.reshape(-1)
    a32 = float(np.float32(ALPHA))
    for calibration in ('category', 'topic'):
        results = Ut.sweep_slate_settings(model, dev, cache, scores, indices, labels, settings, K, per_impression=True, calibration=calibration)
        keys = recommend.topic_table(dev.corpus.news_category.cpu().numpy(), dev.corpus.news_subCategory.cpu().numpy(), calibration)[0]
        n_keys = int(keys.max()) + 1
        for setting, res, old in zip(settings, results, today):
            assert set(res) == set(old) | {'miscalibration', 'n_calibration', 'per_impression', 'status', 'miscalibration_per_impression',
                                           'miscalibration_status'}
            assert all(res[name] == old[name] or (np.isnan(res[name]) and np.isnan(old[name])) for name in old)
            quota = serving.topic_quota(dev.corpus, setting.get('max_per_topic'), 'category')
            cal = serving.calibration(K, setting.get('calibrate_lambda'), setting.get('calibrate_by', 'category'),
                                      setting.get('calibrate_alpha', ALPHA), None, None, setting.get('shortlist'))
            cal = serving.bind_calibration(cal, dev.corpus, dev.hist_index, 'cuda')
            hk = None if cal is None else serving.history_keys(cal.topic_of_news, dev.hist_index[torch.from_numpy(first).long().cuda()],
                                                               torch.from_numpy(mask).cuda())
            positions, _ = serving.select_segments(scores, torch.from_numpy(offsets.astype(np.int64)).cuda(), None, quota, None, cand, K, cal=cal,
                                                   hist_keys=hk)
            want_v, want_s = recommend.slate_miscalibration(positions.cpu().numpy(), K, offsets, cand.cpu().numpy(), keys, n_keys,
                                                            hist_keys_of(keys, hist, mask), None, a32)
            assert np.array_equal(res['miscalibration_status'].cpu().numpy(), want_s)
            bound = metric_bound(hist.shape[1], ALPHA)
            assert np.abs(res['miscalibration_per_impression'].cpu().numpy() - want_v).max() <= bound
            counted = (want_s == 0) & (skip == 0)
            assert res['n_calibration'] == int(counted.sum()) > 20
            assert abs(res['miscalibration'] - want_v[counted].mean()) <= bound + len(labels) * 2.0 ** -53 * max(1.0, want_v.max())
            print('%s %s: miscalibration %.6f over %d' % (calibration, setting, res['miscalibration'], res['n_calibration']))
        assert results[1]['miscalibration'] <= results[0]['miscalibration'] or calibration != 'category'


def test_calibration_lowers_the_miscalibration_where_one_group_dominates_the_scores():
    """Scores that are the category's rank plus a little noise: the plain slate is the top categories' news; the calibrated one follows
    the impression's history."""
    model, dev, indices, labels = split()
    cache = model.build_news_cache(dev.corpus)
    rng = np.random.default_rng(9)
    cat = dev.corpus.news_category[dev.cand_index.reshape(-1).long()].cpu().numpy()
    scores = torch.from_numpy((cat + 0.1 * rng.random(cat.shape[0])).astype(np.float32)).cuda()
    plain, cal = Ut.sweep_slate_settings(model, dev, cache, scores, indices, labels, [{}, {'calibrate_lambda': 0.05}], K, calibration='category')
    print('one group dominates: miscalibration plain %.4f calibrated %.4f; nDCG %.4f / %.4f' % (plain['miscalibration'], cal['miscalibration'],
                                                                                                 plain['ndcg'], cal['ndcg']))
    assert plain['n_calibration'] == cal['n_calibration'] > 20 and cal['miscalibration'] < plain['miscalibration']


def test_the_entry_passes_calibration_through():
    corpus, model, indices, labels = dev_split('naml_att', seed=71)
    dev = DeviceBehaviors.from_devtest(DeviceCorpus(corpus), corpus, 'dev')
    metrics, results = model.evaluate_slates(dev, indices, labels, [{}, {'calibrate_lambda': 0.1}], k=K, rows_per_forward=6, calibration='category')
    plain_metrics, plain = Ut.evaluate_slates_on_device(model, dev, indices, labels, [{}], k=K, rows_per_forward=6)
    assert metrics == plain_metrics and 'miscalibration' not in plain[0]
    assert all(r['n_calibration'] > 20 and np.isfinite(r['miscalibration']) for r in results)
    assert all(results[0][name] == plain[0][name] or np.isnan(plain[0][name]) for name in plain[0])
