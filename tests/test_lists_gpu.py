"""Model.score_lists / Model.recommend_lists and the grouped dev pass on the MI355X against Model.score_behaviors -- the cached dev pass --
on a DeviceBehaviors that holds the P (user, candidate) rows written out, same ``n_src``: test_recommend_gpu.py's set-up (tiny models,
synthetic weights, a synthetic corpus of 60 news, five topics over four categories) with four users -- a full history that contains
some of its own candidates, a short one, an empty one, and a user whose list is empty -- and lists of 37, 9, 1 and 0 candidates: the
first covers all five topics (one of them with a single pair), the second one topic.  The bar is the project's fp32 parity bar,
helpers.rel_err <= 1e-3; the observed values are printed."""
import numpy as np
import pytest
import torch

from lime_cikm25_amd import DeviceBehaviors, DeviceCorpus, Model, make_config, recommend, synth, util
from helpers import rel_err
from user_cases import _TINY

pytestmark = pytest.mark.gpu

TOL = 1e-3
N_NEWS, K = 60, 10
LENS = [37, 9, 1, 0]
U, P = len(LENS), sum(LENS)
OFFSETS = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
TOPICS = [(1, 3), (1, 7), (2, 5), (4, 9), (5, 2)]

CASES = {
    'crown_user': dict(),
    'att_user': dict(user_encoder='ATT'),
    'mhsa_user': dict(user_encoder='MHSA'),
    'attention_off': dict(use_candidate_ware_clicked_news_attention=False),
    'att_attention_off': dict(user_encoder='ATT', use_candidate_ware_clicked_news_attention=False),
    'gated': dict(fusion_method='gated'),
    'residual_off': dict(use_residual_connection=False),
    'kcnn_content': dict(content_encoder='KCNN'),
    'fixed_lifetime': dict(lifetime_type='fixed'),
}
_BUILT = {}


def build(name):
    """(model, score_lists' arguments, score_behaviors' scores [P], n_src, histories, masks, candidates) -- once per case."""
    if name in _BUILT:
        return _BUILT[name]
    assert torch.cuda.is_available(), 'these tests need the GPU'
    cfg = make_config(**{**_TINY, 'content_encoder': 'CROWN', **CASES[name]})
    H = cfg.max_history_num
    corpus = synth.synth_corpus(cfg, n_news=N_NEWS, n_train=1, n_dev=1, seed=41)
    rng = np.random.default_rng(42)
    topic_of = rng.integers(0, len(TOPICS), size=N_NEWS)
    pool = rng.permutation(np.arange(1, N_NEWS))[:LENS[0]].astype(np.int32)
    topic_of[pool] = rng.integers(0, len(TOPICS) - 1, size=LENS[0])
    topic_of[pool[5]] = len(TOPICS) - 1                                   # ... the last topic is held by a single pair
    outside = np.setdiff1d(np.arange(1, N_NEWS), pool)
    second = rng.permutation(outside)[:LENS[1]].astype(np.int32)          # the second list: nine news of ONE topic
    topic_of[second] = 2
    topic_of[np.setdiff1d(outside, second)] = rng.integers(0, len(TOPICS) - 1, size=outside.size - LENS[1])
    corpus.news_category[1:] = np.array([TOPICS[t][0] for t in topic_of[1:]], dtype=np.int32)
    corpus.news_subCategory[1:] = np.array([TOPICS[t][1] for t in topic_of[1:]], dtype=np.int32)
    dc = DeviceCorpus(corpus)
    cands = np.concatenate([pool, second, pool[7:8]]).astype(np.int32)
    assert cands.size == P and set(topic_of[pool].tolist()) == set(range(len(TOPICS)))
    # four users: a full history (with three of its own candidates in it), a short one (with one), an empty one, and one more history
    n_hist = [H, 2, 0, 3]
    rest = np.setdiff1d(outside, second)
    hist = np.zeros((U, H), dtype=np.int32)
    hist[0] = np.concatenate([pool[:3], rng.choice(rest, size=H - 3)])
    hist[1, :2] = [second[4], rest[0]]
    hist[3, :3] = rest[1:4]
    mask = np.arange(H)[None, :] < np.array(n_hist)[:, None]
    ufr = np.where(mask, np.exp(rng.uniform(np.log(60.0), np.log(30 * 86400.0), size=(U, H))), 0.0).astype(np.float32)
    ult = np.where(mask, np.exp(rng.uniform(np.log(600.0), np.log(14 * 86400.0), size=(U, H))), 0.0).astype(np.float32)
    # candidates: a third of the pairs saturate the weight either way, the rest do not
    cfr = np.exp(rng.uniform(np.log(60.0), np.log(3 * 86400.0), size=P)).astype(np.float32)
    delta = rng.uniform(-8.0, 8.0, size=P)
    delta[0::6] = -5000.0
    delta[1::6] = 5000.0
    clt = (cfr.astype(np.float64) + delta).astype(np.float32)
    user = np.repeat(np.arange(U), LENS)
    beh = DeviceBehaviors(dc, user, hist[user], mask[user], ufr[user], ult[user], cands.reshape(P, 1), cfr.reshape(P, 1), clt.reshape(P, 1),
                          eval_shape=True)
    torch.manual_seed(0)
    model = Model(cfg)
    model.initialize()
    synth.fill_state_dict(model, seed=43)
    model = model.cuda().eval()
    cache = model.build_news_cache(dc)
    t = lambda a: torch.from_numpy(a).cuda()
    args = dict(news_cache=cache, corpus=dc, hist_index=t(hist), hist_mask=t(mask), user_freshness=t(ufr), user_lifetime=t(ult),
                cand_offsets=t(OFFSETS), cand_index=t(cands), cand_freshness=t(cfr), cand_lifetime=t(clt))
    n_src = min(P, H + cfg.batch_size)
    want = model.score_behaviors(beh, torch.arange(P, device='cuda'), cache, n_src=n_src)
    _BUILT[name] = (model, args, want, n_src, hist, mask, cands)
    return _BUILT[name]


@pytest.mark.parametrize('name', list(CASES))
def test_score_lists_equals_the_cached_pass(name):
    model, args, want, n_src, *_ = build(name)
    got = model.score_lists(**args, n_src=n_src)
    assert got.shape == (P,) and got.dtype == torch.float32 and torch.isfinite(got).all()
    e = rel_err(got.cpu().numpy(), want.cpu().numpy())
    zeros = want == 0
    print('%s: score_lists vs score_behaviors rel err %.2e over %d pairs (%d exact zeros, %d distinct scores)' % (
        name, e, P, int(zeros.sum()), want.unique().numel()))
    # conditions on the yardstick: the scores differ pair by pair, and the saturated weight gives exact zeros
    assert want.unique().numel() > P // 2 and int(zeros.sum()) > 0
    assert e <= TOL
    assert (got[zeros] == 0).all(), 'an exact zero of the cached pass must be an exact zero here'
    if model.config.user_encoder == 'CROWN':
        assert torch.equal(model.score_lists(**args), got)                # n_src defaults to min(P, H + batch_size)
    host = dict(args, cand_offsets=OFFSETS.tolist())                      # the offsets may live on the host
    assert torch.equal(model.score_lists(**host, n_src=n_src), got)


@pytest.mark.parametrize('name', ['crown_user', 'mhsa_user', 'attention_off'])
def test_lists_that_are_one_shared_pool_give_score_pools_scores(name):
    model, args, want, n_src, hist, mask, cands = build(name)
    C = LENS[0]
    fr, lt = args['cand_freshness'][:C], args['cand_lifetime'][:C]
    pool = model.score_pool(**{k: args[k] for k in ('news_cache', 'corpus', 'hist_index', 'hist_mask', 'user_freshness', 'user_lifetime')},
                            cand_index=args['cand_index'][:C], cand_freshness=fr, cand_lifetime=lt, n_src=n_src)
    lists = dict(args, cand_offsets=torch.arange(U + 1) * C, cand_index=args['cand_index'][:C].repeat(U), cand_freshness=fr.repeat(U),
                 cand_lifetime=lt.repeat(U))
    got = model.score_lists(**lists, n_src=n_src).view(U, C)
    e = rel_err(got.cpu().numpy(), pool.cpu().numpy())
    print('%s: score_lists vs score_pool on one shared pool rel err %.2e' % (name, e))
    assert e <= TOL


@pytest.mark.parametrize('name', ['crown_user', 'att_user'])
def test_one_user_per_pass_gives_the_same_scores(name):
    model, args, want, n_src, *_ = build(name)
    keys = recommend.topic_table(args['corpus'].news_category.cpu().numpy(), args['corpus'].news_subCategory.cpu().numpy(),
                                 'topic' if name == 'crown_user' else 'category')[0][args['cand_index'].cpu().numpy()]
    n_distinct = recommend.list_plan(keys, OFFSETS).n_distinct
    passes = recommend.list_passes(OFFSETS, n_distinct, model.config.max_history_num, 1)
    assert len(passes) == U and len({S for _, _, S in passes}) > 1                    # passes with different slot counts
    assert n_distinct.tolist() == ([5, 1, 1, 0] if name == 'crown_user' else [4, 1, 1, 0])
    one = model.score_lists(**args, n_src=n_src)
    many = model.score_lists(**args, n_src=n_src, pairs_per_pass=1)
    assert rel_err(many.cpu().numpy(), want.cpu().numpy()) <= TOL
    # a pair's match does not depend on the pass; the user side may take another kernel form with fewer rows (gate_ln_sage)
    e = rel_err(many.cpu().numpy(), one.cpu().numpy())
    print('%s: one user per pass vs one pass rel err %.2e' % (name, e))
    assert e <= TOL
    assert torch.equal(many, model.score_lists(**args, n_src=n_src, pairs_per_pass=1))
    assert torch.equal(one, model.score_lists(**args, n_src=n_src))


@pytest.mark.parametrize('name', ['crown_user', 'mhsa_user', 'attention_off'])
def test_recommend_lists_returns_the_best_k_of_the_cached_pass(name):
    model, args, want, n_src, *_ = build(name)
    from lime_cikm25_amd import ops
    pos, top = model.recommend_lists(**args, k=K, n_src=n_src)
    assert pos.shape == top.shape == (U, K) and pos.dtype == torch.int32
    scores = model.score_lists(**args, n_src=n_src)
    p2, t2 = ops.topk_segments(scores, args['cand_offsets'], K)
    assert torch.equal(p2, pos) and torch.equal(t2.view(torch.int32), top.view(torch.int32))
    want = want.cpu().numpy().astype(np.float64)
    tol = TOL * float(np.abs(want).mean())
    pos, top = pos.cpu().numpy(), top.cpu().numpy()
    for u in range(U):
        mine = want[OFFSETS[u]:OFFSETS[u + 1]]
        n = min(K, LENS[u])
        live = pos[u, :n]
        assert len(set(live.tolist())) == n and (live >= 0).all() and (live < LENS[u]).all()       # no position repeats
        assert (pos[u, n:] == -1).all() and np.isneginf(top[u, n:]).all()                        # k above the list's length pads
        if n:
            assert np.abs(top[u, :n] - mine[live]).max() <= tol                                   # the pass's scores at those positions
            assert (np.diff(top[u, :n]) <= 0).all()                                               # descending
            left_out = np.delete(mine, live)
            assert left_out.size == 0 or left_out.max() <= mine[live][-1] + tol                   # nothing left out beats the last one
    assert (pos[3] == -1).all() and np.isneginf(top[3]).all()                                     # the empty list


def test_exclude_history():
    model, args, want, n_src, hist, mask, cands = build('crown_user')
    scores = model.score_lists(**args, n_src=n_src, exclude_history=True).cpu().numpy()
    plain = model.score_lists(**args, n_src=n_src).cpu().numpy()
    pos, top = model.recommend_lists(**args, k=LENS[0], n_src=n_src, exclude_history=True)
    pos, top = pos.cpu().numpy(), top.cpu().numpy()
    for u in range(U):
        seen = set(hist[u][mask[u]].tolist())
        gone = np.array([int(n) in seen for n in cands[OFFSETS[u]:OFFSETS[u + 1]]], dtype=bool)
        assert gone.sum() == [3, 1, 0, 0][u]
        mine, was = scores[OFFSETS[u]:OFFSETS[u + 1]], plain[OFFSETS[u]:OFFSETS[u + 1]]
        assert np.isneginf(mine[gone]).all() and np.array_equal(mine[~gone].view(np.int32), was[~gone].view(np.int32))
        live = pos[u][pos[u] >= 0]
        assert len(live) == LENS[u] - gone.sum() and not gone[live].any() and len(set(live.tolist())) == len(live)
        assert (pos[u][len(live):] == -1).all() and np.isneginf(top[u][len(live):]).all()


def test_exclude_history_does_not_depend_on_the_passes():
    model, args, want, n_src, *_ = build('crown_user')
    one = model.recommend_lists(**args, k=LENS[0], n_src=n_src, exclude_history=True)
    many = model.recommend_lists(**args, k=LENS[0], n_src=n_src, exclude_history=True, pairs_per_pass=1)   # one user a pass, re-planned
    assert torch.equal(many[0], one[0]) and torch.equal(many[1], one[1])


def test_a_user_whose_whole_list_is_in_the_history():
    model, args, want, n_src, hist, mask, cands = build('crown_user')
    few = dict(args, cand_offsets=torch.tensor([0, 3, 3, 5, 5]), cand_index=args['cand_index'][:5], cand_freshness=args['cand_freshness'][:5],
               cand_lifetime=args['cand_lifetime'][:5])                   # user 0's history starts with its first three candidates
    pos, top = model.recommend_lists(**few, k=4, n_src=n_src, exclude_history=True)
    assert pos[0].tolist() == [-1] * 4 and torch.isneginf(top[0]).all()
    assert sorted(pos[2].tolist()) == [-1, -1, 0, 1] and pos[2, 2:].tolist() == [-1, -1]
    assert pos[1].tolist() == pos[3].tolist() == [-1] * 4


# ---- the dev pass ----------------------------------------------------------------------------------------------------------------------
IMP_LENS = [3, 5, 2, 4, 6, 2, 4, 3]             # 29 rows; with 6 rows a forward the 7th impression (rows 22 .. 25) straddles row 24
PER = 6


def dev_split(name, seed=51):
    cfg = make_config(**{**_TINY, 'content_encoder': 'CROWN', **CASES[name]})
    corpus = synth.synth_corpus(cfg, n_news=N_NEWS, n_train=1, n_dev=len(IMP_LENS), seed=seed)
    rng = np.random.default_rng(seed)
    beh, indices, labels = [], [], []
    for i, (b, n) in enumerate(zip(corpus.dev_behaviors, IMP_LENS)):
        for j, cand in enumerate(rng.permutation(np.arange(1, N_NEWS))[:n]):
            fresh = float(np.float32(np.exp(rng.uniform(np.log(60.0), np.log(3 * 86400.0)))))
            # (a remaining lifetime of a few seconds either way: no weight saturates, so no two scores of an impression tie at zero)
            beh.append([b[0], b[1], b[2], int(cand), i, fresh, fresh + float(rng.uniform(-8.0, 8.0)), b[7], b[8]])
            indices.append(i)
        labels.append([1] + [0] * (n - 1))
    corpus.dev_behaviors = beh
    torch.manual_seed(0)
    model = Model(cfg)
    model.initialize()
    synth.fill_state_dict(model, seed=43)
    return corpus, model.cuda().eval(), indices, labels


def no_near_ties(s0):
    """A condition on the yardstick's scores: inside an impression any two lie further apart than the bar lets the two of them move
    (helpers.rel_err judges a score by TOL times its own magnitude, or the mean magnitude where that is larger)."""
    floor = float(np.abs(s0[s0 != 0]).mean())
    room = TOL * np.maximum(np.abs(s0), floor)
    bounds = np.concatenate([[0], np.cumsum(IMP_LENS)])
    for a, b in zip(bounds[:-1], bounds[1:]):
        apart = np.abs(s0[a:b, None] - s0[None, a:b]) > room[a:b, None] + room[None, a:b]
        if not (apart | np.eye(b - a, dtype=bool)).all():
            return False
    return True


@pytest.mark.parametrize('name', ['crown_user', 'att_user'])
def test_the_grouped_dev_pass_equals_the_row_wise_one(name, tmp_path):
    # the split: the first seed whose ROW-WISE scores (the yardstick alone decides) have no near-ties inside an impression
    for seed in range(51, 61):
        corpus, model, indices, labels = dev_split(name, seed)
        dev = DeviceBehaviors.from_devtest(DeviceCorpus(corpus), corpus, 'dev')
        m0, s0 = util.evaluate_cached_on_device(model, dev, indices, labels, result_file=str(tmp_path / 'rows.txt'), rows_per_forward=PER,
                                                return_scores=True)
        s0 = s0.cpu().numpy()
        if no_near_ties(s0):
            break
    else:
        pytest.fail('no seed gives the yardstick scores without near-ties inside an impression')
    assert dev.num == sum(IMP_LENS) and dev.num % PER and indices[(dev.num // PER) * PER - 1] == indices[(dev.num // PER) * PER]
    m1, s1 = util.evaluate_cached_on_device(model, dev, indices, labels, result_file=str(tmp_path / 'lists.txt'), rows_per_forward=PER,
                                            return_scores=True, grouped=True)
    s1 = s1.cpu().numpy()
    e = rel_err(s1, s0)
    print('%s (split seed %d): grouped vs row-wise dev pass rel err %.2e; metrics %s vs %s (apart by %s)' % (
        name, seed, e, tuple(m1), tuple(m0), tuple(abs(a - b) for a, b in zip(m1, m0))))
    assert e <= TOL
    assert (tmp_path / 'lists.txt').read_text() == (tmp_path / 'rows.txt').read_text()
    # one pass many times over: the grouped pass with a tiny row budget
    _, s2 = util.evaluate_cached_on_device(model, dev, indices, labels, rows_per_forward=PER, rows_per_pass=1, return_scores=True, grouped=True)
    assert rel_err(s2.cpu().numpy(), s0) <= TOL


def test_an_impression_with_two_histories_is_refused():
    corpus, model, indices, labels = dev_split('crown_user')
    dev = DeviceBehaviors.from_devtest(DeviceCorpus(corpus), corpus, 'dev')
    dev.user_freshness[4, 0] += 1.0                                       # row 4: the second row of impression 1 (rows 3 .. 7)
    with pytest.raises(ValueError, match=r'impression 1\b.*row 4'):
        util.evaluate_cached_on_device(model, dev, indices, labels, rows_per_forward=PER, grouped=True)
    dev = DeviceBehaviors.from_devtest(DeviceCorpus(corpus), corpus, 'dev')
    dev.hist_index[28, 1] += 1                                            # the last row of the last impression (rows 26 .. 28)
    with pytest.raises(ValueError, match=r'impression 7\b'):
        util.evaluate_cached_on_device(model, dev, indices, labels, rows_per_forward=PER, grouped=True)


def test_trainer_passes_grouped_eval_on():
    import inspect
    from lime_cikm25_amd.trainer import Trainer
    assert inspect.signature(Trainer.__init__).parameters['grouped_eval'].default is False
    assert inspect.signature(util.evaluate_cached_on_device).parameters['grouped'].default is False
