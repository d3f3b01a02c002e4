"""Model.score_pool / Model.recommend on the MI355X against Model.score_behaviors -- the cached dev pass -- on a DeviceBehaviors that
holds the U x C (user, candidate) rows written out, same ``n_src``: tiny models, synthetic weights, a synthetic corpus of 60 news,
three users (one with an empty history) and a pool of 37 news over five topics (four categories), one topic with a single candidate.
The bar is the project's fp32 parity bar, helpers.rel_err <= 1e-3; the observed values are printed."""
import numpy as np
import pytest
import torch

from lime_cikm25_amd import DeviceBehaviors, DeviceCorpus, Model, make_config, synth
from helpers import rel_err
from user_cases import _TINY

pytestmark = pytest.mark.gpu

TOL = 1e-3
U, C, N_NEWS, K = 3, 37, 60, 10
TOPICS = [(1, 3), (1, 7), (2, 5), (4, 9), (5, 2)]

CASES = {
    'crown_user': dict(),
    'att_user': dict(user_encoder='ATT'),
    'mhsa_user': dict(user_encoder='MHSA'),
    'gated': dict(fusion_method='gated'),
    'add': dict(fusion_method='add'),
    'attention_off': dict(use_candidate_ware_clicked_news_attention=False),
    'att_attention_off': dict(user_encoder='ATT', use_candidate_ware_clicked_news_attention=False),
    'residual_off': dict(use_residual_connection=False),
    'kcnn_content': dict(content_encoder='KCNN'),
    'fixed_lifetime': dict(lifetime_type='fixed'),
}
_BUILT = {}


def build(name):
    """(model, news cache, corpus, the pool's arguments, DeviceBehaviors of the U C rows, score_behaviors' scores [U, C]) -- once per case."""
    if name in _BUILT:
        return _BUILT[name]
    assert torch.cuda.is_available(), 'these tests need the GPU'
    cfg = make_config(**{**_TINY, 'content_encoder': 'CROWN', **CASES[name]})
    H = cfg.max_history_num
    corpus = synth.synth_corpus(cfg, n_news=N_NEWS, n_train=1, n_dev=1, seed=41)
    rng = np.random.default_rng(42)
    topic_of = rng.integers(0, len(TOPICS), size=N_NEWS)
    pool = rng.permutation(np.arange(1, N_NEWS))[:C].astype(np.int32)
    topic_of[pool] = rng.integers(0, len(TOPICS) - 1, size=C)
    topic_of[pool[5]] = len(TOPICS) - 1                                   # ... the last topic has exactly one candidate
    corpus.news_category[1:] = np.array([TOPICS[t][0] for t in topic_of[1:]], dtype=np.int32)
    corpus.news_subCategory[1:] = np.array([TOPICS[t][1] for t in topic_of[1:]], dtype=np.int32)
    dc = DeviceCorpus(corpus)
    # three users: a full history (with pool news in it), a short one, an empty one
    n_hist = [H, 2, 0]
    hist = np.zeros((U, H), dtype=np.int32)
    outside = np.setdiff1d(np.arange(1, N_NEWS), pool)
    hist[0] = np.concatenate([pool[:3], rng.choice(outside, size=H - 3)])
    hist[1, :2] = [pool[4], outside[0]]
    mask = np.arange(H)[None, :] < np.array(n_hist)[:, None]
    ufr = np.where(mask, np.exp(rng.uniform(np.log(60.0), np.log(30 * 86400.0), size=(U, H))), 0.0).astype(np.float32)
    ult = np.where(mask, np.exp(rng.uniform(np.log(600.0), np.log(14 * 86400.0), size=(U, H))), 0.0).astype(np.float32)
    # candidates: freshness per news, lifetime per (user, news); a third of the pairs saturate the weight either way, the rest do not
    cfr = np.exp(rng.uniform(np.log(60.0), np.log(3 * 86400.0), size=C)).astype(np.float32)
    delta = rng.uniform(-8.0, 8.0, size=(U, C))
    delta[:, 0::6] = -5000.0
    delta[:, 1::6] = 5000.0
    clt = (cfr[None, :].astype(np.float64) + delta).astype(np.float32)
    beh = DeviceBehaviors(dc, np.repeat(np.arange(U), C), np.repeat(hist, C, axis=0), np.repeat(mask, C, axis=0), np.repeat(ufr, C, axis=0),
                          np.repeat(ult, C, axis=0), np.tile(pool, U).reshape(U * C, 1), np.tile(cfr, U).reshape(U * C, 1),
                          clt.reshape(U * C, 1), eval_shape=True)
    torch.manual_seed(0)
    model = Model(cfg)
    model.initialize()
    synth.fill_state_dict(model, seed=43)
    model = model.cuda().eval()
    cache = model.build_news_cache(dc)
    t = lambda a: torch.from_numpy(a).cuda()
    args = dict(news_cache=cache, corpus=dc, hist_index=t(hist), hist_mask=t(mask), user_freshness=t(ufr), user_lifetime=t(ult),
                cand_index=t(pool), cand_freshness=t(cfr), cand_lifetime=t(clt))
    n_src = min(U * C, H + cfg.batch_size)
    want = model.score_behaviors(beh, torch.arange(U * C, device='cuda'), cache, n_src=n_src).view(U, C)
    _BUILT[name] = (model, args, want, n_src, hist, mask, pool)
    return _BUILT[name]


@pytest.mark.parametrize('name', list(CASES))
def test_score_pool_equals_the_cached_pass(name):
    model, args, want, n_src, *_ = build(name)
    got = model.score_pool(**args, n_src=n_src)
    assert got.shape == (U, C) and got.dtype == torch.float32 and torch.isfinite(got).all()
    e = rel_err(got.cpu().numpy(), want.cpu().numpy())
    zeros = want == 0
    print('%s: score_pool vs score_behaviors rel err %.2e over %d pairs (%d exact zeros, %d distinct scores)' % (
        name, e, U * C, int(zeros.sum()), want.unique().numel()))
    assert e <= TOL
    assert int(zeros.sum()) > 0 and (got[zeros] == 0).all(), 'an exact zero of the cached pass must be an exact zero here'
    assert want.unique().numel() > U * C // 2                              # the pass is a yardstick: scores differ pair by pair
    if model.config.user_encoder == 'CROWN':
        default = model.score_pool(**args)                                 # n_src defaults to min(U C, H + batch_size)
        assert torch.equal(default, got)


@pytest.mark.parametrize('name', ['crown_user', 'att_user'])
def test_several_passes_give_the_same_scores(name):
    model, args, want, n_src, *_ = build(name)
    one = model.score_pool(**args, n_src=n_src)
    many = model.score_pool(**args, n_src=n_src, pairs_per_pass=40)        # 40 rows hold one user's 37 candidates: three passes
    assert rel_err(many.cpu().numpy(), want.cpu().numpy()) <= TOL
    # a pair's match does not depend on the pass; the user side may take another kernel form with fewer rows (gate_ln_sage)
    assert rel_err(many.cpu().numpy(), one.cpu().numpy()) <= TOL
    assert torch.equal(many, model.score_pool(**args, n_src=n_src, pairs_per_pass=40))


def test_candidate_freshness_per_user_and_lifetime_per_news_broadcast():
    model, args, want, n_src, *_ = build('crown_user')
    wide = dict(args, cand_freshness=args['cand_freshness'].unsqueeze(0).expand(U, C).contiguous())
    assert torch.equal(model.score_pool(**wide, n_src=n_src), model.score_pool(**args, n_src=n_src))
    narrow = dict(args, cand_lifetime=args['cand_lifetime'][1])
    both = dict(args, cand_lifetime=args['cand_lifetime'][1].unsqueeze(0).expand(U, C).contiguous())
    assert torch.equal(model.score_pool(**narrow, n_src=n_src), model.score_pool(**both, n_src=n_src))


@pytest.mark.parametrize('name', ['crown_user', 'mhsa_user', 'attention_off'])
def test_recommend_returns_the_best_k_of_the_cached_pass(name):
    model, args, want, n_src, *_ = build(name)
    pos, top = model.recommend(**args, k=K, n_src=n_src)
    assert pos.shape == top.shape == (U, K) and pos.dtype == torch.int32
    want = want.cpu().numpy().astype(np.float64)
    tol = TOL * float(np.abs(want).mean())
    pos, top = pos.cpu().numpy(), top.cpu().numpy()
    for u in range(U):
        assert len(set(pos[u].tolist())) == K and pos[u].min() >= 0 and pos[u].max() < C        # no position repeats
        assert np.abs(top[u] - want[u, pos[u]]).max() <= tol                                      # the pass's scores at those positions
        assert (np.diff(top[u]) <= 0).all()                                                       # descending
        left_out = np.delete(want[u], pos[u])
        assert left_out.max() <= want[u, pos[u]][-1] + tol                                        # nothing left out beats the last one
    scores = model.score_pool(**args, n_src=n_src)
    from lime_cikm25_amd import ops
    p2, t2 = ops.topk_rows(scores, K)
    assert np.array_equal(p2.cpu().numpy(), pos) and np.array_equal(t2.cpu().numpy().view(np.int32), top.view(np.int32))
    again = model.recommend(**args, k=K, n_src=n_src)
    assert np.array_equal(again[0].cpu().numpy(), pos) and np.array_equal(again[1].cpu().numpy().view(np.int32), top.view(np.int32))


def test_exclude_history():
    model, args, want, n_src, hist, mask, pool = build('crown_user')
    pos, top = model.recommend(**args, k=C, n_src=n_src, exclude_history=True)
    scores = model.score_pool(**args, n_src=n_src, exclude_history=True)
    plain = model.score_pool(**args, n_src=n_src)
    pos, top = pos.cpu().numpy(), top.cpu().numpy()
    for u in range(U):
        seen = set(hist[u][mask[u]].tolist())
        gone = np.array([int(n) in seen for n in pool])
        assert gone.sum() == [3, 1, 0][u]
        live = pos[u][pos[u] >= 0]
        assert len(live) == C - gone.sum() and not gone[live].any() and len(set(live.tolist())) == len(live)
        assert (pos[u][len(live):] == -1).all() and np.isneginf(top[u][len(live):]).all()
        assert np.isneginf(scores[u].cpu().numpy()[gone]).all()
        assert torch.equal(scores[u][torch.from_numpy(~gone).cuda()], plain[u][torch.from_numpy(~gone).cuda()])


def test_exclude_history_does_not_depend_on_the_passes():
    model, args, want, n_src, *_ = build('crown_user')
    one = model.recommend(**args, k=C, n_src=n_src, exclude_history=True)
    many = model.recommend(**args, k=C, n_src=n_src, exclude_history=True, pairs_per_pass=40)          # one user a pass
    assert torch.equal(many[0], one[0]) and torch.equal(many[1], one[1])


def test_a_user_whose_whole_pool_is_in_the_history():
    model, args, want, n_src, hist, mask, pool = build('crown_user')
    H = hist.shape[1]
    few = dict(args, cand_index=args['cand_index'][:3], cand_freshness=args['cand_freshness'][:3], cand_lifetime=args['cand_lifetime'][:, :3])
    pos, top = model.recommend(**few, k=5, n_src=n_src, exclude_history=True)   # user 0's history starts with pool[:3]
    assert pos[0].tolist() == [-1] * 5 and torch.isneginf(top[0]).all()
    assert sorted(pos[2].tolist()) == [-1, -1, 0, 1, 2] and pos[2, 3:].tolist() == [-1, -1]
