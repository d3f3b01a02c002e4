"""Model.explain_lists / Model.explain on the MI355X: tests/test_recommend_gpu.py's set-up (tiny models, synthetic weights, a synthetic
corpus of 60 news, five topics over four categories, a pool of 37 news) with three users -- a full history, a 2-slot one and an empty
one -- whose lists are the whole pool, its first nine news and five more.

  * ``score`` is ``score_lists``' on the same call: bit for bit under the CROWN user encoder, helpers.rel_err <= 1e-3 under ATT / MHSA
    (the pool's sum runs in another order), an exact zero staying an exact zero;
  * the dense terms keep the kernel test's two sum bounds (H = 6: one history tile, T = 1, u = 2^-24):
        |sum_h attention - 1| <= 7 u            |sum_h contribution - score| <= 12 u sum_h |contribution|
    and slots / values are the host selection (``recommend.top_slots``) of those terms under the user's history mask;
  * the reader without a history gets slots -1 everywhere and finite scores; several passes; ``Model.explain`` on ``recommend``'s
    positions carries ``recommend``'s score bits, under a topic quota too, and -1 positions come back as -inf / -1;
  * one check that does not go through the library's user side: for the CROWN user encoder the attention and the per-slot terms are
    recomputed in fp64 from oracle/lime_oracle.py's user-side pieces (``topic_representation``, ``candidate_aware_attention``,
    ``graph_sage`` and the K / Q products of ``kq_attention``, which returns the pooled vector and not its weights) on the model's state
    dict and the cached history / candidate rows."""
import math

import numpy as np
import pytest
import torch

from lime_cikm25_amd import DeviceCorpus, Model, make_config, recommend, synth
from lime_cikm25_amd import model as model_module
from helpers import rel_err
from user_cases import _TINY

pytestmark = pytest.mark.gpu

TOL = 1e-3
U, C, N_NEWS, K = 3, 37, 60, 10
TOPICS = [(1, 3), (1, 7), (2, 5), (4, 9), (5, 2)]
LISTS = [np.arange(C), np.arange(9), np.arange(10, 15)]                   # pool positions of every user's list
LENS = [len(l) for l in LISTS]
P = sum(LENS)
U24 = 2.0 ** -24

# name -> (config edits, LIME_OCCURRENCE_MATCH, by)
CASES = {
    'crown_user': (dict(content_encoder='CROWN'), False, 'contribution'),
    'att_user': (dict(content_encoder='CROWN', user_encoder='ATT'), False, 'contribution'),
    'mhsa_user': (dict(content_encoder='CROWN', user_encoder='MHSA'), False, 'contribution'),
    'add': (dict(content_encoder='CROWN', fusion_method='add'), False, 'contribution'),
    'add_occurrence': (dict(content_encoder='CROWN', fusion_method='add'), True, 'contribution'),
    'attention_off': (dict(content_encoder='CROWN', use_candidate_ware_clicked_news_attention=False), False, 'contribution'),
    'naml_att': (dict(news_encoder='NAML', user_encoder='ATT'), False, 'contribution'),            # a baseline: indexed tables
    'mlp': (dict(content_encoder='CROWN', click_predictor='mlp'), False, 'attention'),
}
_BUILT = {}


def build(name):
    """(model, the users' arguments, the pool's, the lists', n_src, histories, masks) -- once per configuration."""
    edits = CASES[name][0]
    key = tuple(sorted(edits.items()))
    if key in _BUILT:
        return _BUILT[key]
    assert torch.cuda.is_available(), 'these tests need the GPU'
    cfg = make_config(**{**_TINY, **edits})
    H = cfg.max_history_num
    corpus = synth.synth_corpus(cfg, n_news=N_NEWS, n_train=1, n_dev=1, seed=41)
    rng = np.random.default_rng(42)
    topic_of = rng.integers(0, len(TOPICS), size=N_NEWS)
    pool = rng.permutation(np.arange(1, N_NEWS))[:C].astype(np.int32)
    topic_of[pool] = rng.integers(0, len(TOPICS) - 1, size=C)
    topic_of[pool[5]] = len(TOPICS) - 1
    corpus.news_category[1:] = np.array([TOPICS[t][0] for t in topic_of[1:]], dtype=np.int32)
    corpus.news_subCategory[1:] = np.array([TOPICS[t][1] for t in topic_of[1:]], dtype=np.int32)
    dc = DeviceCorpus(corpus)
    n_hist = [H, 2, 0]
    hist = np.zeros((U, H), dtype=np.int32)
    outside = np.setdiff1d(np.arange(1, N_NEWS), pool)
    hist[0] = np.concatenate([pool[:3], rng.choice(outside, size=H - 3)])
    hist[1, :2] = [pool[4], outside[0]]
    mask = np.arange(H)[None, :] < np.array(n_hist)[:, None]
    ufr = np.where(mask, np.exp(rng.uniform(np.log(60.0), np.log(30 * 86400.0), size=(U, H))), 0.0).astype(np.float32)
    ult = np.where(mask, np.exp(rng.uniform(np.log(600.0), np.log(14 * 86400.0), size=(U, H))), 0.0).astype(np.float32)
    cfr = np.exp(rng.uniform(np.log(60.0), np.log(3 * 86400.0), size=C)).astype(np.float32)
    delta = rng.uniform(-8.0, 8.0, size=(U, C))
    delta[:, 0::6] = -5000.0                                               # a third of the pairs saturate the weight either way
    delta[:, 1::6] = 5000.0
    clt = (cfr[None, :].astype(np.float64) + delta).astype(np.float32)
    torch.manual_seed(0)
    model = Model(cfg)
    model.initialize()
    synth.fill_state_dict(model, seed=43)
    model = model.cuda().eval()
    cache = model.build_news_cache(dc)
    t = lambda a: torch.from_numpy(a).cuda()
    users = dict(news_cache=cache, corpus=dc, hist_index=t(hist), hist_mask=t(mask), user_freshness=t(ufr), user_lifetime=t(ult))
    pool_args = dict(users, cand_index=t(pool), cand_freshness=t(cfr), cand_lifetime=t(clt))
    list_args = dict(users, cand_offsets=t(np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)),
                     cand_index=t(np.concatenate([pool[l] for l in LISTS])), cand_freshness=t(np.concatenate([cfr[l] for l in LISTS])),
                     cand_lifetime=t(np.concatenate([clt[u, l] for u, l in enumerate(LISTS)])))
    n_src = min(P, H + cfg.batch_size)
    assert n_src == min(U * C, H + cfg.batch_size)
    _BUILT[key] = (model, pool_args, list_args, n_src, hist, mask)
    return _BUILT[key]


@pytest.fixture
def case(request, monkeypatch):
    name = request.param
    monkeypatch.setattr(model_module, 'OCCURRENCE_MATCH', CASES[name][1])
    return (name, CASES[name][2]) + build(name)


USER_OF = np.repeat(np.arange(U), LENS)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_record(a, b):
    for name, x, y in zip(a._fields, a, b):
        assert (x is None) == (y is None), name
        if x is not None:
            assert torch.equal(bits(x), bits(y)), name


@pytest.mark.parametrize('case', list(CASES), indirect=True)
def test_explain_lists_scores_what_score_lists_scores_and_its_terms_add_up(case):
    name, by, model, _, args, n_src, hist, mask = case
    H = hist.shape[1]
    ex = model.explain_lists(**args, top=3, by=by, dense=True, n_src=n_src)
    want = model.score_lists(**args, n_src=n_src)
    assert ex.score.shape == ex.base.shape == ex.weight.shape == (P,) and ex.slots.shape == ex.values.shape == (P, 3)
    assert ex.slots.dtype == torch.int32 and ex.attention.shape == (P, H) and torch.isfinite(ex.score).all()
    crown = model.config.user_encoder == 'CROWN'
    if crown:
        assert torch.equal(bits(ex.score), bits(want))
    else:
        e = rel_err(ex.score.cpu().numpy(), want.cpu().numpy())
        print('%s: explain_lists vs score_lists rel err %.2e' % (name, e))
        assert e <= TOL
    if name != 'mlp':                                                      # (the MLP predictor has no lifetime weight and no exact zero)
        zeros = want == 0
        assert int(zeros.sum()) > 0 or model.plain
        assert (ex.score[zeros] == 0).all(), 'an exact zero of score_lists must be an exact zero here'
    attn = ex.attention.cpu().numpy().astype(np.float64)
    one = np.abs(attn.sum(axis=1) - 1.0).max()
    print('%s: |sum attention - 1| max %.3e (bound %.3e)' % (name, one, 7 * U24))
    assert one <= 7 * U24 and (attn >= 0).all()
    eligible = mask[USER_OF]
    if name == 'mlp':
        assert ex.contribution is None and (ex.weight == 1).all() and torch.equal(bits(ex.base), bits(ex.score))
        values = ex.attention.cpu().numpy()
    else:
        assert ex.contribution.shape == (P, H)
        values = ex.contribution.cpu().numpy()
        c = values.astype(np.float64)
        gap, room = np.abs(c.sum(axis=1) - ex.score.cpu().numpy().astype(np.float64)), 12 * U24 * np.abs(c).sum(axis=1)
        print('%s: |sum contribution - score| / bound max %.3f' % (name, float((gap / np.maximum(room, 1e-300)).max())))
        assert (gap <= room).all()
        score, base, weight = (x.cpu().numpy().astype(np.float64) for x in (ex.score, ex.base, ex.weight))
        assert np.array_equal((base * weight).astype(np.float32), ex.score.cpu().numpy())          # score = fl(base weight)
    slot, top = recommend.top_slots(values, eligible, 3)
    assert np.array_equal(ex.slots.cpu().numpy(), slot) and np.array_equal(ex.values.cpu().numpy().view(np.int32), top.view(np.int32))
    got = ex.slots.cpu().numpy()
    assert (got[USER_OF == 0] >= 0).all()                                  # a full history: three slots named
    assert (got[USER_OF == 1][:, :2] >= 0).all() and (got[USER_OF == 1][:, :2] < 2).all() and (got[USER_OF == 1][:, 2] == -1).all()
    assert (got[USER_OF == 2] == -1).all() and (ex.values[torch.from_numpy(USER_OF == 2).cuda()] == 0).all()     # no history: no slot
    # without the dense terms nothing else moves; 'attention' ranks by the weights alone
    same_record(model.explain_lists(**args, top=3, by=by, n_src=n_src), ex._replace(attention=None, contribution=None))
    by_attention = model.explain_lists(**args, top=2, by='attention', dense=True, n_src=n_src)
    slot, top = recommend.top_slots(by_attention.attention.cpu().numpy(), eligible, 2)
    assert np.array_equal(by_attention.slots.cpu().numpy(), slot) and torch.equal(bits(by_attention.score), bits(ex.score))


@pytest.mark.parametrize('case', ['crown_user', 'att_user', 'add_occurrence', 'naml_att'], indirect=True)
def test_several_passes_give_the_same_record(case):
    name, by, model, _, args, n_src, *_ = case
    one = model.explain_lists(**args, top=3, by=by, dense=True, n_src=n_src)
    many = model.explain_lists(**args, top=3, by=by, dense=True, n_src=n_src, pairs_per_pass=1)        # one user a pass, re-planned
    same_record(many, model.explain_lists(**args, top=3, by=by, dense=True, n_src=n_src, pairs_per_pass=1))
    if model.config.user_encoder == 'CROWN':
        assert torch.equal(bits(many.score), bits(model.score_lists(**args, n_src=n_src, pairs_per_pass=1)))
    same_record(many, one)


@pytest.mark.parametrize('case', ['crown_user', 'mhsa_user', 'naml_att'], indirect=True)
def test_explain_carries_recommends_score_bits(case):
    name, by, model, pool_args, _, n_src, hist, mask = case
    crown = model.config.user_encoder == 'CROWN'
    for kw in (dict(), dict(max_per_topic=2)):
        pos, top = model.recommend(**pool_args, k=K, n_src=n_src, **kw)
        ex = model.explain(**pool_args, positions=pos, top=2, by=by, dense=True, n_src=n_src)
        assert ex.score.shape == (U, K) and ex.slots.shape == (U, K, 2) and ex.attention.shape == (U, K, hist.shape[1])
        filled = pos >= 0
        assert filled.all() or kw
        if crown:
            assert torch.equal(bits(ex.score), bits(top))
            assert torch.equal(bits(model.explain(**pool_args, positions=pos, top=2).score), bits(top))       # n_src defaults as in recommend
        else:
            assert rel_err(ex.score[filled].cpu().numpy(), top[filled].cpu().numpy()) <= TOL
        assert (ex.slots[2] == -1).all() and (ex.slots[0][filled[0]] >= 0).all()
    # unfilled entries: the whole pool without the history's news leaves -1 behind the last one
    pos, top = model.recommend(**pool_args, k=C, n_src=n_src, exclude_history=True)
    assert (pos[0] == -1).sum() == 3 and (pos[2] >= 0).all()
    ex = model.explain(**pool_args, positions=pos, top=2, by=by, n_src=n_src)
    none = pos < 0
    assert torch.isneginf(ex.score[none]).all() and (ex.slots[none] == -1).all() and (ex.values[none] == 0).all()
    assert torch.isfinite(ex.score[~none]).all()
    if crown:
        assert torch.equal(bits(ex.score), bits(top))
    assert ex.attention is None and ex.contribution is None


def test_the_terms_agree_with_the_oracles_user_side():
    """The CROWN user encoder's attention and per-slot terms from oracle/lime_oracle.py in fp64.  ``kq_attention`` returns the pooled
    vector, not its weights, so its two products and its softmax are restated here on the oracle's ``graph_sage`` output; everything
    before them is the oracle's own function.  The history and candidate rows are the model's cached rows, widened."""
    from oracle import lime_oracle as O
    model, _, args, n_src, hist, mask = build('crown_user')
    cfg = model.config
    ex = model.explain_lists(**args, top=3, dense=True, n_src=n_src)
    sd = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    ne, ue = 'news_encoder.', 'user_encoder.'
    cache, dc = args['news_cache'], args['corpus']
    with torch.no_grad():
        hrows = model.news_encoder.encode_cached(cache, args['hist_index'], args['user_freshness'], args['user_lifetime'])
        crows = model.news_encoder.encode_cached(cache, args['cand_index'], args['cand_freshness'], args['cand_lifetime'])
    H, D = hist.shape[1], crows.shape[1]
    who = torch.from_numpy(USER_OF)
    hrows = hrows.view(U, H, D).double().cpu()[who]                        # one row per pair: its user's history
    crows = crows.double().cpu().view(P, 1, D)
    hidx, cidx = args['hist_index'].cpu().long()[who], args['cand_index'].cpu().long()
    cat, sub = dc.news_category.cpu(), dc.news_subCategory.cpu()
    cand_topic = O.topic_representation(sd, ne, cat[cidx].view(P, 1), sub[cidx].view(P, 1))
    hist_topic = O.topic_representation(sd, ne, cat[hidx], sub[hidx])
    refined, _ = O.candidate_aware_attention(sd, ue + 'candidate_aware_attn.', hrows, hist_topic, cand_topic,
                                             torch.from_numpy(mask)[who], residual=cfg.use_residual_connection)
    g = O.graph_sage(sd, ue + 'graph_sage.', refined, sd[ue + 'user_node_embedding'], n_src=n_src)
    Kp = g @ sd[ue + 'K.weight'].t()                                                                # userEncoders.py:161
    Q = crows @ sd[ue + 'Q.weight'].t() + sd[ue + 'Q.bias']                                         # :162
    a = torch.softmax(torch.einsum('bha,bna->bnh', Kp, Q) / math.sqrt(float(cfg.attention_dim)), dim=-1).squeeze(1)      # :163-164
    remaining = (args['cand_lifetime'] - args['cand_freshness']).double().cpu()
    w = recommend.lifetime_weight(remaining.numpy(), cfg.sigmoid_scaling_alpha, cfg.penalty_scaling_beta,
                                  cfg.use_remaining_lifetime_weighting, cfg.use_expired_penalty)
    terms = (a * torch.einsum('bhd,bnd->bnh', g, crows).squeeze(1)).numpy() * w[:, None]
    e_a, e_c = rel_err(ex.attention.cpu().numpy(), a.numpy()), rel_err(ex.contribution.cpu().numpy(), terms)
    e_s = rel_err(ex.score.cpu().numpy(), terms.sum(axis=1))
    print('crown_user vs the oracle: attention rel err %.2e, contribution %.2e, score %.2e' % (e_a, e_c, e_s))
    assert e_a <= TOL and e_c <= TOL and e_s <= TOL
