"""The baseline models -- a content encoder as the news encoder itself, no LIME (config.news_encoder = 'CROWN', 'CNN', 'NAML', 'MHSA',
'KCNN'; reference model.py:41-62) -- on the MI355X: the forward and every stored tap against the reference goldens
(tests/golden/plain_*.npz, grad_plain_*.npz: tools/make_plain_goldens.py), the gradients, graph replay against eager, the encode-once
layout and the per-news cache against the plain eval forward, the serving paths (pool and lists, on lime_grouped_match_indexed_f32 and
on the gather form) against the cached pass, a reproducible training step and one epoch of the Trainer.  The bar is the project's
parity bound, helpers.rel_err < 1e-3; the observed values are printed.  The indexed kernel itself: tests/test_grouped_match_indexed_gpu.py."""
import json
import math
import os

import numpy as np
import pytest
import torch

import plain_cases
from helpers import GOLDEN_DIR, load_golden, rel_err, synth_state_dict
from test_naml_gpu import _with_history_fill, compare_grads, unique_named_parameters
from lime_cikm25_amd import DeviceBehaviors, DeviceCorpus, Model, formats, make_config, model as model_module, ops, synth, util
from lime_cikm25_amd.training import TrainStep, load_checkpoint, negative_log_softmax

pytestmark = pytest.mark.gpu
TOL = 1e-3                      # the project's parity bound against the reference, as tests/test_user_encoders_gpu.py
KTOL = 2e-5                     # fp32-level kernel against the same sums in another order, as tests/test_user_encoders_gpu.py
HIST_ROWS = 2                   # tools/make_plain_goldens.py stores history-level taps for the first rows only


def gpu_model(cfg, seed=plain_cases.WEIGHT_SEED):
    m = Model(cfg)
    m.initialize()
    synth.fill_state_dict(m, seed)
    return m.cuda()


def run(model, batch, eval_shape=False):
    model.eval()
    if not eval_shape:
        model.training = True
    with torch.no_grad():
        out = model(*[v.cuda() for v in batch.values()])
    torch.cuda.synchronize()
    return out.cpu()


def _stages(model, b):
    """The reference's module API on the scoring kernels: news_encoder(...), user_encoder(...), the candidate-aware weights and the
    refined history, the MHSA user encoder's taps."""
    ne, ue = model.news_encoder, model.user_encoder
    with torch.no_grad():
        cand = ne(b['news_title_text'], b['news_title_mask'], b['news_title_entity'], b['news_content_text'], b['news_content_mask'],
                  b['news_content_entity'], b['news_category'], b['news_subCategory'], None, b['news_freshness'],
                  b['news_user_topic_lifetime'])
        hist = ne(b['user_title_text'], b['user_title_mask'], b['user_title_entity'], b['user_content_text'], b['user_content_mask'],
                  b['user_content_entity'], b['user_category'], b['user_subCategory'], None, b['user_freshness'],
                  b['user_user_topic_lifetime'])
        user = ue(b['user_title_text'], b['user_title_mask'], b['user_title_entity'], b['user_content_text'], b['user_content_mask'],
                  b['user_content_entity'], b['news_category'], b['news_subCategory'], b['user_category'], b['user_subCategory'],
                  b['user_history_mask'], b['user_history_graph'], b['user_history_category_mask'],
                  b['user_history_category_indices'], None, cand, b['user_freshness'], b['user_user_topic_lifetime'])
        agg = ue.attention_weights(b['news_category'], b['news_subCategory'], b['user_category'], b['user_subCategory'], b['user_history_mask'])
        taps = {}
        kw = dict(remaining_lifetime=b['remaining_lifetime'].float(), weighting=model.remaining_lifetime_weighting)
        if model.config.user_encoder == 'CROWN':
            if agg is not None:
                taps['hist_refined'] = ue.candidate_aware_attn.refine(hist, agg)
        else:
            kw['taps'] = taps
        user2, logits = ue.match(hist, b['news_category'], b['news_subCategory'], b['user_category'], b['user_subCategory'],
                                 b['user_history_mask'], cand, **kw)
    assert torch.equal(user, user2)
    return cand, user, agg, taps, logits


@pytest.mark.parametrize('name', list(plain_cases.CASES))
def test_forward_matches_the_reference(name):
    cfg, batch, c = plain_cases.build_case(name)
    g = load_golden(name)
    model = gpu_model(cfg)
    logits = run(model, batch, c['eval_shape'])                 # eval cases: the [rows] signature (model.py:158-169)
    assert logits.shape == g['logits'].shape
    e = rel_err(logits.numpy(), g['logits'])
    print('%s: logits vs reference golden %.2e' % (name, e))
    assert e < TOL
    z = g['logits'] == 0                                        # saturated lifetime weight: exact +-0
    assert np.all(logits.numpy()[z] == 0) and np.array_equal(np.signbit(logits.numpy()[z]), np.signbit(g['logits'][z]))
    model.eval()
    b = {k: v.cuda() for k, v in batch.items()}
    if c['eval_shape']:
        for k in list(b):
            if k.startswith('news_') or k == 'remaining_lifetime':
                b[k] = b[k].unsqueeze(1)
    cand, user, agg, taps, logits2 = _stages(model, b)
    errs = {'logits (stages)': rel_err(logits2.cpu().numpy().reshape(g['logits'].shape), g['logits']),
            'news_representation': rel_err(cand.cpu().numpy(), g['news_representation'])}
    assert tuple(user.shape) == g['user_representation'].shape
    errs['user_representation'] = rel_err(user.cpu().numpy(), g['user_representation'])
    if cfg.use_candidate_ware_clicked_news_attention:
        errs['attn_weights_agg'] = rel_err(agg.cpu().numpy(), g['attn_weights_agg'])
        errs['hist_refined'] = rel_err(taps['hist_refined'][:HIST_ROWS].cpu().numpy(), g['hist_refined'])
    else:
        assert agg is None and 'attn_weights_agg' not in g and 'hist_refined' not in g
    if cfg.user_encoder == 'MHSA':
        errs['self_attention'] = rel_err(taps['self_attention'][:HIST_ROWS].cpu().numpy(), g['self_attention'])
        errs['post_affine'] = rel_err(taps['post_affine'][:HIST_ROWS].cpu().numpy(), g['post_affine'])
    else:
        assert 'self_attention' not in g
    print('%s: %s' % (name, ', '.join('%s %.2e' % kv for kv in errs.items())))
    assert max(errs.values()) < TOL, errs
    # every tap the golden stores was compared
    stored = set(g.keys()) - {'logits', 'state_dict_spec', 'trainable'}
    assert stored == set(errs) - {'logits (stages)'}, stored ^ set(errs)


@pytest.mark.parametrize('name', plain_cases.GRAD_CASES)
def test_gradients_match_the_reference(name):
    """Loss and every gradient the reference has within TOL by ``compare_grads``; every parameter it leaves at None has none -- the
    measure and the bound of tests/test_user_encoders_gpu.py::test_gradients_match_the_reference.  ``category_embedding`` is trainable
    here and gets its gradient from the news side and, under the candidate-aware attention, from the user side too."""
    g = load_golden('grad_' + name)
    cfg, batch, c = plain_cases.build_case(name)
    model = gpu_model(cfg)
    model.eval()
    model.training = True
    logits = model(*[v.cuda() for v in batch.values()])
    assert logits.requires_grad
    assert rel_err(logits.detach().cpu().numpy(), g['logits']) < TOL
    loss = negative_log_softmax(logits)
    assert abs(float(loss.detach()) - float(g['loss'])) < TOL * max(1.0, abs(float(g['loss'])))
    loss.backward()
    named = dict(unique_named_parameters(model))
    assert 'news_encoder.category_embedding.weight' in json.loads(str(g['with_grad']))
    for k in json.loads(str(g['without_grad'])):
        assert named[k].grad is None, '%s: the reference leaves this gradient at None' % k
    worst = compare_grads(g, named)
    print('%s: loss %.6f (reference %.6f), worst gradient %s rel err %.2e' % (name, float(loss.detach()), float(g['loss']), *worst))


@pytest.mark.parametrize('news,user', [('CROWN', 'CROWN'), ('NAML', 'ATT')])
def test_one_captured_graph_follows_the_padding_pattern(news, user):
    """Graph replay equals eager bitwise, and ONE captured graph serves batches with different padding patterns."""
    cfg = make_config(news_encoder=news, user_encoder=user, **plain_cases._CFG1)
    model = gpu_model(cfg, seed=61)
    H = cfg.max_history_num
    A = synth.make_batch(cfg, 8, 3, seed=62)
    batches = {'A': A, 'B': _with_history_fill(cfg, A, lambda b: H), 'C': _with_history_fill(cfg, A, lambda b: 1 if b % 4 == 0 else 0),
               'D': _with_history_fill(cfg, synth.make_batch(cfg, 8, 3, seed=63), lambda b: (7 * b) % (H + 1))}
    model.use_graph = True
    model._graphs.clear()
    got = {}
    for name in ('A', 'B', 'C', 'D', 'A'):
        got.setdefault(name, []).append(run(model, batches[name]))
    assert len(model._graphs) == 1
    assert torch.equal(got['A'][0], got['A'][1])
    model.use_graph = False
    for name in ('A', 'B', 'C', 'D'):
        want = run(model, batches[name])
        assert torch.isfinite(want).all() and torch.equal(got[name][0], want), name
    assert not torch.equal(got['A'][0], got['B'][0])


PAIRINGS = [('CROWN', 'CROWN'), ('NAML', 'ATT'), ('MHSA', 'MHSA')]


@pytest.mark.parametrize('news,user', PAIRINGS)
def test_score_impressions_equals_eval_forward_on_expanded_rows(news, user):
    """B impressions x K candidates with every history encoded once (hist_div = K) against the eval forward on the B * K expanded rows
    (not bitwise: the two layouts give the GEMMs other row counts -- the kernel-level bound).  Chunked passes are bitwise."""
    cfg = make_config(news_encoder=news, user_encoder=user, max_history_num=10, max_title_length=16, max_abstract_length=32,
                      batch_size=64, vocabulary_size=5000)
    model = gpu_model(cfg, seed=41)
    B, K = 5, 6
    batch = synth.make_batch(cfg, B, K, seed=42)
    c = {k: v.cuda() for k, v in batch.items()}
    model.eval()
    args = (c['user_category'], c['user_subCategory'], c['user_title_text'], c['user_title_mask'], c['user_content_text'],
            c['user_freshness'], c['user_user_topic_lifetime'], c['user_history_mask'], c['news_category'], c['news_subCategory'],
            c['news_title_text'], c['news_title_mask'], c['news_content_text'], c['news_freshness'], c['news_user_topic_lifetime'],
            c['remaining_lifetime'])
    got = model.score_impressions(*args)
    assert got.shape == (B, K)
    exp = type(batch)()
    for k, v in batch.items():
        exp[k] = v.reshape((B * K,) + tuple(v.shape[2:])) if (k.startswith('news_') or k == 'remaining_lifetime') else v.repeat_interleave(K, dim=0)
    model.use_graph = False
    ref_rows = run(model, exp, True)
    e = rel_err(got.cpu().reshape(-1).numpy(), ref_rows.reshape(-1).numpy())
    print('%s-%s: score_impressions vs expanded rows: %.2e' % (news, user, e))
    assert e < KTOL
    assert torch.equal(model.score_impressions(*args, rows_per_pass=2 * K), got)


def toy(news, user, batch_size=16, **kw):
    """The toy dataset of tests/golden/formats.json, as tests/test_user_encoders_gpu.py and tests/test_end_to_end_gpu.py use it."""
    g = json.load(open(os.path.join(GOLDEN_DIR, 'formats.json')))
    L = g['lines']
    cfg = make_config(news_encoder=news, user_encoder=user, max_history_num=g['max_history_num'], max_title_length=g['max_title_length'],
                      max_abstract_length=g['max_abstract_length'], vocabulary_size=len(g['word_dict']), negative_sample_num=2,
                      category_num=len(g['category_dict']) + 1, subCategory_num=len(g['subCategory_dict']) + 1,
                      user_num=len(g['user_ID_dict']), batch_size=batch_size, **kw)
    corpus = formats.build_corpus(cfg, [L['train_news'], L['dev_news'], L['test_news']],
                                  [L['train_behaviors'], L['dev_behaviors'], L['test_behaviors']], g['news_ID_dict'],
                                  g['user_ID_dict'], g['category_dict'], g['subCategory_dict'], g['word_dict'], dataset='adressa')
    torch.manual_seed(0)
    np.random.seed(0)
    model = Model(cfg)
    model.initialize()
    torch.nn.init.normal_(model.news_encoder.word_embedding.weight, std=0.1)
    return cfg, corpus, model.cuda(), formats.truth_labels(L['dev_behaviors'])


@pytest.mark.parametrize('news,user', PAIRINGS)
def test_the_cached_passes_agree_with_the_uncached_forward(news, user, tmp_path):
    """build_news_cache + score_behaviors against the uncached eval forward on the same rows and n_src; util.compute_scores_cached against
    util.compute_scores (the same rank file and metrics); evaluate_cached_on_device, row-wise and grouped, against the cached host pass."""
    cfg, corpus, model, labels = toy(news, user)
    dc = DeviceCorpus(corpus)
    dev = DeviceBehaviors.from_devtest(dc, corpus, 'dev')
    model.eval()
    cache = model.build_news_cache(dc)
    assert tuple(cache.shape) == (dc.news_title_text.shape[0], model.news_embedding_dim)       # a row is the news' representation
    rows = list(range(dev.num))
    model.use_graph = False
    with torch.no_grad():
        batch = dev.assemble(rows)
        plain = model(*batch, batch[24] - batch[23]).view(-1)           # remaining lifetime: util.py:98-106, lifetime_type 'user_topic'
    cached = model.score_behaviors(dev, rows, cache, n_src=dev.num)
    e = rel_err(cached.cpu().numpy(), plain.cpu().numpy())
    print('%s-%s: score_behaviors vs the uncached eval forward %.2e over %d rows' % (news, user, e, dev.num))
    assert e < KTOL and plain.unique().numel() > dev.num // 2
    # encode_cached is a row gather
    idx = dev.cand_index[:7]
    assert torch.equal(model.news_encoder.encode_cached(cache, idx, dev.cand_freshness[:7], dev.cand_lifetime[:7]), cache[idx.reshape(-1).long()])
    model.use_graph = True
    truth = formats.write_truth_file(str(tmp_path / 'truth.txt'), labels)
    per = max(dev.num, 64) if user != 'CROWN' else dev.num
    a = util.compute_scores(model, [dev.assemble(rows)], corpus.dev_indices, str(tmp_path / 'rank.txt'), truth)
    b = util.compute_scores_cached(model, dev, corpus.dev_indices, str(tmp_path / 'rank_cached.txt'), truth, rows_per_forward=per)
    assert open(tmp_path / 'rank_cached.txt').read() == open(tmp_path / 'rank.txt').read()
    assert a == b
    for grouped in (False, True):
        m = util.evaluate_cached_on_device(model, dev, corpus.dev_indices, labels, result_file=str(tmp_path / ('device_%d.txt' % grouped)),
                                           rows_per_forward=per, grouped=grouped)
        assert open(tmp_path / ('device_%d.txt' % grouped)).read() == open(tmp_path / 'rank_cached.txt').read(), grouped
        assert np.allclose(m, b, rtol=0, atol=1e-12), (grouped, m, b)


# ---- serving: a pool of 70 news over five topics, one of which holds 65 of a user's pairs (the 64-pair tile and one more) -------------
U, C, N_NEWS, K = 3, 70, 90, 4
TOPICS = [(1, 3), (1, 7), (2, 5), (4, 9), (5, 2)]
LENS = [0, 1, 9]
SERVING = {
    'crown_crown': dict(news_encoder='CROWN', user_encoder='CROWN'),
    'crown_att': dict(news_encoder='CROWN', user_encoder='ATT'),
    'mhsa_mhsa': dict(news_encoder='MHSA', user_encoder='MHSA'),
    'mhsa_mhsa_attention_off': dict(news_encoder='MHSA', user_encoder='MHSA', use_candidate_ware_clicked_news_attention=False),
}
_BUILT = {}


def serving(name):
    if name in _BUILT:
        return _BUILT[name]
    cfg = make_config(**{**plain_cases._TINY, **SERVING[name]})
    H = cfg.max_history_num
    corpus = synth.synth_corpus(cfg, n_news=N_NEWS, n_train=1, n_dev=1, seed=41)
    rng = np.random.default_rng(42)
    pool = rng.permutation(np.arange(1, N_NEWS))[:C].astype(np.int32)
    topic_of = rng.integers(0, len(TOPICS), size=N_NEWS)
    topic_of[pool] = 0                                                     # 65 of the pool's 70 news in ONE topic ...
    topic_of[pool[[3, 17, 31, 45, 59]]] = [1, 2, 3, 4, 1]                  # ... the others over the remaining four
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
    model = Model(cfg)
    model.initialize()
    synth.fill_state_dict(model, seed=43)
    model = model.cuda().eval()
    cache = model.build_news_cache(dc)
    t = lambda a: torch.from_numpy(a).cuda()
    users = dict(news_cache=cache, corpus=dc, hist_index=t(hist), hist_mask=t(mask), user_freshness=t(ufr), user_lifetime=t(ult))
    # the pool: every user against all C; the yardstick is the cached dev pass over the U C rows written out
    beh = DeviceBehaviors(dc, np.repeat(np.arange(U), C), np.repeat(hist, C, axis=0), np.repeat(mask, C, axis=0), np.repeat(ufr, C, axis=0),
                          np.repeat(ult, C, axis=0), np.tile(pool, U).reshape(U * C, 1), np.tile(cfr, U).reshape(U * C, 1),
                          clt.reshape(U * C, 1), eval_shape=True)
    n_src = min(U * C, H + cfg.batch_size)
    pool_args = dict(users, cand_index=t(pool), cand_freshness=t(cfr), cand_lifetime=t(clt))
    pool_want = model.score_behaviors(beh, torch.arange(U * C, device='cuda'), cache, n_src=n_src).view(U, C)
    # the lists: 0, 1 and 9 candidates (the nine span four topics, two of them with a saturated weight)
    P = sum(LENS)
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    nine = np.array([0, 1, 2, 3, 17, 31, 6, 7, 8])
    lidx = np.concatenate([pool[20:21], pool[nine]]).astype(np.int32)
    lfr = np.concatenate([cfr[20:21], cfr[nine]])
    llt = np.concatenate([clt[1, 20:21], clt[2, nine]])
    user = np.repeat(np.arange(U), LENS)
    lbeh = DeviceBehaviors(dc, user, hist[user], mask[user], ufr[user], ult[user], lidx.reshape(P, 1), lfr.reshape(P, 1), llt.reshape(P, 1),
                           eval_shape=True)
    n_src_l = min(P, H + cfg.batch_size)
    list_args = dict(users, cand_offsets=t(off), cand_index=t(lidx), cand_freshness=t(lfr), cand_lifetime=t(llt))
    list_want = model.score_behaviors(lbeh, torch.arange(P, device='cuda'), cache, n_src=n_src_l)
    _BUILT[name] = (model, pool_args, pool_want, n_src, list_args, list_want, n_src_l, off)
    return _BUILT[name]


@pytest.fixture(params=[True, False], ids=['indexed', 'gather'])
def indexed(request, monkeypatch):
    """The grouped match on lime_grouped_match_indexed_f32 (the default) and on materialised rows (LIME_INDEXED_MATCH=0)."""
    monkeypatch.setattr(model_module, 'INDEXED_MATCH', request.param)
    return request.param


def _count_indexed(monkeypatch):
    calls = []
    real = ops.grouped_match
    monkeypatch.setattr(ops, 'grouped_match', lambda *a, **kw: (calls.append(kw.get('index') is not None), real(*a, **kw))[1])
    return calls


def topk_positions(scores, k):
    """The stated tie rule on given scores: descending, equal scores (+0.0 == -0.0) lower position first; -1 behind the last."""
    s = np.asarray(scores, dtype=np.float64) + 0.0
    order = sorted(range(len(s)), key=lambda i: (-s[i], i))[:k]
    return order + [-1] * (k - len(order))


@pytest.mark.parametrize('name', list(SERVING))
def test_score_pool_and_recommend_equal_the_cached_pass(name, indexed, monkeypatch):
    model, args, want, n_src, *_ = serving(name)
    calls = _count_indexed(monkeypatch)
    got = model.score_pool(**args, n_src=n_src)
    assert calls and all(c == indexed for c in calls)                      # the form asked for is the form that ran
    assert got.shape == (U, C) and torch.isfinite(got).all()
    e = rel_err(got.cpu().numpy(), want.cpu().numpy())
    zeros = want == 0
    print('%s (%s): score_pool vs score_behaviors rel err %.2e over %d pairs (%d exact zeros, %d distinct scores)' % (
        name, 'indexed' if indexed else 'gather', e, U * C, int(zeros.sum()), want.unique().numel()))
    assert e <= TOL
    assert int(zeros.sum()) > 0 and (got[zeros] == 0).all(), 'an exact zero of the cached pass must be an exact zero here'
    assert want.unique().numel() > U * C // 2
    many = model.score_pool(**args, n_src=n_src, pairs_per_pass=1)         # one user a pass
    assert rel_err(many.cpu().numpy(), want.cpu().numpy()) <= TOL
    pos, top = model.recommend(**args, k=K, n_src=n_src)
    for u in range(U):
        assert pos[u].tolist() == topk_positions(got[u].cpu().numpy(), K)
        assert torch.equal(top[u], got[u][pos[u].long()])
    # exclusion: a candidate in a masked-in slot of the history is never returned
    pos_x, top_x = model.recommend(**args, k=K, n_src=n_src, exclude_history=True)
    hist, mask, pool = args['hist_index'].cpu().numpy(), args['hist_mask'].cpu().numpy(), args['cand_index'].cpu().numpy()
    for u in range(U):
        seen = set(hist[u][mask[u]].tolist())
        s = got[u].cpu().numpy().copy()
        s[[int(n) in seen for n in pool]] = -np.inf
        assert pos_x[u].tolist() == topk_positions(s, K) and not {int(pool[p]) for p in pos_x[u].tolist()} & seen


@pytest.mark.parametrize('name', list(SERVING))
def test_score_lists_and_recommend_lists_equal_the_cached_pass(name, indexed, monkeypatch):
    model, _, _, _, args, want, n_src, off = serving(name)
    calls = _count_indexed(monkeypatch)
    got = model.score_lists(**args, n_src=n_src)
    assert calls and all(c == indexed for c in calls)
    assert got.shape == (sum(LENS),) and torch.isfinite(got).all()
    e = rel_err(got.cpu().numpy(), want.cpu().numpy())
    zeros = want == 0
    print('%s (%s): score_lists vs score_behaviors rel err %.2e over %d pairs (%d exact zeros)' % (
        name, 'indexed' if indexed else 'gather', e, sum(LENS), int(zeros.sum())))
    assert e <= TOL
    assert int(zeros.sum()) > 0 and (got[zeros] == 0).all()
    pos, top = model.recommend_lists(**args, k=K, n_src=n_src)
    assert pos.shape == (U, K)
    for u in range(U):
        s = got[off[u]:off[u + 1]].cpu().numpy()
        assert pos[u].tolist() == topk_positions(s, K)
        live = pos[u][pos[u] >= 0].long()
        assert torch.equal(top[u][:live.numel()], got[off[u]:off[u + 1]][live]) and torch.isneginf(top[u][live.numel():]).all()


def test_the_two_forms_of_the_match_agree_pair_by_pair(monkeypatch):
    """ATT / MHSA: no Q GEMM stands between the two forms, so the indexed match gives the gather form's bits."""
    model, args, _, n_src, largs, _, n_src_l, _ = serving('mhsa_mhsa')
    out = {}
    for form in (True, False):
        monkeypatch.setattr(model_module, 'INDEXED_MATCH', form)
        out[form] = (model.score_pool(**args, n_src=n_src), model.score_lists(**largs, n_src=n_src_l))
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])


def test_lime_models_keep_the_gather_form(monkeypatch):
    """A LIME model's candidate rows depend on the occurrence: it never takes the indexed form."""
    from test_recommend_gpu import build
    model, args, want, n_src, *_ = build('crown_user')
    calls = _count_indexed(monkeypatch)
    got = model.score_pool(**args, n_src=n_src)
    assert calls and not any(calls)
    assert rel_err(got.cpu().numpy(), want.cpu().numpy()) <= TOL


def test_serving_refusals_keep_their_order():
    model, args, *_ = serving('crown_crown')
    with pytest.raises(ValueError, match='news_cache must be'):
        model.score_pool(**dict(args, news_cache=args['news_cache'][:, :0]))
    with pytest.raises(ValueError, match='1 <= k <= 128'):
        model.recommend(**args, k=129)
    with pytest.raises(ValueError, match='pairs_per_pass'):
        model.score_pool(**args, pairs_per_pass=0)


@pytest.mark.parametrize('name', ['plain_crown_crown', 'plain_naml_att'])
@pytest.mark.parametrize('dropout', [0.0, 0.2])
def test_training_step_is_bitwise_reproducible(name, dropout):
    cfg, batch, c = plain_cases.build_case(name)
    cfg.dropout_rate = dropout
    b = [v.cuda() for v in batch.values()]

    def train(steps=2):
        torch.manual_seed(0)
        model = gpu_model(cfg).train()
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        step = TrainStep(model, lr=1e-4, gradient_clip_norm=4.0)
        assert step.names == json.loads(str(load_golden('grad_' + name)['with_grad']))
        losses = [float(step.step(*b)) for _ in range(steps)]
        return losses, before, {k: v.detach().clone() for k, v in model.state_dict().items()}, step.names

    l1, s0, s1, names = train()
    l2, _, s2, _ = train()
    assert all(math.isfinite(x) for x in l1) and l1 == l2
    assert all(torch.equal(s1[k], s2[k]) for k in s1)
    # every bucket parameter moves (user_node_embedding gets an exactly-zero gradient while the rows do not reach past the history slots)
    still = [k for k in names if torch.equal(s0[k], s1[k]) and not k.endswith('user_node_embedding')]
    assert not still, still
    assert 'news_encoder.category_embedding.weight' in names
    # ... and nothing outside the bucket does
    assert all(torch.equal(s0[k], s1[k]) for k in s0 if k not in names and not k.startswith('user_encoder.news_encoder.'))


def test_trainer_trains_crown_crown_for_one_epoch(tmp_path):
    """trainer.Trainer for one epoch of CROWN-CROWN on the toy dataset, with the cached device dev pass and device-side negatives: a
    checkpoint keyed 'CROWN-CROWN' that the reference-layout spec loads strictly."""
    from lime_cikm25_amd.trainer import Trainer
    d = str(tmp_path)
    cfg, corpus, model, labels = toy('CROWN', 'CROWN', batch_size=4, epoch=1, lr=1e-3, dataset='adressa', model_dir=d + '/models',
                                     best_model_dir=d + '/best', dev_res_dir=d + '/dev', result_dir=d + '/results')
    truth = formats.write_truth_file(str(tmp_path / 'truth.txt'), labels)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    trainer = Trainer(model, cfg, corpus, run_index=1, truth_file=truth, device_eval=True, device_sampling=True)
    assert trainer.train() == 1
    assert len(trainer.results['auc']) == 1 and 0.0 <= trainer.results['auc'][0] <= 1.0
    best_file = os.path.join(d, 'best', '#1', 'CROWN-CROWN')
    assert model.model_name == 'CROWN-CROWN' and os.path.exists(best_file)
    payload = torch.load(best_file, map_location='cpu', weights_only=True)
    assert 'CROWN-CROWN' in payload
    saved = payload['CROWN-CROWN']
    assert not torch.equal(saved['news_encoder.category_embedding.weight'], before['news_encoder.category_embedding.weight'].cpu())
    # the reference-layout spec: a model built from the reference's key list takes the checkpoint strictly, and the trained values arrive
    spec = [[k, list(v.shape)] for k, v in saved.items()]
    ref_layout = synth_state_dict(spec)
    assert list(ref_layout) == list(saved)
    fresh = Model(cfg)
    fresh.load_state_dict(ref_layout, strict=True)
    load_checkpoint(best_file, fresh)
    assert torch.equal(fresh.news_encoder.word_embedding.weight, saved['news_encoder.word_embedding.weight'])
    # ... and that key list is the reference's for this pairing (the golden's, with this dataset's table sizes)
    golden_keys = [k for k, _ in json.loads(str(load_golden('plain_crown_crown')['state_dict_spec']))]
    assert list(saved) == golden_keys
