"""The MLP click predictor (config.click_predictor = 'mlp'; reference model.py:113-115, :182-184) on the MI355X: the model against the
reference goldens (tests/golden/mlp_*.npz, grad_mlp_*.npz: tools/make_mlp_goldens.py) with the match on lime_grouped_mlp_match_f32
and on the composed form, graph replay against eager (bitwise), the gradients, a reproducible training step, the predictor's
training-mode dropout against a torch fp64 statement fed with the kernel's mask, and the agreement of the scoring entries: the
encode-once layout, the per-news cache, pools and lists.  The kernel itself: tests/test_grouped_mlp_match_gpu.py."""
import json
import math
import os

import numpy as np
import pytest
import torch

import mlp_cases
from helpers import GOLDEN_DIR, load_golden, rel_err
from test_naml_gpu import _with_history_fill, compare_grads, unique_named_parameters
from test_plain_gpu import topk_positions
from lime_cikm25_amd import DeviceBehaviors, DeviceCorpus, Model, formats, make_config, ops, synth, util
from lime_cikm25_amd import training as TR
from lime_cikm25_amd.training import TrainStep, negative_log_softmax

pytestmark = pytest.mark.gpu
TOL = 1e-3                      # the project's parity bound against the reference, as tests/test_user_encoders_gpu.py
KTOL = 2e-5                     # fp32-level kernel against the same sums in another order, as tests/test_user_encoders_gpu.py


def gpu_model(cfg, seed=mlp_cases.WEIGHT_SEED):
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


@pytest.fixture(params=[True, False], ids=['fused', 'composed'])
def fused(request, monkeypatch):
    """The match on lime_grouped_mlp_match_f32 and on the composed form (existing launches)."""
    monkeypatch.setattr(ops, 'FUSED_MLP_MATCH', request.param)
    return request.param


def _count_fused(monkeypatch):
    calls = []
    real = ops.grouped_mlp_match
    monkeypatch.setattr(ops, 'grouped_mlp_match', lambda *a, **kw: (calls.append(kw.get('index') is not None), real(*a, **kw))[1])
    return calls


@pytest.mark.parametrize('name', list(mlp_cases.CASES))
def test_forward_matches_the_reference(name, fused, monkeypatch):
    cfg, batch, c = mlp_cases.build_case(name)
    g = load_golden(name)
    model = gpu_model(cfg)
    calls = _count_fused(monkeypatch)
    logits = run(model, batch, c['eval_shape'])                 # eval cases: the [rows] signature (model.py:158-169)
    assert bool(calls) == fused                                 # the form asked for is the form that ran
    assert logits.shape == g['logits'].shape
    errs = {'logits': rel_err(logits.numpy(), g['logits'])}
    model.eval()
    b = {k: v.cuda() for k, v in batch.items()}
    if c['eval_shape']:
        for k in list(b):
            if k.startswith('news_') or k == 'remaining_lifetime':
                b[k] = b[k].unsqueeze(1)
    ne, ue = model.news_encoder, model.user_encoder
    with torch.no_grad():
        cand = ne(b['news_title_text'], b['news_title_mask'], b['news_title_entity'], b['news_content_text'], b['news_content_mask'],
                  b['news_content_entity'], b['news_category'], b['news_subCategory'], None, b['news_freshness'],
                  b['news_user_topic_lifetime'])
        user = ue(b['user_title_text'], b['user_title_mask'], b['user_title_entity'], b['user_content_text'], b['user_content_mask'],
                  b['user_content_entity'], b['news_category'], b['news_subCategory'], b['user_category'], b['user_subCategory'],
                  b['user_history_mask'], b['user_history_graph'], b['user_history_category_mask'],
                  b['user_history_category_indices'], None, cand, b['user_freshness'], b['user_user_topic_lifetime'])
    assert tuple(user.shape) == g['user_representation'].shape
    errs['news_representation'] = rel_err(cand.cpu().numpy(), g['news_representation'])
    errs['user_representation'] = rel_err(user.cpu().numpy(), g['user_representation'])
    print('%s (%s): %s' % (name, 'fused' if fused else 'composed', ', '.join('%s %.2e' % kv for kv in errs.items())))
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize('name', list(mlp_cases.CASES))
def test_both_forms_of_the_match_agree(name, monkeypatch):
    cfg, batch, c = mlp_cases.build_case(name)
    model = gpu_model(cfg)
    model.use_graph = False
    out = {}
    for form in (True, False):
        monkeypatch.setattr(ops, 'FUSED_MLP_MATCH', form)
        out[form] = run(model, batch, c['eval_shape'])
    e = rel_err(out[True].numpy(), out[False].numpy())
    print('%s: fused vs composed %.2e' % (name, e))
    assert e < KTOL


@pytest.mark.parametrize('kw', [dict(content_encoder='CROWN', user_encoder='CROWN'), dict(content_encoder='NAML', user_encoder='ATT'),
                                dict(news_encoder='MHSA', user_encoder='MHSA')], ids=['lime_crown_crown', 'lime_naml_att', 'mhsa_mhsa'])
def test_graph_replay_is_bitwise_equal_to_eager(kw, fused):
    """Graph replay equals eager bitwise, and ONE captured graph serves batches with different padding patterns: the offsets of the
    regular [B, N] shape are built by the eager warm-up, outside the capture."""
    cfg = make_config(**mlp_cases._CFG1, **kw)
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


@pytest.mark.parametrize('name', mlp_cases.GRAD_CASES)
def test_gradients_match_the_reference(name):
    """Loss and every gradient the reference has within TOL by ``compare_grads``; every parameter it leaves at None has none.
    ``out.bias`` is taken out of the relative check: it adds one constant to every logit of a row, the softmax loss does not feel it,
    and its gradient is identically zero -- the golden holds the reference's rounding residue (1.5e-8 and 7.5e-9 in the two cases),
    which is no scale to measure against.  It is held to an absolute bound instead (below)."""
    g = load_golden('grad_' + name)
    cfg, batch, c = mlp_cases.build_case(name)
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
    for k in json.loads(str(g['without_grad'])):
        assert named[k].grad is None, '%s: the reference leaves this gradient at None' % k
    with_grad = json.loads(str(g['with_grad']))
    assert mlp_cases.ZERO_GRADIENT in with_grad and with_grad[-4:] == ['mlp.weight', 'mlp.bias', 'out.weight', 'out.bias']
    rest = dict(g, with_grad=np.array(json.dumps([k for k in with_grad if k != mlp_cases.ZERO_GRADIENT])))
    worst = compare_grads(rest, named)
    print('%s: loss %.6f (reference %.6f), worst gradient %s rel err %.2e' % (name, float(loss.detach()), float(g['loss']), *worst))
    # The gradient of out.bias is (1 / B) sum_b sum_n d[b, n] with d = softmax(logits[b]) - onehot: B N terms.  Each d[b, n] / B is at
    # most 1 / B in magnitude and carries at most one fp32 epsilon of relative error from the softmax (2^-23 / B absolute); summing
    # B N such terms, every partial sum at most 1 in magnitude, adds at most half an epsilon per addition.  Together at most
    # N eps + B N eps / 2 <= B N eps for B >= 2: the number of logits times fp32's epsilon.  (The exact value is 0.)
    bound = logits.numel() * 2.0 ** -23
    got = float(named[mlp_cases.ZERO_GRADIENT].grad.abs().max())
    residue = float(np.abs(g['full:' + mlp_cases.ZERO_GRADIENT]).max())
    print('%s: |d loss / d out.bias| %.2e, the reference\'s residue %.2e, bound %.2e' % (name, got, residue, bound))
    assert got <= bound and residue <= bound


@pytest.mark.parametrize('name', mlp_cases.GRAD_CASES)
@pytest.mark.parametrize('dropout', [0.0, 0.2])
def test_training_step_is_bitwise_reproducible(name, dropout):
    cfg, batch, c = mlp_cases.build_case(name)
    cfg.dropout_rate = dropout
    b = [v.cuda() for v in batch.values()]

    def train(steps=2):
        torch.manual_seed(0)
        model = gpu_model(cfg).train()
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        step = TrainStep(model, lr=1e-4, gradient_clip_norm=4.0)
        assert step.names == json.loads(str(load_golden('grad_' + name)['with_grad']))
        losses = [float(step.step(*b)) for _ in range(steps)]
        return losses, before, {k: v.detach().clone() for k, v in model.state_dict().items()}

    l1, s0, s1 = train()
    l2, _, s2 = train()
    assert all(math.isfinite(x) for x in l1) and l1 == l2
    assert all(torch.equal(s1[k], s2[k]) for k in s1)
    for k in ('mlp.weight', 'mlp.bias', 'out.weight'):                     # the predictor trains
        assert not torch.equal(s0[k], s1[k]), k


@pytest.mark.parametrize('user_rows', ['per_candidate', 'pooled'])
def test_predictor_dropout_matches_torch_on_the_same_mask(user_rows):
    """Training mode: ``Model.dropout`` (p = config.dropout_rate) behind the predictor's ReLU (model.py:183).  The mask is read back
    through ops.dropout on an all-ones tensor and fed to a torch fp64 statement; the logits and the gradients of both inputs and of
    the four parameters must match.  In eval mode the site draws nothing."""
    cfg = make_config(content_encoder='NAML', user_encoder='ATT', vocabulary_size=3000, max_history_num=6, batch_size=8, dropout_rate=0.2,
                      click_predictor='mlp')
    model = gpu_model(cfg, seed=71)
    B, N, D = 6, 3, model.news_embedding_dim
    Dh = D // 2
    g = torch.Generator().manual_seed(72)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1
    user, cand, G = rnd(B, N if user_rows == 'per_candidate' else 1, D), rnd(B, N, D), rnd(B, N)
    ud, cd = user.float().cuda().requires_grad_(True), cand.float().cuda().requires_grad_(True)
    model.train()
    torch.manual_seed(5)
    out = TR.mlp_logits(model, ud, cd)
    (out * G.float().cuda()).sum().backward()
    torch.manual_seed(5)
    mask = ops.dropout(torch.ones(B * N, Dh, device='cuda'), 0.2, TR._draw_seed(), TR._SITE_CLICK_PREDICTOR).cpu().double()
    assert 0.1 < float((mask == 0).double().mean()) < 0.3 and mask.unique().numel() == 2
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.named_parameters() if k.startswith(('mlp.', 'out.'))}
    u64, c64 = user.clone().requires_grad_(True), cand.clone().requires_grad_(True)
    x = torch.cat([u64.expand(B, N, D), c64], dim=2).reshape(B * N, 2 * D)
    hidden = torch.relu(x @ sd['mlp.weight'].t() + sd['mlp.bias']) * mask                                     # model.py:183
    want = (hidden @ sd['out.weight'].t() + sd['out.bias']).view(B, N)                                        # :184
    e = rel_err(out.detach().cpu().numpy(), want.detach().numpy())
    print('logits under dropout (%s): %.2e' % (user_rows, e))
    assert e < TOL
    (want * G).sum().backward()
    assert rel_err(ud.grad.cpu().numpy(), u64.grad.numpy()) < TOL and rel_err(cd.grad.cpu().numpy(), c64.grad.numpy()) < TOL
    named = dict(model.named_parameters())
    for k, v in sd.items():
        assert rel_err(named[k].grad.cpu().numpy(), v.grad.numpy()) < TOL, k
    # eval mode: no mask, and nothing is drawn from the generator
    model.eval()
    state = torch.random.get_rng_state()
    with torch.no_grad():
        plain = TR.mlp_logits(model, ud.detach(), cd.detach())
    assert torch.equal(torch.random.get_rng_state(), state)
    hidden = torch.relu(x @ sd['mlp.weight'].t() + sd['mlp.bias'])
    assert rel_err(plain.cpu().numpy(), (hidden @ sd['out.weight'].t() + sd['out.bias']).view(B, N).detach().numpy()) < TOL


def test_model_forward_in_training_mode_draws_the_predictor_dropout():
    """``model.train()`` under no_grad takes the differentiable path with its dropouts (Model.forward): with config.dropout_rate > 0 two
    seeds give two results, one seed the same bits; the scoring chain refuses to run with the dropout active."""
    cfg, batch, c = mlp_cases.build_case('mlp_lime_naml_att')
    cfg.dropout_rate = 0.2
    model = gpu_model(cfg).train()
    b = [v.cuda() for v in batch.values()]
    outs = []
    with torch.no_grad():
        for seed in (1, 1, 2):
            torch.manual_seed(seed)
            outs.append(model(*b))
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    with pytest.raises(NotImplementedError, match='dropout'), torch.no_grad():
        model._forward_impl(*b)


PAIRINGS = [dict(content_encoder='CROWN', user_encoder='CROWN'), dict(content_encoder='NAML', user_encoder='ATT'),
            dict(content_encoder='NAML', user_encoder='ATT', use_candidate_ware_clicked_news_attention=False),
            dict(news_encoder='MHSA', user_encoder='MHSA'), dict(news_encoder='CROWN', user_encoder='CROWN')]
PAIRING_IDS = ['lime_crown_crown', 'lime_naml_att', 'lime_naml_att_attention_off', 'mhsa_mhsa', 'crown_crown']


@pytest.mark.parametrize('kw', PAIRINGS, ids=PAIRING_IDS)
def test_score_impressions_equals_eval_forward_on_expanded_rows(kw, fused):
    """B impressions x K candidates with every history encoded once (hist_div = K) against the eval forward on the B * K expanded rows
    (not bitwise: the two layouts give the GEMMs other row counts -- the kernel-level bound).  Chunked passes are bitwise."""
    cfg = make_config(max_history_num=10, max_title_length=16, max_abstract_length=32, batch_size=64, vocabulary_size=5000,
                      click_predictor='mlp', **kw)
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
    print('score_impressions vs expanded rows: %.2e' % e)
    assert e < KTOL
    assert torch.equal(model.score_impressions(*args, rows_per_pass=2 * K), got)


def toy(**kw):
    """The toy dataset of tests/golden/formats.json, as tests/test_plain_gpu.py uses it."""
    g = json.load(open(os.path.join(GOLDEN_DIR, 'formats.json')))
    L = g['lines']
    cfg = make_config(max_history_num=g['max_history_num'], max_title_length=g['max_title_length'], click_predictor='mlp',
                      max_abstract_length=g['max_abstract_length'], vocabulary_size=len(g['word_dict']), negative_sample_num=2,
                      category_num=len(g['category_dict']) + 1, subCategory_num=len(g['subCategory_dict']) + 1,
                      user_num=len(g['user_ID_dict']), batch_size=16, **kw)
    corpus = formats.build_corpus(cfg, [L['train_news'], L['dev_news'], L['test_news']],
                                  [L['train_behaviors'], L['dev_behaviors'], L['test_behaviors']], g['news_ID_dict'],
                                  g['user_ID_dict'], g['category_dict'], g['subCategory_dict'], g['word_dict'], dataset='adressa')
    torch.manual_seed(0)
    np.random.seed(0)
    model = Model(cfg)
    model.initialize()
    torch.nn.init.normal_(model.content_encoder.word_embedding.weight, std=0.1)
    return cfg, corpus, model.cuda(), formats.truth_labels(L['dev_behaviors'])


@pytest.mark.parametrize('kw', [PAIRINGS[0], PAIRINGS[1], PAIRINGS[3]], ids=[PAIRING_IDS[0], PAIRING_IDS[1], PAIRING_IDS[3]])
def test_the_cached_passes_agree_with_the_uncached_forward(kw, fused, tmp_path):
    """build_news_cache + score_behaviors against the uncached eval forward on the same rows and n_src; util.compute_scores_cached against
    util.compute_scores (the same rank file and metrics); evaluate_cached_on_device, row-wise and grouped, against the cached host pass."""
    cfg, corpus, model, labels = toy(**kw)
    dc = DeviceCorpus(corpus)
    dev = DeviceBehaviors.from_devtest(dc, corpus, 'dev')
    model.eval()
    cache = model.build_news_cache(dc)
    rows = list(range(dev.num))
    model.use_graph = False
    with torch.no_grad():
        batch = dev.assemble(rows)
        plain = model(*batch, batch[24] - batch[23]).view(-1)           # remaining lifetime: util.py:98-106, lifetime_type 'user_topic'
    cached = model.score_behaviors(dev, rows, cache, n_src=dev.num)
    e = rel_err(cached.cpu().numpy(), plain.cpu().numpy())
    print('score_behaviors vs the uncached eval forward %.2e over %d rows' % (e, dev.num))
    assert e < KTOL and plain.unique().numel() > dev.num // 2
    model.use_graph = True
    truth = formats.write_truth_file(str(tmp_path / 'truth.txt'), labels)
    per = max(dev.num, 64) if cfg.user_encoder != 'CROWN' else dev.num
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
    'lime_crown': dict(content_encoder='CROWN', user_encoder='CROWN'),
    'lime_att': dict(content_encoder='CROWN', user_encoder='ATT'),
    'crown_crown': dict(news_encoder='CROWN', user_encoder='CROWN'),                      # a baseline: the tables read in place, Dh = 450
    'crown_att': dict(news_encoder='CROWN', user_encoder='ATT'),
    'mhsa_mhsa_attention_off': dict(news_encoder='MHSA', user_encoder='MHSA', use_candidate_ware_clicked_news_attention=False),   # Dh = 150
}
_BUILT = {}


def serving(name):
    """(model, the pool's arguments and its rows as a DeviceBehaviors, n_src, the lists' arguments and their rows, n_src, the lists'
    offsets) -- once per case; the yardstick, score_behaviors over the rows written out, is taken by the test under its own form."""
    if name in _BUILT:
        return _BUILT[name]
    cfg = make_config(**{**mlp_cases._TINY, **SERVING[name]})
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
    clt = (cfr[None, :].astype(np.float64) + rng.uniform(-8.0, 8.0, size=(U, C))).astype(np.float32)
    model = Model(cfg)
    model.initialize()
    synth.fill_state_dict(model, seed=43)
    model = model.cuda().eval()
    cache = model.build_news_cache(dc)
    t = lambda a: torch.from_numpy(a).cuda()
    users = dict(news_cache=cache, corpus=dc, hist_index=t(hist), hist_mask=t(mask), user_freshness=t(ufr), user_lifetime=t(ult))
    beh = DeviceBehaviors(dc, np.repeat(np.arange(U), C), np.repeat(hist, C, axis=0), np.repeat(mask, C, axis=0), np.repeat(ufr, C, axis=0),
                          np.repeat(ult, C, axis=0), np.tile(pool, U).reshape(U * C, 1), np.tile(cfr, U).reshape(U * C, 1),
                          clt.reshape(U * C, 1), eval_shape=True)
    n_src = min(U * C, H + cfg.batch_size)
    pool_args = dict(users, cand_index=t(pool), cand_freshness=t(cfr), cand_lifetime=t(clt))
    # the lists: 0, 1 and 9 candidates (the nine span four topics)
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
    _BUILT[name] = (model, pool_args, beh, n_src, list_args, lbeh, n_src_l, off)
    return _BUILT[name]


@pytest.mark.parametrize('name', list(SERVING))
def test_score_pool_and_recommend_equal_the_cached_pass(name, fused, monkeypatch):
    model, args, beh, n_src, *_ = serving(name)
    want = model.score_behaviors(beh, torch.arange(U * C, device='cuda'), args['news_cache'], n_src=n_src).view(U, C)
    calls = _count_fused(monkeypatch)
    got = model.score_pool(**args, n_src=n_src)
    assert bool(calls) == fused
    if fused:                                                              # a baseline reads its tables in place, a LIME model cannot
        assert all(c == (model.plain) for c in calls)
    assert got.shape == (U, C) and torch.isfinite(got).all()
    e = rel_err(got.cpu().numpy(), want.cpu().numpy())
    print('%s (%s): score_pool vs score_behaviors rel err %.2e over %d pairs (%d distinct scores)' % (
        name, 'fused' if fused else 'composed', e, U * C, want.unique().numel()))
    assert e < KTOL
    assert want.unique().numel() > U * C // 2                              # the pass is a yardstick: scores differ pair by pair
    many = model.score_pool(**args, n_src=n_src, pairs_per_pass=1)         # one user a pass
    assert rel_err(many.cpu().numpy(), want.cpu().numpy()) < KTOL
    pos, top = model.recommend(**args, k=K, n_src=n_src)
    for u in range(U):
        assert pos[u].tolist() == topk_positions(got[u].cpu().numpy(), K)
        assert torch.equal(top[u], got[u][pos[u].long()])


@pytest.mark.parametrize('name', list(SERVING))
def test_score_lists_and_recommend_lists_equal_the_cached_pass(name, fused, monkeypatch):
    model, _, _, _, args, lbeh, n_src, off = serving(name)
    want = model.score_behaviors(lbeh, torch.arange(sum(LENS), device='cuda'), args['news_cache'], n_src=n_src)
    calls = _count_fused(monkeypatch)
    got = model.score_lists(**args, n_src=n_src)
    assert bool(calls) == fused
    assert got.shape == (sum(LENS),) and torch.isfinite(got).all()
    e = rel_err(got.cpu().numpy(), want.cpu().numpy())
    print('%s (%s): score_lists vs score_behaviors rel err %.2e over %d pairs' % (name, 'fused' if fused else 'composed', e, sum(LENS)))
    assert e < KTOL
    pos, top = model.recommend_lists(**args, k=K, n_src=n_src)
    assert pos.shape == (U, K)
    for u in range(U):
        s = got[off[u]:off[u + 1]].cpu().numpy()
        assert pos[u].tolist() == topk_positions(s, K)
        live = pos[u][pos[u] >= 0].long()
        assert torch.equal(top[u][:live.numel()], got[off[u]:off[u + 1]][live]) and torch.isneginf(top[u][live.numel():]).all()
