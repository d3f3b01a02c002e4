"""LIME-KCNN-{CROWN,ATT,MHSA} on the MI355X, at TOL = 1e-3 throughout: the model against the reference goldens
(tests/golden/kcnn_*.npz, grad_kcnn_*.npz: tools/make_kcnn_goldens.py), graph replay against eager (bitwise), score_impressions against
the eval forward on expanded rows, the per-news content cache against the uncached forward, a reproducible training step that moves
the encoder's own parameters, and the dropout sites of training mode."""
import json
import math
import os

import pytest
import torch

import kcnn_cases
from helpers import load_golden, rel_err
from lime_cikm25_amd import Model, make_config, ops, synth
from lime_cikm25_amd import training as TR
from lime_cikm25_amd.training import TrainStep, negative_log_softmax

pytestmark = pytest.mark.gpu
TOL = 1e-3                      # the project's parity bound against the reference, as test_user_encoders_gpu.py
KTOL = 2e-5                     # fp32-level kernels against the same sums in another order, as test_user_encoders_gpu.py
HIST_ROWS = 2                   # tools/make_kcnn_goldens.py stores history-level taps for the first rows only


def gpu_model(cfg, seed=kcnn_cases.WEIGHT_SEED):
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


@pytest.fixture(params=[True, False], ids=['fused', 'unfused'])
def fused_conv_pool(request, monkeypatch):
    monkeypatch.setattr(ops, 'FUSED_CONV_POOL', request.param)
    return request.param


@pytest.mark.parametrize('name', list(kcnn_cases.CASES))
def test_forward_matches_the_reference(name, fused_conv_pool):
    cfg, batch, c = kcnn_cases.build_case(name)
    g = load_golden(name)
    model = gpu_model(cfg)
    logits = run(model, batch, c['eval_shape'])
    assert logits.shape == g['logits'].shape
    e = rel_err(logits.numpy(), g['logits'])
    print('%s: logits vs reference golden %.2e' % (name, e))
    assert e < TOL
    model.eval()
    b = {k: v.cuda() for k, v in batch.items()}
    if c['eval_shape']:
        b = {k: (v.unsqueeze(1) if k.startswith('news_') else v) for k, v in b.items()}
    ne, ue = model.news_encoder, model.user_encoder
    news_args = (b['news_title_text'], b['news_title_mask'], b['news_title_entity'], b['news_content_text'], b['news_content_mask'],
                 b['news_content_entity'], b['news_category'], b['news_subCategory'], None, b['news_freshness'], b['news_user_topic_lifetime'])
    hist_args = (b['user_title_text'], b['user_title_mask'], b['user_title_entity'], b['user_content_text'], b['user_content_mask'],
                 b['user_content_entity'], b['user_category'], b['user_subCategory'], None, b['user_freshness'], b['user_user_topic_lifetime'])
    with torch.no_grad():
        cand = ne(*news_args)
        content = ne.base_news_encoder(*news_args)
        hist_content = ne.base_news_encoder(*hist_args)
        user = ue(b['user_title_text'], b['user_title_mask'], b['user_title_entity'], b['user_content_text'], b['user_content_mask'],
                  b['user_content_entity'], b['news_category'], b['news_subCategory'], b['user_category'], b['user_subCategory'],
                  b['user_history_mask'], b['user_history_graph'], b['user_history_category_mask'],
                  b['user_history_category_indices'], None, cand, b['user_freshness'], b['user_user_topic_lifetime'])
    assert rel_err(cand.cpu().numpy(), g['news_representation']) < TOL
    assert rel_err(content.cpu().numpy(), g['content_candidates']) < TOL
    assert rel_err(hist_content.cpu().numpy()[:HIST_ROWS], g['content_history']) < TOL
    assert rel_err(user.cpu().numpy(), g['user_representation']) < TOL


def unique_named_parameters(model):
    seen = set()
    for k, p in model.named_parameters():
        if id(p) not in seen:
            seen.add(id(p))
            yield k, p


def compare_grads(g, named):
    """tests/test_training_gpu.py's procedure (copied): every gradient the reference has, against its full tensor or its largest
    entries + L2 norm."""
    worst = ('', 0.0)
    for k in json.loads(str(g['with_grad'])):
        got = named[k].grad
        assert got is not None, '%s has no gradient' % k
        got = got.detach().cpu().double().reshape(-1)
        assert torch.isfinite(got).all(), k
        scale = float(g['norm:' + k]) / max(1.0, got.numel()) ** 0.5
        if 'full:' + k in g:
            want = g['full:' + k].reshape(-1)
            e = rel_err(got.numpy(), want, floor=max(scale, 1e-5))
        else:
            idx, want = g['idx:' + k], g['val:' + k]
            e = rel_err(got.numpy()[idx], want, floor=max(scale, 1e-5))
            e = max(e, abs(float(got.norm()) - float(g['norm:' + k])) / (float(g['norm:' + k]) + 1e-6))
        if e > worst[1]:
            worst = (k, e)
        assert e < TOL, '%s: gradient rel err %.3e' % (k, e)
    return worst


@pytest.mark.parametrize('name', kcnn_cases.GRAD_CASES)
def test_gradients_match_the_reference(name):
    """Loss and every gradient the reference has within TOL by ``compare_grads``; every parameter it leaves at None has none."""
    g = load_golden('grad_' + name)
    cfg, batch, c = kcnn_cases.build_case(name)
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
    worst = compare_grads(g, named)
    print('%s: loss %.6f (reference %.6f), worst gradient %s rel err %.2e' % (name, float(loss.detach()), float(g['loss']), *worst))


def _with_history_fill(cfg, batch, fill):
    """Copy of ``batch`` whose row b has its first fill(b) history slots live and the rest the padding news."""
    b2 = type(batch)((k, v.clone()) for k, v in batch.items())
    for b in range(b2['user_history_mask'].shape[0]):
        n = fill(b)
        for k in ('user_category', 'user_subCategory', 'user_title_text', 'user_title_entity', 'user_content_text'):
            b2[k][b, n:] = 0
        b2['user_title_mask'][b, n:] = False
        b2['user_title_mask'][b, n:, 0] = True
        b2['user_history_mask'][b, :n] = True
        b2['user_history_mask'][b, n:] = False
    return b2


def _batch(cfg, B, N, seed, eval_shape=False):
    return kcnn_cases.with_entities(cfg, synth.make_batch(cfg, B, N, seed=seed, eval_shape=eval_shape), seed)


@pytest.mark.parametrize('user', ['CROWN', 'MHSA'])
def test_one_captured_graph_follows_the_padding_pattern(user, fused_conv_pool):
    """Graph replay equals eager bitwise, and ONE captured graph (its inputs include the two entity tensors) serves batches with
    different padding patterns and entity ids."""
    cfg = make_config(content_encoder='KCNN', user_encoder=user, vocabulary_size=5000, entity_size=700, max_history_num=10,
                      max_title_length=16, max_abstract_length=32)
    model = gpu_model(cfg, seed=61)
    H = cfg.max_history_num
    A = _batch(cfg, 8, 3, 62)
    batches = {'A': A, 'B': _with_history_fill(cfg, A, lambda b: H), 'C': _with_history_fill(cfg, A, lambda b: 1 if b % 4 == 0 else 0),
               'D': _with_history_fill(cfg, _batch(cfg, 8, 3, 63), lambda b: (7 * b) % (H + 1))}
    model.use_graph = True
    model._graphs.clear()
    got = {}
    for name in ('A', 'B', 'C', 'D', 'A'):
        got.setdefault(name, []).append(run(model, batches[name]))
    assert len(model._graphs) == 1
    assert torch.equal(got['A'][0], got['A'][1])
    assert not torch.equal(got['A'][0], got['D'][0])
    model.use_graph = False
    for name in ('A', 'B', 'C', 'D'):
        want = run(model, batches[name])
        assert torch.isfinite(want).all() and torch.equal(got[name][0], want), name
    # the entity ids are inputs of the graph: other ids, other logits
    model.use_graph = True
    E = type(A)((k, v.clone()) for k, v in A.items())
    E['news_title_entity'] = torch.where(E['news_title_text'] != 0, (E['news_title_entity'] + 5) % cfg.entity_size, E['news_title_entity'])
    moved = run(model, E)
    assert len(model._graphs) == 1 and not torch.equal(moved, got['A'][0])
    model.use_graph = False
    assert torch.equal(moved, run(model, E))


@pytest.mark.parametrize('user', ['CROWN', 'ATT', 'MHSA'])
def test_score_impressions_equals_eval_forward_on_expanded_rows(user):
    """B impressions x K candidates with every history encoded once against the eval forward on the B * K expanded rows, within the
    kernel-level bound (the two layouts give the GEMMs different row counts); the entity ids are required."""
    cfg = make_config(content_encoder='KCNN', user_encoder=user, max_history_num=10, max_title_length=16, max_abstract_length=32,
                      batch_size=64, vocabulary_size=5000, entity_size=700)
    model = gpu_model(cfg, seed=41)
    B, K = 5, 6
    batch = _batch(cfg, B, K, 42)
    c = {k: v.cuda() for k, v in batch.items()}
    model.eval()
    args = (c['user_category'], c['user_subCategory'], c['user_title_text'], c['user_title_mask'], c['user_content_text'],
            c['user_freshness'], c['user_user_topic_lifetime'], c['user_history_mask'], c['news_category'], c['news_subCategory'],
            c['news_title_text'], c['news_title_mask'], c['news_content_text'], c['news_freshness'], c['news_user_topic_lifetime'],
            c['remaining_lifetime'])
    ents = dict(user_title_entity=c['user_title_entity'], news_title_entity=c['news_title_entity'])
    with pytest.raises(TypeError, match='title_entity'):
        model.score_impressions(*args)
    got = model.score_impressions(*args, **ents)
    assert got.shape == (B, K)
    exp = type(batch)()
    for k, v in batch.items():
        exp[k] = v.reshape((B * K,) + tuple(v.shape[2:])) if (k.startswith('news_') or k == 'remaining_lifetime') else v.repeat_interleave(K, dim=0)
    model.use_graph = False
    ref_rows = run(model, exp, True)
    e = rel_err(got.cpu().reshape(-1).numpy(), ref_rows.reshape(-1).numpy())
    print('score_impressions vs expanded rows: %.2e' % e)
    assert e < KTOL
    again = model.score_impressions(*args, rows_per_pass=2 * K, **ents)
    assert torch.equal(again, got)


@pytest.mark.parametrize('user', ['CROWN', 'ATT'])
def test_content_cache_agrees_with_the_uncached_forward(user, tmp_path):
    """util.compute_scores_cached (every news through KCNN once, build_content_cache reading DeviceCorpus.news_title_entity) against
    util.compute_scores on the toy corpus with random entity ids: the same rank file and metrics."""
    from lime_cikm25_amd import formats, util
    from lime_cikm25_amd.device_data import DeviceBehaviors, DeviceCorpus
    from helpers import GOLDEN_DIR
    g = json.load(open(os.path.join(GOLDEN_DIR, 'formats.json')))
    L = g['lines']
    cfg = make_config(content_encoder='KCNN', user_encoder=user, max_history_num=g['max_history_num'], max_title_length=g['max_title_length'],
                      max_abstract_length=g['max_abstract_length'], vocabulary_size=len(g['word_dict']), negative_sample_num=2,
                      category_num=len(g['category_dict']) + 1, subCategory_num=len(g['subCategory_dict']) + 1,
                      user_num=len(g['user_ID_dict']), batch_size=16, entity_size=40)
    corpus = formats.build_corpus(cfg, [L['train_news'], L['dev_news'], L['test_news']],
                                  [L['train_behaviors'], L['dev_behaviors'], L['test_behaviors']], g['news_ID_dict'],
                                  g['user_ID_dict'], g['category_dict'], g['subCategory_dict'], g['word_dict'], dataset='adressa')
    # the caller fills the entity ids: random ids on the live title tokens
    ent = synth.randint('toy.title_entity', 0, corpus.news_title_text.size, 0, cfg.entity_size).reshape(corpus.news_title_text.shape)
    corpus.news_title_entity = (ent * (corpus.news_title_text != 0)).astype(corpus.news_title_text.dtype)
    assert int((corpus.news_title_entity != 0).sum()) > 0
    dev = DeviceBehaviors.from_devtest(DeviceCorpus(corpus), corpus, 'dev')
    torch.manual_seed(0)
    model = Model(cfg)
    model.initialize()
    enc = model.news_encoder.base_news_encoder
    torch.nn.init.normal_(enc.word_embedding.weight, std=0.1)
    torch.nn.init.normal_(enc.entity_embedding.weight, std=0.5)
    torch.nn.init.normal_(enc.context_embedding.weight, std=0.5)
    model = model.cuda()
    truth = tmp_path / 'truth.txt'
    with open(truth, 'w') as f:
        for i, labels in enumerate(formats.truth_labels(L['dev_behaviors'])):
            f.write('%d %s\n' % (i + 1, json.dumps(labels).replace(' ', '')))
    a = util.compute_scores(model, [dev.assemble(list(range(dev.num)))], corpus.dev_indices, str(tmp_path / 'rank.txt'), str(truth))
    # CROWN's GraphSAGE bounds the rows of a forward by its node slots; ATT has no such bound: twice the batch size is as legal as any
    per = dev.num if user == 'CROWN' else max(dev.num, 64)
    b = util.compute_scores_cached(model, dev, corpus.dev_indices, str(tmp_path / 'rank_cached.txt'), str(truth), rows_per_forward=per)
    assert open(tmp_path / 'rank_cached.txt').read() == open(tmp_path / 'rank.txt').read()
    assert a == b
    # the entity ids reach the cache: without them its rows differ
    with_ids = model.build_news_cache(dev.corpus)
    saved = dev.corpus.news_title_entity
    dev.corpus.news_title_entity = torch.zeros_like(saved)
    try:
        assert not torch.equal(model.build_news_cache(dev.corpus), with_ids)
    finally:
        dev.corpus.news_title_entity = saved


@pytest.mark.parametrize('name', ['kcnn_naive', 'kcnn_group4_att'])
def test_training_step_is_bitwise_reproducible(name):
    cfg, batch, c = kcnn_cases.build_case(name)
    b = [v.cuda() for v in batch.values()]
    prefix = 'news_encoder.base_news_encoder.'

    def train(steps=3):
        torch.manual_seed(0)
        model = gpu_model(cfg).train()
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        step = TrainStep(model, lr=1e-5, gradient_clip_norm=4.0)
        for k in ('entity_embedding.weight', 'context_embedding.weight', 'M_entity.weight', 'M_context.bias'):
            assert prefix + k in step.names
        losses = [float(step.step(*b)) for _ in range(steps)]
        return losses, before, {k: v.detach().clone() for k, v in model.state_dict().items()}

    l1, s0, s1 = train()
    l2, _, s2 = train()
    assert all(math.isfinite(x) for x in l1) and l1 == l2
    assert all(torch.equal(s1[k], s2[k]) for k in s1)
    assert l1[0] != l1[-1]                                     # the steps did update the parameters
    moved = [k for k in s0 if k.startswith(prefix) and not torch.equal(s0[k], s1[k])]
    for part in ('knowledge_cnn.', 'M_entity.weight', 'M_context.weight', 'entity_embedding.weight', 'context_embedding.weight'):
        assert any(k.startswith(prefix + part) for k in moved), part
    assert torch.equal(s0[prefix + 'subCategory_embedding.weight'], s1[prefix + 'subCategory_embedding.weight'])


def test_training_mode_dropout_draws_only_the_feature_fusion_sites():
    """Training mode at dropout_rate 0.2 (newsEncoders.py:221-226, :625-638): the convolution's columns are the eval ones bit for bit --
    no dropout in front of or behind the convolution -- and the category / subcategory columns are the eval ones under the masks of
    sites 0 and 1, read back through ops.dropout on all-ones tensors."""
    cfg = make_config(content_encoder='KCNN', vocabulary_size=3000, entity_size=300, max_title_length=16, dropout_rate=0.2)
    model = gpu_model(cfg, seed=71)
    enc = model.news_encoder.base_news_encoder
    M, T, p, K = 48, cfg.max_title_length, 0.2, cfg.cnn_kernel_num
    g = torch.Generator().manual_seed(73)
    ids = torch.randint(0, cfg.vocabulary_size, (M, T), generator=g, dtype=torch.int32).cuda()
    ent = (torch.randint(0, cfg.entity_size, (M, T), generator=g, dtype=torch.int32) * (torch.rand(M, T, generator=g) < 0.25)).int().cuda()
    cat = torch.randint(0, cfg.category_num, (M,), generator=g, dtype=torch.int32).cuda()
    sub = torch.randint(0, cfg.subCategory_num, (M,), generator=g, dtype=torch.int32).cuda()
    mask = (ids != 0)
    enc.eval()
    with torch.no_grad():
        plain = TR.content_flat(enc, ids, mask, ids, cat, sub, title_entity=ent)
    enc.train()
    torch.manual_seed(5)
    out = TR.content_flat(enc, ids, mask, ids, cat, sub, title_entity=ent)
    assert out.requires_grad
    torch.manual_seed(5)
    seed = TR._draw_seed()
    m_cat = ops.dropout(torch.ones(M, 50, device='cuda'), p, seed, 0)
    m_sub = ops.dropout(torch.ones(M, 50, device='cuda'), p, seed, 1)
    assert 0.05 < float((m_cat == 0).float().mean()) < 0.4 and not torch.equal(m_cat, m_sub)
    assert torch.equal(out[:, :K].detach(), plain[:, :K])
    assert rel_err(out[:, K:K + 50].detach().cpu().numpy(), (plain[:, K:K + 50] * m_cat).cpu().numpy()) < 1e-6
    assert rel_err(out[:, K + 50:].detach().cpu().numpy(), (plain[:, K + 50:] * m_sub).cpu().numpy()) < 1e-6
    out.sum().backward()
    assert enc.knowledge_cnn.conv.weight.grad is not None and enc.entity_embedding.weight.grad is not None
