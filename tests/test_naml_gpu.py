"""LIME-NAML-CROWN on the MI355X: the model against the reference goldens (tests/golden/naml_*.npz, grad_naml_*.npz:
tools/make_naml_goldens.py), the compacted path against the dense one and graph replay against eager (bitwise), a reproducible training
step, training-mode dropout against a torch fp64 statement fed with the kernels' masks, and the per-news content cache against the
uncached forward.  The fused attention pool itself: tests/test_attn_pool_gpu.py."""
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

import naml_cases
from helpers import load_golden, rel_err
from lime_cikm25_amd import Model, make_config, newsEncoders, ops, synth
from lime_cikm25_amd import training as TR
from lime_cikm25_amd.training import TrainStep, negative_log_softmax

pytestmark = pytest.mark.gpu
TOL = 1e-3                      # the north star, as test_model_gpu.py
HIST_ROWS = 2                   # tools/make_goldens.py stores history-level taps for the first rows only


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale


def ref_conv(x, w, b, T):
    """fp64 nn.Conv1d over sequences of T rows: x [n T, C], w [O, C, win] -> [n T, O] (zero padding at the sequence ends)."""
    n = x.shape[0] // T
    y = F.conv1d(x.view(n, T, -1).permute(0, 2, 1), w, b, padding=(w.shape[2] - 1) // 2)
    return y.permute(0, 2, 1).reshape(n * T, -1)


def _ids(n, T, V, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, V, (n, T), generator=g, dtype=torch.int32)
    lens = torch.randint(1, T + 1, (n,), generator=g)
    for s in range(n):
        ids[s, lens[s]:] = 0                                   # padding word 0 behind the text
    ids[0] = 0                                                 # one all-padding sequence
    return ids


def gpu_model(cfg, seed=naml_cases.WEIGHT_SEED):
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


@pytest.fixture(params=[False, True], ids=['two_launch', 'fused'])
def fused_pool(request, monkeypatch):
    """The attention pools on linear(tanh) + additive_pool (the dispatcher's default) and on the fused launch."""
    monkeypatch.setattr(ops, 'FUSED_ATTN_POOL', request.param)
    return request.param


@pytest.mark.parametrize('name', list(naml_cases.CASES))
def test_forward_matches_the_reference(name, fused_pool):
    cfg, batch, c = naml_cases.build_case(name)
    g = load_golden(name)
    model = gpu_model(cfg)
    logits = run(model, batch, c['eval_shape'])
    assert logits.shape == g['logits'].shape
    e = rel_err(logits.numpy(), g['logits'])
    print('%s: logits vs reference golden %.2e' % (name, e))
    assert e < TOL
    if c['eval_shape']:
        return
    model.eval()
    b = {k: v.cuda() for k, v in batch.items()}
    ne, ue = model.news_encoder, model.user_encoder
    with torch.no_grad():
        cand = ne(b['news_title_text'], b['news_title_mask'], b['news_title_entity'], b['news_content_text'], b['news_content_mask'],
                  b['news_content_entity'], b['news_category'], b['news_subCategory'], None, b['news_freshness'],
                  b['news_user_topic_lifetime'])
        hist_args = (b['user_title_text'], b['user_title_mask'], b['user_title_entity'], b['user_content_text'], b['user_content_mask'],
                     b['user_content_entity'], b['user_category'], b['user_subCategory'], None, b['user_freshness'],
                     b['user_user_topic_lifetime'])
        content = ne.base_news_encoder(b['news_title_text'], b['news_title_mask'], b['news_title_entity'], b['news_content_text'],
                                       b['news_content_mask'], b['news_content_entity'], b['news_category'], b['news_subCategory'],
                                       None, b['news_freshness'], b['news_user_topic_lifetime'])
        hist_content = ne.base_news_encoder(*hist_args)
        user = ue(b['user_title_text'], b['user_title_mask'], b['user_title_entity'], b['user_content_text'], b['user_content_mask'],
                  b['user_content_entity'], b['news_category'], b['news_subCategory'], b['user_category'], b['user_subCategory'],
                  b['user_history_mask'], b['user_history_graph'], b['user_history_category_mask'],
                  b['user_history_category_indices'], None, cand, b['user_freshness'], b['user_user_topic_lifetime'])
    assert rel_err(cand.cpu().numpy(), g['news_representation']) < TOL
    assert rel_err(content.cpu().numpy(), g['cand_content']) < TOL
    assert rel_err(hist_content.cpu().numpy()[:HIST_ROWS], g['hist_content']) < TOL
    assert rel_err(user.cpu().numpy(), g['user_representation']) < TOL


def unique_named_parameters(model):
    seen = set()
    for k, p in model.named_parameters():
        if id(p) not in seen:
            seen.add(id(p))
            yield k, p


def compare_grads(g, named):
    """tests/test_training_gpu.py's procedure (copied): every gradient the reference has, against its full tensor or its 2048
    largest entries + L2 norm."""
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


@pytest.mark.parametrize('name', naml_cases.GRAD_CASES)
def test_gradients_match_the_reference(name):
    g = load_golden('grad_' + name)
    cfg, batch, c = naml_cases.build_case(name)
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


def _full_cfg(**over):
    return make_config(content_encoder='NAML', vocabulary_size=50000, **over)


def _with_history_fill(cfg, batch, fill):
    """Copy of ``batch`` whose row b has its first fill(b) history slots live and the rest the padding news."""
    b2 = {k: v.clone() for k, v in batch.items()}
    H = cfg.max_history_num
    for b in range(b2['user_history_mask'].shape[0]):
        n = fill(b)
        for k in ('user_category', 'user_subCategory', 'user_title_text', 'user_content_text'):
            b2[k][b, n:] = 0
        b2['user_title_mask'][b, n:] = False
        b2['user_title_mask'][b, n:, 0] = True
        b2['user_history_mask'][b, :n] = True
        b2['user_history_mask'][b, n:] = False
    return b2


@pytest.mark.parametrize('method', ['naive', 'group3'])
def test_compacted_equals_dense_bitwise(method, fused_pool, monkeypatch):
    over = dict(cnn_method='group3', cnn_kernel_num=300) if method == 'group3' else {}
    cfg = _full_cfg(**over)
    model = gpu_model(cfg, seed=37)
    model.use_graph = False
    batch = _with_history_fill(cfg, synth.make_batch(cfg, 32, 5, seed=38), lambda b: (3 * b) % (cfg.max_history_num + 1))
    for r in (3, 7):                                           # all-zero titles / bodies of live news (NAML reads no mask)
        batch['user_title_text'][r, 0] = 0
        batch['user_title_mask'][r, 0] = True
        batch['user_content_text'][r, 1] = 0
    batch['news_content_text'][5, 2] = 0
    monkeypatch.setattr(newsEncoders, 'DEDUP', True)
    got = run(model, batch)
    monkeypatch.setattr(newsEncoders, 'DEDUP', False)
    dense = run(model, batch)
    assert torch.isfinite(got).all() and torch.equal(got, dense), float((got - dense).abs().max())


def test_one_captured_graph_follows_the_padding_pattern(fused_pool, monkeypatch):
    cfg = _full_cfg()
    model = gpu_model(cfg, seed=61)
    H = cfg.max_history_num
    A = synth.make_batch(cfg, 32, 5, seed=62)
    batches = {'A': A, 'B': _with_history_fill(cfg, A, lambda b: H), 'C': _with_history_fill(cfg, A, lambda b: 1 if b % 8 == 0 else 0),
               'D': _with_history_fill(cfg, synth.make_batch(cfg, 32, 5, seed=63), lambda b: (7 * b) % (H + 1))}
    monkeypatch.setattr(newsEncoders, 'DEDUP', True)
    model.use_graph = True
    model._graphs.clear()
    got = {}
    for name in ('A', 'B', 'C', 'D', 'A'):
        got.setdefault(name, []).append(run(model, batches[name]))
    assert len(model._graphs) == 1
    assert torch.equal(got['A'][0], got['A'][1])
    model.use_graph = False
    for dedup in (True, False):
        monkeypatch.setattr(newsEncoders, 'DEDUP', dedup)
        for name in ('A', 'B', 'C', 'D'):
            want = run(model, batches[name])
            assert torch.equal(got[name][0], want), (name, dedup)
    model.use_graph = True


def test_training_step_is_bitwise_reproducible():
    cfg, batch, c = naml_cases.build_case('naml_naive')
    b = [v.cuda() for v in batch.values()]

    def train(steps=3):
        torch.manual_seed(0)
        model = gpu_model(cfg).train()
        step = TrainStep(model, lr=1e-5, gradient_clip_norm=4.0)
        losses = [float(step.step(*b)) for _ in range(steps)]
        return losses, {k: v.detach().clone() for k, v in model.state_dict().items()}

    l1, s1 = train()
    l2, s2 = train()
    assert all(math.isfinite(x) for x in l1) and l1 == l2
    assert all(torch.equal(s1[k], s2[k]) for k in s1)
    assert l1[0] != l1[-1]                                     # the steps did update the parameters


@pytest.mark.parametrize('method', ['naive', 'group3'])
def test_dropout_matches_torch_on_the_same_masks(method):
    """Training mode at dropout_rate 0.2: the four masks of naml_content (title / body word embeddings, title / body conv outputs) are
    read back through ops.dropout on all-ones tensors and fed to a torch fp64 statement of newsEncoders.py:671-695; forward and the
    gradients of every trained parameter of the encoder must match."""
    over = dict(cnn_method='group3', cnn_kernel_num=300) if method == 'group3' else {}
    cfg = make_config(content_encoder='NAML', vocabulary_size=3000, max_title_length=16, max_abstract_length=32, dropout_rate=0.2, **over)
    model = gpu_model(cfg, seed=71)
    enc = model.news_encoder.base_news_encoder.train()
    M, T, L, p = 48, cfg.max_title_length, cfg.max_abstract_length, 0.2
    tid = _ids(M, T, cfg.vocabulary_size, seed=72)
    bid = _ids(M, L, cfg.vocabulary_size, seed=76)
    mask = torch.ones(M, T, dtype=torch.bool)
    g = torch.Generator().manual_seed(73)
    cat = torch.randint(0, cfg.category_num, (M,), generator=g, dtype=torch.int32)
    sub = torch.randint(0, cfg.subCategory_num, (M,), generator=g, dtype=torch.int32)
    K = cfg.cnn_kernel_num
    G = rnd(M, K, seed=74)
    torch.manual_seed(5)
    out = TR.content_flat(enc, tid.cuda(), mask.cuda(), bid.cuda(), cat.cuda(), sub.cuda())
    (out * G.float().cuda()).sum().backward()
    torch.manual_seed(5)
    seed = TR._draw_seed()
    masks = [ops.dropout(torch.ones(r, c, device='cuda'), p, seed, site).cpu().double()
             for site, (r, c) in enumerate([(M * T, 300), (M * L, 300), (M * T, K), (M * L, K)])]
    assert 0.1 < float((masks[2] == 0).double().mean()) < 0.3
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in enc.named_parameters()}
    names = ['conv'] if method == 'naive' else ['conv1', 'conv2', 'conv3']

    def text(ids, S, conv, att, m_emb, m_conv):
        x = sd['word_embedding.weight'][ids.long().reshape(-1)] * m_emb
        c = torch.relu(torch.cat([ref_conv(x, sd['%s.%s.weight' % (conv, n)], sd['%s.%s.bias' % (conv, n)], S) for n in names], dim=1))
        c = c * m_conv
        h = torch.tanh(c @ sd[att + '.affine1.weight'].t() + sd[att + '.affine1.bias'])
        s = (h @ sd[att + '.affine2.weight'].t()).view(M, S)                                    # no mask (:686-687)
        return (torch.softmax(s, dim=1).unsqueeze(2) * c.view(M, S, K)).sum(dim=1)

    t_rep = text(tid, T, 'title_conv', 'title_attention', masks[0], masks[2])
    b_rep = text(bid, L, 'content_conv', 'content_attention', masks[1], masks[3])
    c_rep = torch.relu(sd['category_embedding.weight'][cat.long()] @ sd['category_affine.weight'].t() + sd['category_affine.bias'])
    s_rep = torch.relu(enc.subCategory_embedding.weight.detach().cpu().double()[sub.long()] @ sd['subCategory_affine.weight'].t()
                       + sd['subCategory_affine.bias'])
    feature = torch.stack([t_rep, b_rep, c_rep, s_rep], dim=1)
    alpha = torch.softmax(torch.tanh(feature @ sd['affine1.weight'].t() + sd['affine1.bias']) @ sd['affine2.weight'].t(), dim=1)
    want = (feature * alpha).sum(dim=1)
    assert rel_err(out.detach().cpu().numpy(), want.detach().numpy()) < TOL
    (want * G).sum().backward()
    named = dict(enc.named_parameters())
    for k, v in sd.items():
        if v.grad is None:
            assert named[k].grad is None or not named[k].requires_grad, k
            continue
        e = rel_err(named[k].grad.cpu().numpy(), v.grad.numpy())
        assert e < TOL, (k, e)


def test_scoring_and_training_forwards_agree(fused_pool):
    """The fused attention pools of encode_flat against the unfused training forward: within rounding, not bit for bit."""
    cfg, batch, c = naml_cases.build_case('naml_w5_body128')
    enc = gpu_model(cfg).news_encoder.base_news_encoder.eval()
    b = {k: v.cuda() for k, v in batch.items()}
    flat = newsEncoders._flat_inputs(b['news_title_text'], b['news_title_mask'], b['news_content_text'], b['news_category'],
                                     b['news_subCategory'])
    out = torch.empty((flat[0].shape[0], cfg.cnn_kernel_num), device='cuda')
    with torch.no_grad():
        enc.encode_flat(*flat, out)
        train = TR.content_flat(enc, *flat)
    assert rel_err(out.cpu().numpy(), train.cpu().numpy()) < 1e-5


def test_content_cache_agrees_with_the_uncached_forward(tmp_path, fused_pool):
    """util.compute_scores_cached (every news through NAML once, build_content_cache) against util.compute_scores on the toy corpus:
    the same rank file and metrics."""
    from lime_cikm25_amd import formats, util
    from lime_cikm25_amd.device_data import DeviceBehaviors, DeviceCorpus
    from helpers import GOLDEN_DIR
    g = json.load(open(os.path.join(GOLDEN_DIR, 'formats.json')))
    L = g['lines']
    cfg = make_config(content_encoder='NAML', max_history_num=g['max_history_num'], max_title_length=g['max_title_length'],
                      max_abstract_length=g['max_abstract_length'], vocabulary_size=len(g['word_dict']), negative_sample_num=2,
                      category_num=len(g['category_dict']) + 1, subCategory_num=len(g['subCategory_dict']) + 1,
                      user_num=len(g['user_ID_dict']), batch_size=16)
    corpus = formats.build_corpus(cfg, [L['train_news'], L['dev_news'], L['test_news']],
                                  [L['train_behaviors'], L['dev_behaviors'], L['test_behaviors']], g['news_ID_dict'],
                                  g['user_ID_dict'], g['category_dict'], g['subCategory_dict'], g['word_dict'], dataset='adressa')
    dev = DeviceBehaviors.from_devtest(DeviceCorpus(corpus), corpus, 'dev')
    torch.manual_seed(0)
    model = Model(cfg)
    model.initialize()
    torch.nn.init.normal_(model.news_encoder.base_news_encoder.word_embedding.weight, std=0.1)
    model = model.cuda()
    truth = tmp_path / 'truth.txt'
    with open(truth, 'w') as f:
        for i, labels in enumerate(formats.truth_labels(L['dev_behaviors'])):
            f.write('%d %s\n' % (i + 1, json.dumps(labels).replace(' ', '')))
    a = util.compute_scores(model, [dev.assemble(list(range(dev.num)))], corpus.dev_indices, str(tmp_path / 'rank.txt'), str(truth))
    b = util.compute_scores_cached(model, dev, corpus.dev_indices, str(tmp_path / 'rank_cached.txt'), str(truth), rows_per_forward=dev.num)
    assert open(tmp_path / 'rank_cached.txt').read() == open(tmp_path / 'rank.txt').read()
    assert a == b
