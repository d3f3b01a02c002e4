"""The ATT and MHSA user encoders on the MI355X: the model against the reference goldens (tests/golden/user_*.npz, grad_user_*.npz:
tools/make_user_goldens.py) with the tail on the one-launch kernel and on the two existing launches, graph replay against eager
(bitwise), the encode-once scoring layout and the per-news cache against the plain forward, a reproducible training step, and the
training-mode dropouts of the MHSA user encoder against a torch fp64 statement fed with the kernels' masks.  The tail kernel itself:
tests/test_pool_match_gpu.py."""
import json
import math
import os

import pytest
import torch

import user_cases
from helpers import load_golden, rel_err
from test_naml_gpu import _with_history_fill, compare_grads, unique_named_parameters
from lime_cikm25_amd import Model, make_config, newsEncoders, ops, synth
from lime_cikm25_amd import training as TR
from lime_cikm25_amd.training import TrainStep, negative_log_softmax

pytestmark = pytest.mark.gpu
TOL = 1e-3                      # the project's parity bound against the reference, as test_model_gpu.py / test_naml_gpu.py
KTOL = 2e-5                     # fp32-level kernel against the same sums in another order, as tests/test_attn_pool_gpu.py
HIST_ROWS = 2                   # tools/make_user_goldens.py stores history-level taps for the first rows only
PAIRINGS = [('NAML', 'ATT'), ('MHSA', 'MHSA')]
KEY_BIAS = {'multiheadAttention.W_K.bias': 'multiheadAttention.W_Q.bias', 'candidate_aware_attn.key_proj.bias': 'candidate_aware_attn.query_proj.bias'}


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale


def gpu_model(cfg, seed=user_cases.WEIGHT_SEED):
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


@pytest.fixture(params=[True, False], ids=['fused', 'two_launch'])
def fused_tail(request, monkeypatch):
    """The pool + match + lifetime weight on lime_pool_match_f32 and on additive_pool + lifetime_score."""
    monkeypatch.setattr(ops, 'FUSED_POOL_MATCH', request.param)
    return request.param


@pytest.mark.parametrize('n_seq,S,nh,hd', [(5, 50, 10, 20), (3, 50, 20, 20), (4, 10, 20, 20)])
def test_masked_token_attention_at_history_shapes(n_seq, S, nh, hd):
    """ops.token_attention with a key mask at S = H (the self-attention of the MHSA user encoder: 50 slots, head_dim 20) against fp64;
    sequence 0 has every key masked (uniform weights, layers.py:231-233)."""
    tok, W = n_seq * S, nh * hd
    qkv = rnd(tok, 3 * W, seed=S + nh)
    g = torch.Generator().manual_seed(4)
    lens = torch.randint(1, S + 1, (n_seq,), generator=g)
    lens[0] = 0
    mask = torch.arange(S).unsqueeze(0) < lens.unsqueeze(1)
    q, k, v = (qkv[:, i * W:(i + 1) * W].reshape(n_seq, S, nh, hd).permute(0, 2, 1, 3) for i in range(3))
    a = (q @ k.transpose(-1, -2) / math.sqrt(hd)).masked_fill(mask.view(n_seq, 1, 1, S) == 0, -1e9)
    want = (torch.softmax(a, dim=-1) @ v).permute(0, 2, 1, 3).reshape(tok, W)
    d = qkv.float().cuda()
    got = ops.token_attention(d[:, :W], d[:, W:2 * W], d[:, 2 * W:], n_seq, S, nh, hd, 1.0 / math.sqrt(hd), key_mask=mask.reshape(-1).cuda())
    assert rel_err(got.cpu().numpy(), want.numpy()) < KTOL


def _user_side(model, b):
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
        taps = {}
        agg = ue.attention_weights(b['news_category'], b['news_subCategory'], b['user_category'], b['user_subCategory'], b['user_history_mask'])
        user2, logits = ue.match(hist, b['news_category'], b['news_subCategory'], b['user_category'], b['user_subCategory'],
                                 b['user_history_mask'], cand, remaining_lifetime=b['remaining_lifetime'].float(),
                                 weighting=model.remaining_lifetime_weighting, taps=taps)
    assert torch.equal(user, user2)
    return cand, user, agg, taps, logits


@pytest.mark.parametrize('name', list(user_cases.CASES))
def test_forward_matches_the_reference(name, fused_tail):
    cfg, batch, c = user_cases.build_case(name)
    g = load_golden(name)
    model = gpu_model(cfg)
    logits = run(model, batch, c['eval_shape'])                 # eval cases: the [rows] signature (model.py:158-169)
    assert logits.shape == g['logits'].shape
    e = rel_err(logits.numpy(), g['logits'])
    print('%s: logits vs reference golden %.2e' % (name, e))
    assert e < TOL
    model.eval()
    b = {k: v.cuda() for k, v in batch.items()}
    if c['eval_shape']:
        for k in list(b):
            if k.startswith('news_') or k == 'remaining_lifetime':
                b[k] = b[k].unsqueeze(1)
    cand, user, agg, taps, logits2 = _user_side(model, b)
    assert rel_err(logits2.cpu().numpy(), g['logits']) < TOL
    assert rel_err(cand.cpu().numpy(), g['news_representation']) < TOL
    assert tuple(user.shape) == g['user_representation'].shape
    assert rel_err(user.cpu().numpy(), g['user_representation']) < TOL
    if cfg.use_candidate_ware_clicked_news_attention:
        assert rel_err(agg.cpu().numpy(), g['attn_weights_agg']) < TOL
        assert rel_err(taps['hist_refined'][:HIST_ROWS].cpu().numpy(), g['hist_refined']) < TOL
    else:
        assert agg is None and 'attn_weights_agg' not in g
    if cfg.user_encoder == 'MHSA':
        assert rel_err(taps['self_attention'][:HIST_ROWS].cpu().numpy(), g['self_attention']) < TOL
        assert rel_err(taps['post_affine'][:HIST_ROWS].cpu().numpy(), g['post_affine']) < TOL


@pytest.mark.parametrize('name', list(user_cases.CASES))
def test_both_forms_of_the_tail_agree(name, monkeypatch):
    cfg, batch, c = user_cases.build_case(name)
    model = gpu_model(cfg)
    model.use_graph = False
    out = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, 'FUSED_POOL_MATCH', fused)
        out[fused] = run(model, batch, c['eval_shape'])
    assert rel_err(out[True].numpy(), out[False].numpy()) < KTOL


@pytest.mark.parametrize('name', user_cases.GRAD_CASES)
def test_gradients_match_the_reference(name):
    """Loss and every gradient the reference has within TOL by ``compare_grads``; every parameter it leaves at None has none.

    The tightest entry is ``user_encoder.multiheadAttention.W_K.bias``: that gradient is identically zero (a constant added to every
    key's score of a query leaves the softmax alone), the golden holds the reference's own rounding residue (up to 7.5e-9) and
    compare_grads' floor of 1e-5 makes its bound 1e-8 absolute.  training._MaskedAttention(center_keys=True) takes the kernel's
    common residue out of dK (2e-8 before, 9e-10 after, measured); tools/make_user_goldens.py refuses a golden whose reference
    residue alone reaches 1e-8, and prints how far the reference's fp32 gradients are from its own fp64 ones (tests/user_cases.py says
    where that decided a batch seed)."""
    g = load_golden('grad_' + name)
    cfg, batch, c = user_cases.build_case(name)
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


def _full_cfg(content, user, **over):
    return make_config(content_encoder=content, user_encoder=user, vocabulary_size=50000, **over)


@pytest.mark.parametrize('content,user', PAIRINGS)
def test_one_captured_graph_follows_the_padding_pattern(content, user, fused_tail, monkeypatch):
    """Graph replay equals eager bitwise, and ONE captured graph serves batches with different padding patterns (batch 32, history 50,
    K = 1 + 4, title 32, body 128)."""
    cfg = _full_cfg(content, user)
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
    for name in ('A', 'B', 'C', 'D'):
        want = run(model, batches[name])
        assert torch.isfinite(want).all() and torch.equal(got[name][0], want), name
    model.use_graph = True


@pytest.mark.parametrize('content,user', PAIRINGS + [('CROWN', 'ATT')])
@pytest.mark.parametrize('cand_aware', [True, False])
def test_score_impressions_equals_eval_forward_on_expanded_rows(content, user, cand_aware):
    """B impressions x K candidates with every history encoded once (hist_div = K) against the eval forward on the B * K expanded rows.
    Not bitwise: the two layouts give the encoder and gate GEMMs different row counts (B (K + H) news here, B K (1 + H) there), which
    the GEMM dispatcher may hand to kernels with another k order -- the bound is the kernel-level one.  Chunked passes are bitwise."""
    cfg = make_config(content_encoder=content, user_encoder=user, max_history_num=10, max_title_length=16, max_abstract_length=32,
                      batch_size=64, vocabulary_size=5000, use_candidate_ware_clicked_news_attention=cand_aware)
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
    again = model.score_impressions(*args, rows_per_pass=2 * K)
    assert torch.equal(again, got)


@pytest.mark.parametrize('content,user', PAIRINGS)
def test_content_cache_agrees_with_the_uncached_forward(content, user, tmp_path, fused_tail):
    """util.compute_scores_cached against util.compute_scores on the toy corpus: the same rank file and metrics."""
    from lime_cikm25_amd import formats, util
    from lime_cikm25_amd.device_data import DeviceBehaviors, DeviceCorpus
    from helpers import GOLDEN_DIR
    g = json.load(open(os.path.join(GOLDEN_DIR, 'formats.json')))
    L = g['lines']
    cfg = make_config(content_encoder=content, user_encoder=user, max_history_num=g['max_history_num'], max_title_length=g['max_title_length'],
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
    # no GraphSAGE node slots to bound the rows of a forward: twice the batch size is as legal as any other count
    b = util.compute_scores_cached(model, dev, corpus.dev_indices, str(tmp_path / 'rank_cached.txt'), str(truth), rows_per_forward=max(dev.num, 64))
    assert open(tmp_path / 'rank_cached.txt').read() == open(tmp_path / 'rank.txt').read()
    assert a == b


@pytest.mark.parametrize('name', ['user_att_naml', 'user_mhsa_mhsa'])
def test_training_step_is_bitwise_reproducible(name):
    cfg, batch, c = user_cases.build_case(name)
    b = [v.cuda() for v in batch.values()]

    def train(steps=3):
        torch.manual_seed(0)
        model = gpu_model(cfg).train()
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        step = TrainStep(model, lr=1e-5, gradient_clip_norm=4.0)
        assert 'news_encoder.category_affine.weight' not in step.names
        assert ('user_encoder.affine.weight' in step.names) == (cfg.user_encoder == 'MHSA')
        losses = [float(step.step(*b)) for _ in range(steps)]
        return losses, before, {k: v.detach().clone() for k, v in model.state_dict().items()}

    l1, s0, s1 = train()
    l2, _, s2 = train()
    assert all(math.isfinite(x) for x in l1) and l1 == l2
    assert all(torch.equal(s1[k], s2[k]) for k in s1)
    assert l1[0] != l1[-1]                                     # the steps did update the parameters
    assert torch.equal(s0['news_encoder.category_affine.weight'], s1['news_encoder.category_affine.weight'])
    assert not torch.equal(s0['user_encoder.attention.affine1.weight'], s1['user_encoder.attention.affine1.weight'])
    if cfg.user_encoder == 'MHSA':
        assert not torch.equal(s0['user_encoder.affine.weight'], s1['user_encoder.affine.weight'])


@pytest.mark.parametrize('cand_aware', [True, False])
def test_mhsa_user_dropout_matches_torch_on_the_same_masks(cand_aware):
    """Training mode: the p = 0.5 dropout behind ``affine`` (userEncoders.py:487, whatever config.dropout_rate says) and the p = 0.2
    dropout on the per-head probabilities of the candidate-aware layer (layers.py:36,74).  Both masks are read back through
    ops.dropout on all-ones tensors and fed to a torch fp64 statement of userEncoders.py:470-489; the user vector and the gradients
    of every parameter of the encoder must match."""
    cfg = make_config(content_encoder='MHSA', user_encoder='MHSA', vocabulary_size=3000, max_history_num=12, batch_size=8, dropout_rate=0.2,
                      use_candidate_ware_clicked_news_attention=cand_aware)
    model = gpu_model(cfg, seed=71)
    ue = model.user_encoder.train()
    ne = model.news_encoder
    B, N, H, D = 6, 3, cfg.max_history_num, ne.news_embedding_dim
    hist = rnd(B, H, D, seed=72)
    g = torch.Generator().manual_seed(73)
    cat = torch.randint(0, cfg.category_num, (B, N), generator=g, dtype=torch.int32)
    ucat = torch.randint(0, cfg.category_num, (B, H), generator=g, dtype=torch.int32)
    mask = torch.rand(B, H, generator=g) < 0.7
    mask[:, 0] = True
    mask[2] = False                                            # an empty history
    G = rnd(B, D, seed=74)
    hd_ = hist.float().cuda().requires_grad_(True)
    torch.manual_seed(5)
    out = TR.pooled_user(ue, hd_, cat.cuda(), ucat.cuda(), mask.cuda())
    (out * G.float().cuda()).sum().backward()
    torch.manual_seed(5)
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in ue.named_parameters() if not k.startswith('news_encoder.')}
    x = hist.clone().requires_grad_(True)
    xin = x
    if cand_aware:
        caa = ue.candidate_aware_attn
        nh, E = caa.num_heads, D
        seed_caa = TR._draw_seed()
        m_caa = ops.dropout(torch.ones(B * nh * N, H, device='cuda'), 0.2, seed_caa, 0).cpu().double().view(B, nh, N, H)
        table = ne.category_embedding.weight.detach().cpu().double()
        pre = 'candidate_aware_attn.'
        Q = (table[cat.long()] @ sd[pre + 'query_proj.weight'].t() + sd[pre + 'query_proj.bias']).view(B, N, nh, E // nh).transpose(1, 2)
        K = (table[ucat.long()] @ sd[pre + 'key_proj.weight'].t() + sd[pre + 'key_proj.bias']).view(B, H, nh, E // nh).transpose(1, 2)
        sc = ((Q @ K.transpose(-2, -1)) / (E ** 0.5)).masked_fill(mask.view(B, 1, 1, H) == 0, -1e9)
        a = torch.softmax(sc, dim=-1) * m_caa
        qw = torch.softmax(torch.norm(Q.transpose(1, 2).reshape(B, N, -1), dim=-1), dim=1)
        agg = torch.softmax((a.sum(dim=1) * qw.unsqueeze(-1)).sum(dim=1), dim=-1)                      # layers.py:66-81
        wx = agg.unsqueeze(-1) * x
        gate = torch.sigmoid(wx @ sd[pre + 'gate_proj.weight'].t() + sd[pre + 'gate_proj.bias'])
        xin = torch.nn.functional.layer_norm(gate * wx + (1 - gate) * x, (D,), sd[pre + 'layernorm.weight'], sd[pre + 'layernorm.bias'],
                                             caa.layernorm.eps)                                        # layers.py:83-91
    seed = TR._draw_seed()
    m_aff = ops.dropout(torch.ones(B * H, D, device='cuda'), 0.5, seed, 0).cpu().double().view(B, H, D)
    assert 0.4 < float((m_aff == 0).double().mean()) < 0.6
    mha = ue.multiheadAttention
    heads = lambda n: (xin @ sd['multiheadAttention.%s.weight' % n].t() + sd['multiheadAttention.%s.bias' % n]).view(B, H, mha.h, mha.d_k).transpose(1, 2)
    a = (heads('W_Q') @ heads('W_K').transpose(-1, -2) / math.sqrt(mha.d_k)).masked_fill(mask.view(B, 1, 1, H) == 0, -1e9)
    c = (torch.softmax(a, dim=-1) @ heads('W_V')).transpose(1, 2).reshape(B, H, mha.h * mha.d_k)      # layers.py:222-238
    h = torch.relu((c @ sd['affine.weight'].t() + sd['affine.bias']) * m_aff)                         # :487
    s = torch.tanh(h @ sd['attention.affine1.weight'].t() + sd['attention.affine1.bias']) @ sd['attention.affine2.weight'].t()
    want = (torch.softmax(s, dim=1) * h).sum(dim=1)                                                    # :489, no mask
    e = rel_err(out.detach().cpu().numpy(), want.detach().numpy())
    print('user vector under dropout: %.2e' % e)
    assert e < TOL
    (want * G).sum().backward()
    assert rel_err(hd_.grad.cpu().numpy(), x.grad.numpy()) < TOL
    named = dict(ue.named_parameters())
    for k, v in sd.items():
        if v.grad is None:
            assert named[k].grad is None, k
            continue
        floor = None
        if k in KEY_BIAS:
            # the gradient of a key bias is identically zero (a constant added to every key's score of a query leaves the softmax
            # alone): the fp64 statement holds 1e-17 rounding noise, which is no scale to measure against.  The sums that cancel are
            # those of the query bias beside it (same shape, same path, no cancellation), so the error is judged against that
            # gradient's magnitude
            floor = float(sd[KEY_BIAS[k]].grad.abs().mean())
        e = rel_err(named[k].grad.cpu().numpy(), v.grad.numpy(), floor=floor)
        assert e < TOL, (k, e)
