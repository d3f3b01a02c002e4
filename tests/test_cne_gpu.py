"""LIME-CNE-{CROWN,ATT} on the MI355X: the model against the reference goldens (tests/golden/cne_*.npz, grad_cne_*.npz:
tools/make_cne_goldens.py), graph replay against eager (bitwise), the scoring forward
against the training forward, training-mode dropout against a torch fp64 statement fed with the kernels' masks, a reproducible training
step, score_impressions against the eval forward, and the cached entry points against the uncached forward.  The LSTM step kernel
itself: tests/test_lstm_gpu.py."""
import json
import math
import os

import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import cne_cases
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


def gpu_model(cfg, seed=cne_cases.WEIGHT_SEED):
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


@pytest.mark.parametrize('name', list(cne_cases.CASES))
def test_forward_matches_the_reference(name):
    cfg, batch, c = cne_cases.build_case(name)
    g = load_golden(name)
    model = gpu_model(cfg)
    b = {k: v.cuda() for k, v in batch.items()}
    model.eval()
    if not c['eval_shape']:
        model.training = True
    with torch.no_grad():
        logits = model(*b.values()).cpu()
    for k in ('user_title_mask', 'user_content_mask', 'news_title_mask', 'news_content_mask'):
        assert torch.equal(b[k].cpu(), batch[k]), 'the mask-slot-0 rule must not edit the caller\'s tensors (%s)' % k
    assert logits.shape == g['logits'].shape
    e = rel_err(logits.numpy(), g['logits'])
    print('%s: logits vs reference golden %.2e' % (name, e))
    assert e < TOL
    if c['eval_shape']:
        return
    model.eval()
    ne, ue = model.news_encoder, model.user_encoder
    with torch.no_grad():
        cand_args = (b['news_title_text'], b['news_title_mask'], b['news_title_entity'], b['news_content_text'], b['news_content_mask'],
                     b['news_content_entity'], b['news_category'], b['news_subCategory'], None, b['news_freshness'], b['news_user_topic_lifetime'])
        hist_args = (b['user_title_text'], b['user_title_mask'], b['user_title_entity'], b['user_content_text'], b['user_content_mask'],
                     b['user_content_entity'], b['user_category'], b['user_subCategory'], None, b['user_freshness'], b['user_user_topic_lifetime'])
        cand = ne(*cand_args)
        content = ne.base_news_encoder(*cand_args)
        hist_content = ne.base_news_encoder(*hist_args)
        user = ue(b['user_title_text'], b['user_title_mask'], b['user_title_entity'], b['user_content_text'], b['user_content_mask'],
                  b['user_content_entity'], b['news_category'], b['news_subCategory'], b['user_category'], b['user_subCategory'],
                  b['user_history_mask'], b['user_history_graph'], b['user_history_category_mask'],
                  b['user_history_category_indices'], None, cand, b['user_freshness'], b['user_user_topic_lifetime'])
    errs = dict(news_representation=rel_err(cand.cpu().numpy(), g['news_representation']),
                cand_content=rel_err(content.cpu().numpy(), g['cand_content']),
                hist_content=rel_err(hist_content.cpu().numpy()[:HIST_ROWS], g['hist_content']),
                user_representation=rel_err(user.cpu().numpy(), g['user_representation']))
    print('%s: %s' % (name, ' '.join('%s %.2e' % kv for kv in errs.items())))
    assert max(errs.values()) < TOL


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


@pytest.mark.parametrize('name', cne_cases.GRAD_CASES)
def test_gradients_match_the_reference(name):
    g = load_golden('grad_' + name)
    cfg, batch, c = cne_cases.build_case(name)
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
    b2 = {k: v.clone() for k, v in batch.items()}
    for b in range(b2['user_history_mask'].shape[0]):
        n = fill(b)
        for k in ('user_category', 'user_subCategory', 'user_title_text', 'user_content_text'):
            b2[k][b, n:] = 0
        for k in ('user_title_mask', 'user_content_mask'):
            b2[k][b, n:] = False
            b2[k][b, n:, 0] = True
        b2['user_history_mask'][b, :n] = True
        b2['user_history_mask'][b, n:] = False
    return b2


def test_one_captured_graph_follows_the_padding_pattern():
    """CNE has no compacted form (a paired pass shares nothing): one captured graph follows the lengths and the pairing of four padding
    patterns through device-side lengths and sorts, and equals the eager forward bit for bit."""
    cfg = make_config(content_encoder='CNE', vocabulary_size=50000, hidden_dim=48, max_history_num=20, max_title_length=16,
                      max_abstract_length=32)
    model = gpu_model(cfg, seed=61)
    H = cfg.max_history_num
    A = synth.make_batch(cfg, 32, 5, seed=62)
    batches = {'A': A, 'B': _with_history_fill(cfg, A, lambda b: H), 'C': _with_history_fill(cfg, A, lambda b: 1 if b % 8 == 0 else 0),
               'D': _with_history_fill(cfg, synth.make_batch(cfg, 32, 5, seed=63), lambda b: (7 * b) % (H + 1))}
    model.use_graph = True
    model._graphs.clear()
    got = {}
    for name in ('A', 'B', 'C', 'D', 'A'):
        got.setdefault(name, []).append(run(model, batches[name]))
    assert len(model._graphs) == 1
    assert torch.equal(got['A'][0], got['A'][1])
    model.use_graph = False
    for name in ('A', 'B', 'C', 'D'):
        assert torch.equal(got[name][0], run(model, batches[name])), name
    model.use_graph = True


def _flat(b, side):
    M = b[side + '_title_text'].shape[0] * b[side + '_title_text'].shape[1]
    flat = newsEncoders._flat_inputs(b[side + '_title_text'], b[side + '_title_mask'], b[side + '_content_text'], b[side + '_category'],
                                     b[side + '_subCategory'])
    return flat, b[side + '_content_mask'].reshape(M, -1).contiguous()


@pytest.mark.parametrize('paired', [False, True], ids=['own_news', 'reference_pairs'])
@pytest.mark.parametrize('name', ['cne_body128', 'cne_h400_empty_history'])
def test_scoring_and_training_forwards_agree(name, paired):
    cfg, batch, c = cne_cases.build_case(name)
    enc = gpu_model(cfg).news_encoder.base_news_encoder.eval()
    b = {k: v.cuda() for k, v in batch.items()}
    flat, cmask = _flat(b, 'user')
    out = torch.empty((flat[0].shape[0], enc.news_embedding_dim), device='cuda')
    groups = [flat[0].shape[0]] if paired else None
    with torch.no_grad():
        enc.encode_flat(*flat, out, content_mask=cmask, pair_groups=groups)
        train = TR.content_flat(enc, *flat, content_mask=cmask, pair_groups=groups)
    e = rel_err(out.cpu().numpy(), train.cpu().numpy())
    print('%s: scoring vs training forward %.2e' % (name, e))
    assert e < 1e-5


def test_training_step_is_bitwise_reproducible():
    cfg, batch, c = cne_cases.build_case('cne_small')
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


def _texts(n, S, V, seed):
    """ids with the padding word behind a random length, and the prefix mask of that length; row 0 all padding (mask all zero: the
    slot-0 rule gives it length 1)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, V, (n, S), generator=g, dtype=torch.int32)
    lens = torch.randint(1, S + 1, (n,), generator=g)
    mask = torch.arange(S)[None, :] < lens[:, None]
    ids[~mask] = 0
    ids[0] = 0
    mask[0] = False
    return ids, mask


def test_dropout_matches_torch_on_the_same_masks():
    """Training mode at dropout_rate 0.2: the four masks of cne_content (title / body word embeddings, category / subcategory
    embeddings) are read back through ops.dropout on all-ones tensors and fed to a torch fp64 statement of newsEncoders.py:486-532
    (nn.LSTM under pack_padded_sequence); the forward and the gradients of every trained parameter of the encoder must match."""
    h = 32
    cfg = make_config(content_encoder='CNE', vocabulary_size=3000, max_title_length=8, max_abstract_length=16, hidden_dim=h, dropout_rate=0.2)
    model = gpu_model(cfg, seed=71)
    enc = model.news_encoder.base_news_encoder.train()
    M, T, L, p, A = 24, cfg.max_title_length, cfg.max_abstract_length, 0.2, cfg.attention_dim
    tid, tmask = _texts(M, T, cfg.vocabulary_size, seed=72)
    bid, bmask = _texts(M, L, cfg.vocabulary_size, seed=76)
    g = torch.Generator().manual_seed(73)
    cat = torch.randint(0, cfg.category_num, (M,), generator=g, dtype=torch.int32)
    sub = torch.randint(0, cfg.subCategory_num, (M,), generator=g, dtype=torch.int32)
    G = rnd(M, 4 * h + 100, seed=74)
    torch.manual_seed(5)
    out = TR.content_flat(enc, tid.cuda(), tmask.cuda(), bid.cuda(), cat.cuda(), sub.cuda(), content_mask=bmask.cuda(), pair_groups=[M])
    (out * G.float().cuda()).sum().backward()
    torch.manual_seed(5)
    seed = TR._draw_seed()
    masks = [ops.dropout(torch.ones(r, c, device='cuda'), p, seed, site).cpu().double()
             for site, (r, c) in enumerate([(M * T, 300), (M * L, 300), (M, 50), (M, 50)])]
    assert 0.1 < float((masks[0] == 0).double().mean()) < 0.3
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in enc.named_parameters()}

    def lstm64(name):
        m = torch.nn.LSTM(300, h, batch_first=True, bidirectional=True).double()
        m.load_state_dict({k[len(name) + 1:]: v.detach() for k, v in sd.items() if k.startswith(name + '.')})
        return m

    lstms = {'title_lstm': lstm64('title_lstm'), 'content_lstm': lstm64('content_lstm')}

    def recur(ids, mask, S, name, m_emb):
        mk = mask.clone()
        mk[:, 0] = True                                                                          # :492-493
        x = (sd['word_embedding.weight'][ids.long().reshape(-1)] * m_emb).view(M, S, -1)       # :501-502
        o, (_, c_n) = lstms[name](pack_padded_sequence(x, mk.sum(1), batch_first=True, enforce_sorted=False))
        hh, _ = pad_packed_sequence(o, batch_first=True, total_length=S)
        order = torch.sort(mk.sum(1), descending=True, stable=True).indices                     # :496-499, ties in input order
        return mk, hh, torch.cat([c_n[0], c_n[1]], dim=1), order, torch.sort(order).indices      # :512-515

    tk, th, tm, t_sort, t_desort = recur(tid, tmask, T, 'title_lstm', masks[0])
    bk, bh, bm, b_sort, b_desort = recur(bid, bmask, L, 'content_lstm', masks[1])
    # the gates act in SORTED order, each text in its own (:517-521): sorted position j of the titles meets sorted position j of the bodies
    th_s, bh_s, tm_s, bm_s = th[t_sort], bh[b_sort], tm[t_sort], bm[b_sort]
    tg = (th_s * torch.sigmoid(th_s @ sd['title_H.weight'].t() + (bm_s @ sd['title_M.weight'].t() + sd['title_M.bias']).unsqueeze(1)))[t_desort]
    bg = (bh_s * torch.sigmoid(bh_s @ sd['content_H.weight'].t() + (tm_s @ sd['content_M.weight'].t() + sd['content_M.bias']).unsqueeze(1)))[b_desort]

    def self_att(x, mk, name):
        s = (torch.tanh(x @ sd[name + '.affine1.weight'].t() + sd[name + '.affine1.bias']) @ sd[name + '.affine2.weight'].t()).squeeze(2)
        return (torch.softmax(s.masked_fill(~mk, -1e9), dim=1).unsqueeze(2) * x).sum(dim=1)

    def cross_att(x, query, mk, name):
        q = query @ sd[name + '.Q.weight'].t() + sd[name + '.Q.bias']
        a = torch.bmm(x @ sd[name + '.K.weight'].t(), q.unsqueeze(2)).squeeze(2) / math.sqrt(float(A))
        return (torch.softmax(a.masked_fill(~mk, -1e9), dim=1).unsqueeze(2) * x).sum(dim=1)

    ts, bs = self_att(tg, tk, 'title_self_attention'), self_att(bg, bk, 'content_self_attention')                                 # :524-525
    tc, bc = cross_att(tg, bs, tk, 'title_cross_attention'), cross_att(bg, ts, bk, 'content_cross_attention')                     # :527-528
    want = torch.cat([ts + tc, bs + bc, sd['category_embedding.weight'][cat.long()] * masks[2],
                      enc.subCategory_embedding.weight.detach().cpu().double()[sub.long()] * masks[3]], dim=1)
    e = rel_err(out.detach().cpu().numpy(), want.detach().numpy())
    print('dropout forward %.2e' % e)
    assert e < TOL
    (want * G).sum().backward()
    named = dict(enc.named_parameters())
    worst = ('', 0.0)
    for k, v in sd.items():
        ref = v.grad
        for name, m in lstms.items():
            if k.startswith(name + '.'):
                ref = dict(m.named_parameters())[k[len(name) + 1:]].grad
        if ref is None:
            assert named[k].grad is None or not named[k].requires_grad, k
            continue
        e = rel_err(named[k].grad.cpu().numpy(), ref.numpy())
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e < TOL, (k, e)
    print('dropout gradients: worst %s %.2e' % worst)


def test_score_impressions_equals_eval_forward_on_expanded_rows():
    """Under CNE nothing of a history can be shared between the K candidates of an impression (the gates' partners depend on the encoder
    call), so score_impressions evaluates the expanded rows themselves: the result is the eval forward's, bit for bit."""
    cfg = make_config(content_encoder='CNE', hidden_dim=48, max_history_num=10, max_title_length=16, max_abstract_length=32, batch_size=64,
                      vocabulary_size=5000)
    model = gpu_model(cfg, seed=41)
    B, K = 5, 6
    batch = synth.make_batch(cfg, B, K, seed=42)
    c = {k: v.cuda() for k, v in batch.items()}
    model.eval()
    args = (c['user_category'], c['user_subCategory'], c['user_title_text'], c['user_title_mask'], c['user_content_text'],
            c['user_freshness'], c['user_user_topic_lifetime'], c['user_history_mask'], c['news_category'], c['news_subCategory'],
            c['news_title_text'], c['news_title_mask'], c['news_content_text'], c['news_freshness'], c['news_user_topic_lifetime'],
            c['remaining_lifetime'])
    with pytest.raises(TypeError, match='body mask'):
        model.score_impressions(*args)
    masks = dict(user_content_mask=c['user_content_mask'], news_content_mask=c['news_content_mask'])
    got = model.score_impressions(*args, **masks)
    assert got.shape == (B, K)
    exp = type(batch)()
    for k, v in batch.items():
        exp[k] = v.reshape((B * K,) + tuple(v.shape[2:])) if (k.startswith('news_') or k == 'remaining_lifetime') else v.repeat_interleave(K, dim=0)
    model.use_graph = False
    ref_rows = run(model, exp, True)
    e = rel_err(got.cpu().reshape(-1).numpy(), ref_rows.reshape(-1).numpy())
    print('score_impressions vs expanded rows: %.2e' % e)
    assert e < 2e-5                                            # the bound of test_user_encoders_gpu.py (here the rows are the same: 0 expected)


def test_content_cache_agrees_with_the_uncached_forward(tmp_path):
    """util.compute_scores_cached against util.compute_scores on the toy corpus, over the SAME batch (rows_per_forward = all rows: CNE's
    scores depend on the batch): the same rank file and metrics.  Under CNE the cache is empty and the cached pass sends the rows' batch
    through the eval forward (Model.build_news_cache), so this checks that entry point's plumbing, not a cache."""
    from lime_cikm25_amd import formats, util
    from lime_cikm25_amd.device_data import DeviceBehaviors, DeviceCorpus
    from helpers import GOLDEN_DIR
    g = json.load(open(os.path.join(GOLDEN_DIR, 'formats.json')))
    L = g['lines']
    cfg = make_config(content_encoder='CNE', hidden_dim=48, max_history_num=g['max_history_num'], max_title_length=g['max_title_length'],
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
