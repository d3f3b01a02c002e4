"""LIME-CNN-CROWN on the MI355X: the windowed conv kernels (csrc/conv_sp_f32.hip) against fp64 torch on the CPU, then the model
against the reference goldens (tests/golden/cnn_*.npz, grad_cnn_*.npz: tools/make_cnn_goldens.py), the compacted path against the
dense one and graph replay against eager (bitwise), a reproducible training step, training-mode dropout against a torch fp64 statement
fed with the kernels' masks, and the per-news content cache against the uncached forward."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_cases
from helpers import load_golden, rel_err
from lime_cikm25_amd import Model, make_config, newsEncoders, ops, synth
from lime_cikm25_amd import training as TR
from lime_cikm25_amd.training import TrainStep, negative_log_softmax

pytestmark = pytest.mark.gpu
TOL = 1e-3                      # the north star, as test_model_gpu.py
KTOL = 2e-5                     # kernel level: fp32-level products against fp64
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
        ids[s, lens[s]:] = 0                                   # padding word 0 inside the title
    ids[0] = 0                                                 # one all-padding sequence
    return ids.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [300, 84])
@pytest.mark.parametrize('T', [1, 7, 16, 32])
@pytest.mark.parametrize('win', [1, 3, 5])
@pytest.mark.parametrize('gather', [True, False])
def test_conv_window_against_fp64(C, T, win, gather):
    O, V, n = 200, 97, 37
    table = rnd(V, C, seed=1)
    table[0] = rnd(C, seed=2) + 2.0                            # word 0 is NOT zero: out-of-range taps must read zeros, not word 0
    w, b = rnd(O, C, win, seed=3, scale=0.2), rnd(O, seed=4)
    ids = _ids(n, T, V, seed=5 + T)
    x = table[ids.long()]
    want = torch.relu(ref_conv(x, w, b, T))
    wp = ops.conv1d_pack(w.float().cuda())
    if gather:
        got = ops.conv1d_window(table.float().cuda(), wp, win, T, ids=ids.cuda(), bias=b.float().cuda(), act='relu')
    else:
        got = ops.conv1d_window(x.float().cuda(), wp, win, T, bias=b.float().cuda(), act='relu')
    e = rel_err(got.cpu().numpy(), want.numpy())
    assert e < KTOL, e


def test_conv_window_row_count_and_column_slice():
    """m_dev below the allocated rows: rows beyond it are left untouched; the output is a column slice of a wider matrix, added into
    with accumulate."""
    C, T, win, O, V, n = 300, 16, 3, 100, 50, 40
    table = rnd(V, C, seed=11)
    w, b = rnd(O, C, win, seed=12, scale=0.2), rnd(O, seed=13)
    ids = _ids(n, T, V, seed=14)
    want = torch.relu(ref_conv(table[ids.long()], w, b, T))
    live = 23 * T
    big = torch.full((n * T, 3 * O), 7.0, device='cuda')
    m_dev = torch.tensor([live], dtype=torch.int32, device='cuda')
    ops.conv1d_window(table.float().cuda(), ops.conv1d_pack(w.float().cuda()), win, T, ids=ids.cuda(), bias=b.float().cuda(), act='relu',
                      out=big[:, O:2 * O], m_dev=m_dev)
    got = big.cpu()
    assert rel_err(got[:live, O:2 * O].numpy(), want[:live].numpy()) < KTOL
    assert torch.all(got[live:] == 7.0) and torch.all(got[:, :O] == 7.0) and torch.all(got[:, 2 * O:] == 7.0)
    ops.conv1d_window(table.float().cuda(), ops.conv1d_pack(w.float().cuda()), win, T, ids=ids.cuda(), out=big[:, O:2 * O], accumulate=True,
                      m_dev=m_dev)
    lin = ref_conv(table[ids.long()], w, None, T)
    got = big.cpu()
    assert rel_err(got[:live, O:2 * O].numpy(), (want[:live] + lin[:live]).numpy()) < KTOL
    assert torch.all(got[live:] == 7.0)


@pytest.mark.parametrize('C,O,T,win', [(300, 400, 32, 3), (84, 100, 7, 5), (300, 100, 16, 1), (120, 36, 1, 3)])
@pytest.mark.parametrize('gather', [True, False])
def test_conv_gradients_against_fp64_autograd(C, O, T, win, gather):
    V, n = 61, 29
    table = rnd(V, C, seed=21)
    table[0] = 1.5
    w = rnd(O, C, win, seed=22, scale=0.2).requires_grad_(True)
    ids = _ids(n, T, V, seed=23)
    x = table[ids.long()].clone().requires_grad_(True)
    dy = rnd(n * T, O, seed=24)
    (ref_conv(x, w, None, T) * dy).sum().backward()
    dyc = dy.float().cuda()
    dx = ops.conv1d_window(dyc, ops.conv1d_pack_dgrad(w.detach().float().cuda()), win, T)
    assert rel_err(dx.cpu().numpy(), x.grad.numpy()) < KTOL
    if gather:
        dw = ops.conv1d_window_wgrad(dyc, table.float().cuda(), win, T, ids=ids.cuda())
    else:
        dw = ops.conv1d_window_wgrad(dyc, x.detach().float().cuda(), win, T)
    got = dw.view(O, win, C).permute(0, 2, 1).cpu()
    assert rel_err(got.numpy(), w.grad.numpy()) < KTOL
    again = ops.conv1d_window_wgrad(dyc, x.detach().float().cuda(), win, T)
    assert torch.equal(again, ops.conv1d_window_wgrad(dyc, x.detach().float().cuda(), win, T))      # fixed summation order


def test_exact_fp32_mfma_form():
    """lime_set_split_gemm(0): the same kernels on the fp32 matrix cores."""
    C, T, win, O, V, n = 300, 16, 3, 128, 40, 20
    table = rnd(V, C, seed=31)
    w, b = rnd(O, C, win, seed=32, scale=0.2), rnd(O, seed=33)
    ids = _ids(n, T, V, seed=34)
    want = torch.relu(ref_conv(table[ids.long()], w, b, T))
    dy = rnd(n * T, O, seed=35)
    prev = ops.set_split_gemm(False)
    try:
        got = ops.conv1d_window(table.float().cuda(), ops.conv1d_pack(w.float().cuda()), win, T, ids=ids.cuda(), bias=b.float().cuda(),
                                act='relu')
        dw = ops.conv1d_window_wgrad(dy.float().cuda(), table.float().cuda(), win, T, ids=ids.cuda())
    finally:
        ops.set_split_gemm(prev)
    assert rel_err(got.cpu().numpy(), want.numpy()) < KTOL
    wr = w.clone().requires_grad_(True)
    (ref_conv(table[ids.long()], wr, None, T) * dy).sum().backward()
    assert rel_err(dw.view(O, win, C).permute(0, 2, 1).cpu().numpy(), wr.grad.numpy()) < KTOL


# The edges of the shared tile product (csrc/conv_frag.h conv_tile_product, its tap and [row0, row_end) arguments) as conv_sp_kernel
# drives it: 19 sequences of 7 tokens = 133 rows (the second 128-row tile holds 5 live rows), C = 36 (the second 32-deep chunk is
# masked past 4 columns), N = 132 (the second column block is 4 wide), without a device row count and with one of 126 (2 live rows
# short of the first tile, the second tile returns).
EDGE_T, EDGE_N_SEQ, EDGE_C, EDGE_O, EDGE_LIVE = 7, 19, 36, 132, 126


@functools.lru_cache(maxsize=None)
def edge_problem(win):
    """-> table, ids, x = table[ids], w, b, base (what the output holds before the launch), relu(conv) in fp64: computed once."""
    V = 41
    table = rnd(V, EDGE_C, seed=81)
    table[0] = rnd(EDGE_C, seed=82) + 2.0                      # word 0 is not zero
    w, b = rnd(EDGE_O, EDGE_C, win, seed=83, scale=0.3), rnd(EDGE_O, seed=84)
    ids = _ids(EDGE_N_SEQ, EDGE_T, V, seed=85)
    x = table[ids.long()]
    base = rnd(EDGE_N_SEQ * EDGE_T, EDGE_O + 8, seed=86).float()
    return table, ids, x, w, b, base, torch.relu(ref_conv(x, w, b, EDGE_T))


def run_edge_window(win, gather, accumulate, split, live):
    """The launch of test_conv_window_tile_edges -> the whole [133, 140] matrix whose columns 4 .. 135 are the output."""
    table, ids, x, w, b, base, _ = edge_problem(win)
    big = base.cuda()
    m_dev = None if live is None else torch.tensor([live], dtype=torch.int32, device='cuda')
    prev = ops.set_split_gemm(split)
    try:
        ops.conv1d_window((table if gather else x).float().cuda(), ops.conv1d_pack(w.float().cuda()), win, EDGE_T,
                          ids=ids.cuda() if gather else None, bias=b.float().cuda(), act='relu', out=big[:, 4:4 + EDGE_O],
                          accumulate=accumulate, m_dev=m_dev)
    finally:
        ops.set_split_gemm(prev)
    return big.cpu()


@pytest.mark.parametrize('split', [True, False])
@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('gather', [True, False])
@pytest.mark.parametrize('win', [3, 5])
def test_conv_window_tile_edges(win, gather, accumulate, split):
    base, want = edge_problem(win)[5:]
    cols = slice(4, 4 + EDGE_O)
    if accumulate:
        want = want + base[:, cols].double()
    for live in (None, EDGE_LIVE):
        got = run_edge_window(win, gather, accumulate, split, live)
        n = EDGE_N_SEQ * EDGE_T if live is None else live
        e = rel_err(got[:n, cols].numpy(), want[:n].numpy())
        print('win %d gather %d accumulate %d split %d live %s: %.2e' % (win, gather, accumulate, split, live, e))
        assert e < KTOL, e
        assert torch.equal(got[n:], base[n:])                  # the rows behind the count keep what they held
        assert torch.equal(got[:, :4], base[:, :4]) and torch.equal(got[:, 4 + EDGE_O:], base[:, 4 + EDGE_O:])


def run_edge_wgrad(split):
    """The launch of test_conv_wgrad_tile_edges: dW [8, 3 * 36] of 133 rows."""
    x = edge_problem(3)[2]
    dy = rnd(EDGE_N_SEQ * EDGE_T, 8, seed=87)
    prev = ops.set_split_gemm(split)
    try:
        return ops.conv1d_window_wgrad(dy.float().cuda(), x.float().cuda(), 3, EDGE_T), dy
    finally:
        ops.set_split_gemm(prev)


@pytest.mark.parametrize('split', [True, False])
def test_conv_wgrad_tile_edges(split):
    """133 rows are four whole 32-row chunks and one of 5; 8 outputs and 36 columns leave most of the 64 x 128 tile masked."""
    dw, dy = run_edge_wgrad(split)
    x = edge_problem(3)[2]
    w = torch.zeros(8, EDGE_C, 3, dtype=torch.float64, requires_grad=True)
    (ref_conv(x, w, None, EDGE_T) * dy).sum().backward()
    e = rel_err(dw.view(8, 3, EDGE_C).permute(0, 2, 1).cpu().numpy(), w.grad.numpy())
    assert e < KTOL, e
    assert torch.equal(run_edge_wgrad(split)[0], dw)           # fixed summation order


# ---------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------
def gpu_model(cfg, seed=cnn_cases.WEIGHT_SEED):
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


@pytest.mark.parametrize('name', list(cnn_cases.CASES))
def test_forward_matches_the_reference(name):
    cfg, batch, c = cnn_cases.build_case(name)
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


@pytest.mark.parametrize('name', cnn_cases.GRAD_CASES)
def test_gradients_match_the_reference(name):
    g = load_golden('grad_' + name)
    cfg, batch, c = cnn_cases.build_case(name)
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
    return make_config(content_encoder='CNN', vocabulary_size=50000, **over)


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
def test_compacted_equals_dense_bitwise(method, monkeypatch):
    over = dict(cnn_method='group3', cnn_kernel_num=300) if method == 'group3' else {}
    cfg = _full_cfg(**over)
    model = gpu_model(cfg, seed=37)
    model.use_graph = False
    batch = _with_history_fill(cfg, synth.make_batch(cfg, 32, 5, seed=38), lambda b: (3 * b) % (cfg.max_history_num + 1))
    for r in (3, 7):                                           # all-zero titles under a mask that is not the padding news' one
        batch['user_title_text'][r, 0] = 0
        batch['user_title_mask'][r, 0] = True
    monkeypatch.setattr(newsEncoders, 'DEDUP', True)
    got = run(model, batch)
    monkeypatch.setattr(newsEncoders, 'DEDUP', False)
    dense = run(model, batch)
    assert torch.isfinite(got).all() and torch.equal(got, dense), float((got - dense).abs().max())


def test_one_captured_graph_follows_the_padding_pattern(monkeypatch):
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
    cfg, batch, c = cnn_cases.build_case('cnn_naive')
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
    """Training mode at dropout_rate 0.2: the four masks of cnn_content (word embedding, conv output, category, subcategory) are read
    back through ops.dropout on all-ones tensors and fed to a torch fp64 statement of newsEncoders.py:548-563; forward and the gradients
    of every trained parameter of the encoder must match."""
    over = dict(cnn_method='group3', cnn_kernel_num=300) if method == 'group3' else {}
    cfg = make_config(content_encoder='CNN', vocabulary_size=3000, max_title_length=16, dropout_rate=0.2, **over)
    model = gpu_model(cfg, seed=71)
    enc = model.news_encoder.base_news_encoder.train()
    M, T, p = 48, cfg.max_title_length, 0.2
    ids = _ids(M, T, cfg.vocabulary_size, seed=72).view(M, T)
    mask = ids != 0
    mask[:, 0] = True
    g = torch.Generator().manual_seed(73)
    cat = torch.randint(0, cfg.category_num, (M,), generator=g, dtype=torch.int32)
    sub = torch.randint(0, cfg.subCategory_num, (M,), generator=g, dtype=torch.int32)
    K = cfg.cnn_kernel_num
    G = rnd(M, K + 100, seed=74)
    torch.manual_seed(5)
    out = TR.content_flat(enc, ids.cuda(), mask.cuda(), ids.cuda(), cat.cuda(), sub.cuda())
    (out * G.float().cuda()).sum().backward()
    torch.manual_seed(5)
    seed = TR._draw_seed()
    masks = [ops.dropout(torch.ones(r, c, device='cuda'), p, seed, site).cpu().double()
             for site, (r, c) in enumerate([(M * T, 300), (M * T, K), (M, 50), (M, 50)])]
    assert 0.1 < float((masks[1] == 0).double().mean()) < 0.3
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in enc.named_parameters()}
    x = sd['word_embedding.weight'][ids.long().reshape(-1)] * masks[0]
    convs = [('conv.conv', cfg.cnn_window_size)] if method == 'naive' else [('conv.conv1', 1), ('conv.conv2', 3), ('conv.conv3', 5)]
    c = torch.relu(torch.cat([ref_conv(x, sd[n + '.weight'], sd[n + '.bias'], T) for n, _ in convs], dim=1)) * masks[1]
    h = torch.tanh(c @ sd['attention.affine1.weight'].t() + sd['attention.affine1.bias'])
    s = (h @ sd['attention.affine2.weight'].t()).view(M, T).masked_fill(~mask, -1e9)
    rep = (torch.softmax(s, dim=1).unsqueeze(2) * c.view(M, T, K)).sum(dim=1)
    cat_e = sd['category_embedding.weight'][cat.long()] * masks[2]
    sub_e = enc.subCategory_embedding.weight.detach().cpu().double()[sub.long()] * masks[3]
    want = torch.cat([rep, cat_e, sub_e], dim=1)
    assert rel_err(out.detach().cpu().numpy(), want.detach().numpy()) < TOL
    (want * G).sum().backward()
    named = dict(enc.named_parameters())
    for k, v in sd.items():
        if v.grad is None:
            assert named[k].grad is None or not named[k].requires_grad, k
            continue
        e = rel_err(named[k].grad.cpu().numpy(), v.grad.numpy())
        assert e < TOL, (k, e)


def test_content_cache_agrees_with_the_uncached_forward(tmp_path):
    """util.compute_scores_cached (every news through the CNN once, build_content_cache) against util.compute_scores on the toy corpus:
    the same rank file and metrics."""
    from lime_cikm25_amd import formats, util
    from lime_cikm25_amd.device_data import DeviceBehaviors, DeviceCorpus
    from helpers import GOLDEN_DIR
    g = json.load(open(os.path.join(GOLDEN_DIR, 'formats.json')))
    L = g['lines']
    cfg = make_config(content_encoder='CNN', max_history_num=g['max_history_num'], max_title_length=g['max_title_length'],
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
