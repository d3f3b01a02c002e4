"""CNE's per-news recurrence cache on the MI355X: the two row movers of csrc/seq_cache_f32.hip alone (ops.seq_pack against torch
indexing, ops.cne_gate_cached against an fp64 torch statement), the encoder from the cache against the reference goldens
(tests/golden/cne_*.npz), cached against uncached scores on the toy corpus of tests/golden/formats.json, the bounded-sort pairing
against the per-call loop it replaced, and the refusal of a cache that is older than the weights."""
import functools
import json
import os

import pytest
import torch

import cne_cases
from helpers import GOLDEN_DIR, load_golden, rel_err
from lime_cikm25_amd import Model, _lib, formats, make_config, newsEncoders, ops, synth, util
from lime_cikm25_amd.device_data import DeviceBehaviors, DeviceCorpus
from lime_cikm25_amd.training import TrainStep

pytestmark = pytest.mark.gpu
TOL = 1e-3                      # the project's kernel tolerance (test_lstm_gpu.py) and the north star (test_cne_gpu.py)
ROUTES = 2e-5                   # two fp32 routes to one function (test_cne_gpu.py:339, test_user_encoders_gpu.py)
HIST_ROWS = 2                   # the goldens store history-level taps for the first rows only
N_NEWS, CAP, LIVE = 7, 9, 6     # news of the kernel tests' cache; batch slots and how many of them are live
SENTINEL = -7.5


@functools.lru_cache(maxsize=None)
def packed_problem(C, S):
    """A dense [n S, C] pair (h, hh), lengths that include 1 and S, and the rows torch selects from them: computed once per shape,
    shared by the kernel tests, never modified."""
    g = torch.Generator().manual_seed(100 * C + S)
    lens = torch.randint(1, S + 1, (N_NEWS,), generator=g)
    lens[0], lens[-1] = 1, S
    offsets = torch.zeros(N_NEWS + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(lens, 0)
    h = torch.rand(N_NEWS * S, C, generator=g) * 2 - 1
    hh = (torch.rand(N_NEWS * S, C, generator=g) * 2 - 1) * 3
    live = (torch.arange(S)[None, :] < lens[:, None]).reshape(-1)
    return dict(lens=lens, offsets=offsets, h=h, hh=hh, live=live, h_packed=h[live], hh_packed=hh[live])


@pytest.mark.parametrize('S', [1, 5, 32])
@pytest.mark.parametrize('C', [32, 96])
def test_pack_moves_the_live_rows_and_nothing_else(C, S):
    p = packed_problem(C, S)
    rows = int(p['offsets'][-1])
    dst = torch.full((rows + 1, C), SENTINEL, device='cuda')                   # one guard row behind sum(lens)
    ops.seq_pack(p['h'].cuda(), p['lens'].int().cuda(), p['offsets'].cuda(), dst, S)
    torch.cuda.synchronize()
    assert torch.equal(dst[:rows].cpu(), p['h_packed'])
    assert bool((dst[rows] == SENTINEL).all()), 'the guard row behind sum(lens) was written'


@pytest.mark.parametrize('S', [1, 5, 32])
@pytest.mark.parametrize('C', [32, 96])
def test_gate_matches_fp64_and_leaves_dead_slots_alone(C, S):
    p = packed_problem(C, S)
    g = torch.Generator().manual_seed(7 * C + S)
    idx = torch.tensor([3, 0, 3, N_NEWS - 1, 5, 1, 2, 4, 6], dtype=torch.int32)       # a repeated news, the last news of the cache
    tm = torch.rand(CAP, C, generator=g) * 2 - 1
    args = (p['h_packed'].cuda(), p['hh_packed'].cuda(), p['offsets'].cuda(), p['lens'].int().cuda(), idx.cuda(), tm.cuda(), S)
    n_dev = torch.tensor([LIVE], dtype=torch.int32, device='cuda')
    outs = []
    for _ in range(2):
        out = torch.full((CAP * S, C), SENTINEL, device='cuda')
        ops.cne_gate_cached(*args, out=out, n_rows_dev=n_dev)
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1]), 'two runs differ'
    got = outs[0].view(CAP, S, C)
    h64, hh64 = p['h'].double().view(N_NEWS, S, C), p['hh'].double().view(N_NEWS, S, C)
    j = idx[:LIVE].long()
    live = torch.arange(S)[None, :] < p['lens'][j][:, None]                     # [LIVE, S]
    want = h64[j] * torch.sigmoid(hh64[j] + tm[:LIVE].double()[:, None, :]) * live[:, :, None]
    e = rel_err(got[:LIVE].numpy(), want.numpy())
    print('gate C=%d S=%d: rel err vs fp64 %.2e' % (C, S, e))
    assert e < TOL
    assert bool((got[:LIVE][~live] == 0).all()), 'slots behind the length must be exact zeros'
    assert bool((got[LIVE:] == SENTINEL).all()), 'slots >= n_rows_dev were written'


def test_arguments_are_checked_before_any_launch():
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device='cuda')
    lens, offs, idx = torch.ones(2, dtype=torch.int32, device='cuda'), z(3, dt=torch.int64), z(2, dt=torch.int32)
    with pytest.raises(ValueError, match='multiple of 4'):
        ops.seq_pack(z(8, 6), lens, offs, z(2, 6), 4)
    with pytest.raises(ValueError, match='multiple of 4'):
        ops.cne_gate_cached(z(2, 6), z(2, 6), offs, lens, idx, z(2, 6), 4)
    with pytest.raises(ValueError, match='S must be'):
        ops.seq_pack(z(8, 8), lens, offs, z(2, 8), 0)
    with pytest.raises(ValueError, match='S must be'):
        ops.cne_gate_cached(z(2, 8), z(2, 8), offs, lens, idx, z(2, 8), 0)
    # the C entry points themselves: NULL, C = 6 and S = 0 are refused with a status, nothing is launched
    lib = _lib.load()
    P = lambda t: t.data_ptr()
    a, o = z(8, 8), z(8, 8)
    assert lib.lime_seq_pack_f32(None, P(lens), P(offs), P(o), 2, 4, 8, None) == -1 and b'NULL' in lib.lime_last_error_string()
    assert lib.lime_seq_pack_f32(P(a), P(lens), P(offs), P(o), 2, 4, 6, None) == -1
    assert lib.lime_seq_pack_f32(P(a), P(lens), P(offs), P(o), 2, 0, 8, None) == -1
    assert lib.lime_cne_gate_cached_f32(P(a), P(a), P(offs), P(lens), P(idx), None, P(o), 2, 4, 8, None, None) == -1
    assert b'NULL' in lib.lime_last_error_string()
    assert lib.lime_cne_gate_cached_f32(P(a), P(a), P(offs), P(lens), P(idx), P(a), P(o), 2, 4, 6, None, None) == -1
    assert lib.lime_cne_gate_cached_f32(P(a), P(a), P(offs), P(lens), P(idx), P(a), P(o), 2, 0, 8, None, None) == -1
    assert lib.lime_cne_gate_cached_f32(P(a), P(a), P(offs), P(lens), P(idx), P(a), P(o), -1, 4, 8, None, None) == -1
    assert lib.lime_cne_gate_cached_f32(P(a), P(a), P(offs), P(lens), P(idx), P(a), P(o), 0, 4, 8, None, None) == 0      # cap = 0: nothing to do
    assert lib.lime_seq_pack_f32(P(a), P(lens), P(offs), P(o), 0, 4, 8, None) == 0
    torch.cuda.synchronize()
    assert bool((o == 0).all())


def gpu_model(cfg, seed=cne_cases.WEIGHT_SEED):
    m = Model(cfg)
    m.initialize()
    synth.fill_state_dict(m, seed)
    return m.cuda()


@pytest.mark.parametrize('name', [n for n, c in cne_cases.CASES.items() if not c['eval_shape']])
def test_encoder_from_the_cache_matches_the_reference(name):
    """The case's candidate and history news as one corpus (idx = arange), the cache over them, one cached pass with the pair_groups the
    model passes (candidates, history) against the golden content taps."""
    cfg, batch, c = cne_cases.build_case(name)
    g = load_golden(name)
    enc = gpu_model(cfg).news_encoder.base_news_encoder.eval()
    b = {k: v.cuda() for k, v in batch.items()}
    B, N, H = b['news_title_text'].shape[0], b['news_title_text'].shape[1], b['user_title_text'].shape[1]
    flat = lambda k: torch.cat([b['news_' + k].reshape((B * N,) + tuple(b['news_' + k].shape[2:])),
                                b['user_' + k].reshape((B * H,) + tuple(b['user_' + k].shape[2:]))])
    M = B * N + B * H
    with torch.no_grad():
        cache = enc.build_recurrence_cache(flat('title_text'), flat('title_mask'), flat('content_text'), flat('content_mask'), news_per_pass=5)
        out = torch.empty((M, enc.news_embedding_dim), device='cuda')
        enc.encode_cached_flat(cache, torch.arange(M, dtype=torch.int32, device='cuda'), flat('title_mask'), flat('content_mask'),
                               flat('category').int().contiguous(), flat('subCategory').int().contiguous(), out, pair_groups=[B * N, B * H])
    torch.cuda.synchronize()
    lens_t, lens_b = cache.title.lens.cpu().tolist(), cache.body.lens.cpu().tolist()
    assert cache.nbytes == newsEncoders.CNERecurrenceCache.packed_nbytes(lens_t, lens_b, cfg.hidden_dim)
    errs = dict(cand_content=rel_err(out[:B * N].view(B, N, -1).cpu().numpy(), g['cand_content']),
                hist_content=rel_err(out[B * N:].view(B, H, -1).cpu().numpy()[:HIST_ROWS], g['hist_content']))
    print('%s from the cache: %s' % (name, ' '.join('%s %.2e' % kv for kv in errs.items())))
    assert max(errs.values()) < TOL


def loop_pairs(lens_t, lens_b, groups, cap):
    """CNE.reference_pairs as it was before the bounded-sort form: two sorts per call."""
    dev = lens_t.device
    pt, pb = torch.arange(cap, device=dev), torch.arange(cap, device=dev)
    o = 0
    for n in groups:
        st = torch.sort(lens_t[o:o + n], descending=True, stable=True).indices
        sc = torch.sort(lens_b[o:o + n], descending=True, stable=True).indices
        pt[o + st] = sc + o
        pb[o + sc] = st + o
        o += n
    return pt.to(torch.int32), pb.to(torch.int32)


def test_bounded_sort_pairs_equal_the_loop():
    groups = [3, 30, 3, 30, 2, 20]
    cap = sum(groups) + 4                                                       # four slots behind the groups: they pair with themselves
    g = torch.Generator().manual_seed(9)
    lens_t = torch.randint(1, 4, (cap,), generator=g, dtype=torch.int32).cuda()      # many tied lengths
    lens_b = torch.randint(1, 6, (cap,), generator=g, dtype=torch.int32).cuda()
    want = loop_pairs(lens_t, lens_b, groups, cap)
    got = newsEncoders.CNE.reference_pairs(lens_t, lens_b, groups, cap)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(want[0].cpu(), torch.arange(cap, dtype=torch.int32))      # the case does pair across news
    calls = torch.repeat_interleave(torch.arange(len(groups)), torch.tensor(groups)).cuda()
    got = newsEncoders.CNE.reference_pairs(lens_t, lens_b, calls, cap)                # the same calls as per-news call numbers
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def build_toy():
    """The toy corpus of tests/golden/formats.json under LIME-CNE-CROWN at hidden_dim 48 (test_cne_gpu.py's cached-route test): model, dev
    split, both caches."""
    g = json.load(open(os.path.join(GOLDEN_DIR, 'formats.json')))
    L = g['lines']
    cfg = make_config(content_encoder='CNE', hidden_dim=48, max_history_num=g['max_history_num'], max_title_length=g['max_title_length'],
                      max_abstract_length=g['max_abstract_length'], vocabulary_size=len(g['word_dict']), negative_sample_num=2,
                      category_num=len(g['category_dict']) + 1, subCategory_num=len(g['subCategory_dict']) + 1,
                      user_num=len(g['user_ID_dict']), batch_size=16)
    corpus = formats.build_corpus(cfg, [L['train_news'], L['dev_news'], L['test_news']],
                                  [L['train_behaviors'], L['dev_behaviors'], L['test_behaviors']], g['news_ID_dict'],
                                  g['user_ID_dict'], g['category_dict'], g['subCategory_dict'], g['word_dict'], dataset='adressa')
    dc = DeviceCorpus(corpus)
    dev = DeviceBehaviors.from_devtest(dc, corpus, 'dev')
    torch.manual_seed(0)
    model = Model(cfg)
    model.initialize()
    torch.nn.init.normal_(model.news_encoder.base_news_encoder.word_embedding.weight, std=0.1)
    model = model.cuda().eval()
    keys = list(model.state_dict())
    rc = model.build_recurrence_cache(dc)
    assert list(model.state_dict()) == keys, 'the cache must be a plain object, not a buffer or parameter'
    return dict(cfg=cfg, corpus=corpus, dc=dc, dev=dev, model=model, rc=rc, cache=model.build_news_cache(dc),
                labels=formats.truth_labels(L['dev_behaviors']))


@pytest.fixture(scope='module')
def toy():
    """One model and its caches for the tests that only read them."""
    return build_toy()


def test_cached_scores_equal_uncached_scores(toy):
    model, dev, rc, cache = toy['model'], toy['dev'], toy['rc'], toy['cache']
    rows = list(range(dev.num))
    assert dev.num == 20
    one = model.score_behaviors(dev, rows, cache).cpu()
    got = model.score_behaviors(dev, rows, cache, recurrence_cache=rc).cpu()
    e1 = rel_err(got.numpy(), one.numpy())
    per4 = torch.cat([model.score_behaviors(dev, rows[r:r + 4], cache) for r in range(0, dev.num, 4)]).cpu()
    got4 = model.score_behaviors(dev, rows, cache, recurrence_cache=rc, rows_per_forward=4).cpu()
    e4 = rel_err(got4.numpy(), per4.numpy())
    got6 = model.score_behaviors(dev, rows, cache, recurrence_cache=rc, rows_per_forward=6).cpu()        # a short last chunk (2 rows)
    per6 = torch.cat([model.score_behaviors(dev, rows[r:r + 6], cache) for r in range(0, dev.num, 6)]).cpu()
    e6 = rel_err(got6.numpy(), per6.numpy())
    print('cached vs uncached scores: one forward %.2e, four-row forwards %.2e, six-row forwards %.2e' % (e1, e4, e6))
    assert rel_err(per4.numpy(), one.numpy()) > 1e-4, 'the chunking must matter for the comparison to mean anything'
    assert e1 < ROUTES and e4 < ROUTES and e6 < ROUTES


def test_cached_dev_pass_gives_the_uncached_metrics(toy, tmp_path):
    model, dev, corpus = toy['model'], toy['dev'], toy['corpus']
    truth = tmp_path / 'truth.txt'
    formats.write_truth_file(str(truth), toy['labels'])
    a = util.compute_scores_cached(model, dev, corpus.dev_indices, str(tmp_path / 'rank.txt'), str(truth), rows_per_forward=4)
    b = util.compute_scores_cached(model, dev, corpus.dev_indices, str(tmp_path / 'rank_rc.txt'), str(truth), rows_per_forward=4,
                                   recurrence_cache=True)
    c = util.evaluate_cached_on_device(model, dev, corpus.dev_indices, toy['labels'], rows_per_forward=4, rows_per_pass=8,
                                       recurrence_cache=True)
    print('metrics uncached %s, cached %s, cached on the device %s' % (a, b, tuple(c)))
    assert all(abs(x - y) <= 1e-3 for x, y in zip(a, b))                       # README: metrics agree within +-0.001
    assert all(abs(x - float(y)) <= 1e-3 for x, y in zip(a, c))


def test_a_news_in_two_chunks_gets_each_chunks_partner(toy):
    """The content of a news depends on the chunk it is encoded in (its gates' partner is another news of the same reference call): in
    one cached pass over chunks of four rows the same news comes out with two contents, each that of the uncached encoder over
    that chunk alone."""
    model, dev, rc, dc = toy['model'], toy['dev'], toy['rc'], toy['dc']
    enc = model.news_encoder.base_news_encoder
    R, H, p = dev.num, dev.hist_index.shape[1], 4
    idx = torch.cat([dev.cand_index.reshape(-1), dev.hist_index.reshape(-1)])
    chunk = torch.arange(R, device='cuda') // p
    calls = torch.cat([2 * chunk, 2 * chunk.repeat_interleave(H) + 1])
    fields = lambda ix: (dc.news_title_mask[ix.long()], dc.news_abstract_mask[ix.long()], dc.news_category[ix.long()].int().contiguous(),
                         dc.news_subCategory[ix.long()].int().contiguous())
    with torch.no_grad():
        tm, am, cat, sub = fields(idx)
        got = enc.encode_cached_flat(rc, idx, tm, am, cat, sub, torch.empty((idx.numel(), enc.news_embedding_dim), device='cuda'),
                                     pair_groups=calls)
        want = torch.empty_like(got)
        for r0 in range(0, R, p):
            sel = torch.cat([torch.arange(r0, r0 + p), R + torch.arange(r0 * H, (r0 + p) * H)]).cuda()
            tm, am, cat, sub = fields(idx[sel])
            want[sel] = enc.encode_flat(dc.news_title_text[idx[sel].long()], tm, dc.news_abstract_text[idx[sel].long()], cat, sub,
                                        torch.empty((sel.numel(), enc.news_embedding_dim), device='cuda'), content_mask=am,
                                        pair_groups=[p, p * H])
    torch.cuda.synchronize()
    got, want, idx, calls = got.cpu(), want.cpu(), idx.cpu(), calls.cpu()
    e = rel_err(got.numpy(), want.numpy())
    scale = float(want.abs().mean())
    twice = [(int(q1), int(q2)) for j in idx.unique() for q in [torch.nonzero(idx == j).reshape(-1)] for q1 in q for q2 in q
             if calls[q1] // 2 != calls[q2] // 2 and float((want[q1] - want[q2]).abs().max()) > 0.01 * scale]
    print('cached vs uncached contents per chunk %.2e; %d (position, position) pairs of one news with two contents' % (e, len(twice)))
    assert twice, 'no news with two different contents: the rows do not exercise the per-chunk pairing'
    assert e < ROUTES
    q1, q2 = twice[0]
    assert float((got[q1] - got[q2]).abs().max()) > 0.01 * scale


def test_a_cache_older_than_the_weights_is_refused():
    toy = build_toy()                                                           # a model of its own: the test changes the weights
    model, dev, dc, cache = toy['model'], toy['dev'], toy['dc'], toy['cache']
    rows = list(range(8))
    keys = list(model.state_dict())
    rc = model.build_recurrence_cache(dc)
    assert list(model.state_dict()) == keys
    want = model.score_behaviors(dev, rows, cache, recurrence_cache=rc)
    enc = model.news_encoder.base_news_encoder
    enc.title_H.weight.data.add_(0.01)
    with pytest.raises(RuntimeError, match='rebuild'):
        model.score_behaviors(dev, rows, cache, recurrence_cache=rc)
    enc.title_H.weight.data.sub_(0.01)
    rc = model.build_recurrence_cache(dc)
    assert rel_err(model.score_behaviors(dev, rows, cache, recurrence_cache=rc).cpu().numpy(), want.cpu().numpy()) < ROUTES
    # an optimizer step (the native Adam writes the flat parameter bucket directly)
    train = synth.make_batch(toy['cfg'], 4, 3, seed=5)
    step = TrainStep(model.train(), lr=1e-3)
    model.eval()
    model.score_behaviors(dev, rows, cache, recurrence_cache=rc)                # re-pointing the parameters changes no value
    model.train()
    step.step(*[v.cuda() for v in train.values()])
    model.eval()
    with pytest.raises(RuntimeError, match='rebuild'):
        model.score_behaviors(dev, rows, cache, recurrence_cache=rc)
    model.score_behaviors(dev, rows, cache, recurrence_cache=model.build_recurrence_cache(dc))
