"""Measurements of the KCNN content encoder on one MI355X (the numbers behind DESIGN.md's "KCNN content encoder").  Prints one JSON line.

    python tools/bench_kcnn.py [--part all|kernel|score|train] [--rounds R] [--inner I] [--warmup W]

Every comparison is interleaved: a round times ``inner`` back-to-back calls of each candidate in turn (HIP events around them), and the
figure reported is the MEDIAN over the rounds of the per-call time, with the spread (min .. max) beside it -- so a drift of the clocks or a
neighbour on the machine hits both candidates of a pair alike.

kernel  ops.conv_pool fused (lime_conv_pool_f32, one launch) and unfused (conv1d_window per source + relu_maxpool) on the scoring shape
        (1760 news x 32 tokens, three sources of 300 columns -> 400, window 3: word rows gathered by id, the two entity sources gathered
        from [entity_size, 300] tables) and on one 8192-news pass of the content cache; algorithmic TFLOP/s = 2 M N (3 window C) / t.
score   graph-replayed scoring ms of LIME-KCNN-CROWN (both forms of conv_pool) next to LIME-CNN-CROWN at batch 32, history 50, K = 1 + 4,
        title 32, eval mode.
train   one TrainStep (forward + backward + clip + Adam) of LIME-KCNN-CROWN next to LIME-CNN-CROWN at the same batch, dropout_rate 0.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lime_cikm25_amd import Model, make_config, ops, synth  # noqa: E402
from lime_cikm25_amd.training import TrainStep  # noqa: E402

ENTITY_SIZE = 30000


def interleaved(fns, rounds, inner, warmup):
    """{name: (median ms, min ms, max ms)} per call of each fn, the candidates taking turns within every round."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / inner)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def _report(res, prefix, stats, flop=None):
    for k, (med, lo, hi) in stats.items():
        res['%s_%s_ms' % (prefix, k)] = round(med, 5)
        res['%s_%s_ms_range' % (prefix, k)] = [round(lo, 5), round(hi, 5)]
        if flop:
            res['%s_%s_tflops' % (prefix, k)] = round(flop / med / 1e9, 2)


def bench_kernel(rounds, inner, warmup):
    res = {}
    T, C, O, win, pad, V = 32, 300, 400, 3, 1, 50000
    g = torch.Generator().manual_seed(1)
    word = (torch.rand(V, C, generator=g) * 2 - 1).cuda()
    ent_t = torch.tanh(torch.rand(ENTITY_SIZE, C, generator=g) * 2 - 1).cuda()
    ctx_t = torch.tanh(torch.rand(ENTITY_SIZE, C, generator=g) * 2 - 1).cuda()
    w = ((torch.rand(O, C, win, 3, generator=g) * 2 - 1) * 0.05).cuda()
    b = (torch.rand(O, generator=g) - 0.5).cuda()
    wp = ops.conv_pool_pack(w)
    for label, n in (('score_1760', 1760), ('cache_8192', 8192)):
        ids = torch.randint(0, V, (n * T,), generator=g, dtype=torch.int32).cuda()
        ent = (torch.randint(1, ENTITY_SIZE, (n * T,), generator=g) * (torch.rand(n * T, generator=g) < 0.25)).int().cuda()
        src = [(word, ids), (ent_t, ent), (ctx_t, ent)]
        outs = {k: torch.empty(n, O, device='cuda') for k in ('fused', 'unfused')}
        fns = {k: (lambda k=k: ops.conv_pool(src, wp, win, pad, T - win + 1, T, bias=b, out=outs[k], fused=(k == 'fused'))) for k in outs}
        _report(res, label, interleaved(fns, rounds, inner, warmup), flop=2.0 * n * T * O * 3 * win * C)
        res['%s_max_abs_diff' % label] = float((outs['fused'] - outs['unfused']).abs().max())
    return res


def _model(content_encoder, **over):
    extra = dict(entity_size=ENTITY_SIZE) if content_encoder == 'KCNN' else {}
    cfg = make_config(content_encoder=content_encoder, vocabulary_size=50000, **extra, **over)
    m = Model(cfg)
    m.initialize()
    synth.fill_state_dict(m, 7)
    return cfg, m.cuda()


def _batch(cfg, seed):
    batch = synth.make_batch(cfg, 32, 5, seed=seed)
    if cfg.content_encoder == 'KCNN':
        for side in ('user', 'news'):
            text = batch[side + '_title_text']
            on = torch.from_numpy(synth.uniform01(side + '.bench_entity.on', seed, text.numel()) < 0.25).view(text.shape)
            ids = torch.from_numpy(synth.randint(side + '.bench_entity.ids', seed, text.numel(), 1, cfg.entity_size)).view(text.shape)
            batch[side + '_title_entity'] = torch.where(on & (text != 0), ids, torch.zeros_like(ids)).int()
    return [v.cuda() for v in batch.values()]


def bench_score(rounds, inner, warmup):
    fns = {}
    keep = []
    for name, enc, fused in (('kcnn_fused', 'KCNN', True), ('kcnn_unfused', 'KCNN', False), ('cnn', 'CNN', None)):
        cfg, model = _model(enc)
        batch = _batch(cfg, 3)
        model.eval()
        model.training = True
        keep.append((model, batch))

        def fwd(model=model, batch=batch, fused=fused):
            if fused is not None and not model._graphs:
                ops.FUSED_CONV_POOL = fused               # read while the graph is captured, on the first call
            with torch.no_grad():
                model(*batch)
        fns[name] = fwd
    res = {}
    _report(res, 'score', interleaved(fns, rounds, inner, warmup))
    return res


def bench_train(rounds, inner, warmup):
    fns = {}
    for name, enc in (('kcnn', 'KCNN'), ('cnn', 'CNN')):
        cfg, model = _model(enc)
        batch = _batch(cfg, 4)
        model.train()
        torch.manual_seed(0)
        step = TrainStep(model, lr=1e-4, gradient_clip_norm=4.0)
        fns[name] = (lambda step=step, batch=batch: step.step(*batch))
    res = {}
    _report(res, 'train_step', interleaved(fns, rounds, inner, warmup))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='all', choices=['all', 'kernel', 'score', 'train'])
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    out = {'device': torch.cuda.get_device_name(0), 'rounds': a.rounds, 'inner': a.inner}
    if a.part in ('all', 'kernel'):
        out.update(bench_kernel(a.rounds, a.inner, a.warmup))
    if a.part in ('all', 'score'):
        out.update(bench_score(a.rounds, a.inner, a.warmup))
    if a.part in ('all', 'train'):
        out.update(bench_train(a.rounds, max(1, a.inner // 5), a.warmup))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
