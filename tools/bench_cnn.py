"""Measurements of the CNN content encoder on one MI355X (the numbers behind DESIGN.md's CNN row).  Prints one JSON line.

    python tools/bench_cnn.py [--part all|conv|score|train] [--steps N] [--warmup W]

conv   the windowed conv kernel on the scoring shape (1760 news x 32 tokens, 300 -> 400, window 3, word rows gathered in the A fetch)
       next to ops.linear (the same split-product arithmetic) on a materialised [56320, 900] im2col matrix of the same rows (the
       im2col build is not timed); algorithmic TFLOP/s = 2 M N (window C) / t for both.
score  impressions/s of LIME-CNN-CROWN at the config-2 shape (batch 32, history 50, K = 1 + 4, title 32), compacted and dense
       (LIME_DENSE_TOKENS=1 form), next to LIME-MHSA-CROWN in the same process (graph replay, eval mode).
train  training-step ms (TrainStep: forward + backward + clip + Adam) at dropout_rate 0 and 0.2.
For kernel times run ``--part score`` under ``rocprofv3 --kernel-trace --stats -- python tools/bench_cnn.py --part score``.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lime_cikm25_amd import Model, make_config, newsEncoders, ops, synth  # noqa: E402
from lime_cikm25_amd.training import TrainStep  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps          # ms per call


def bench_conv(steps, warmup):
    n, T, C, O, win, V = 1760, 32, 300, 400, 3, 50000
    g = torch.Generator().manual_seed(1)
    table = (torch.rand(V, C, generator=g) * 2 - 1).cuda()
    ids = torch.randint(0, V, (n * T,), generator=g, dtype=torch.int32).cuda()
    w = ((torch.rand(O, C, win, generator=g) * 2 - 1) * 0.1).cuda()
    b = (torch.rand(O, generator=g) - 0.5).cuda()
    wp = ops.conv1d_pack(w)
    out = torch.empty(n * T, O, device='cuda')
    t_conv = timed(lambda: ops.conv1d_window(table, wp, win, T, ids=ids, bias=b, act='relu', out=out), steps, warmup)
    x = table[ids.long()].view(n, T, C)
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1))
    im2col = torch.cat([xp[:, j:j + T] for j in range(win)], dim=2).reshape(n * T, win * C).contiguous()
    out2 = torch.empty(n * T, O, device='cuda')
    t_lin = timed(lambda: ops.linear(im2col, wp, b, act='relu', out=out2), steps, warmup)
    flop = 2.0 * n * T * O * win * C
    diff = float((out - out2).abs().max())
    return dict(conv_ms=t_conv, conv_tflops=flop / t_conv / 1e9, im2col_linear_ms=t_lin, im2col_linear_tflops=flop / t_lin / 1e9,
                gflop=flop / 1e9, max_abs_diff=diff, linear_kernel=ops._lib.load().lime_last_linear_kernel().decode())


def _model(content_encoder, **over):
    cfg = make_config(content_encoder=content_encoder, vocabulary_size=50000, **over)
    m = Model(cfg)
    m.initialize()
    synth.fill_state_dict(m, 7)
    return cfg, m.cuda()


def bench_score(steps, warmup):
    res = {}
    for enc in ('CNN', 'MHSA'):
        cfg, model = _model(enc)
        batch = [v.cuda() for v in synth.make_batch(cfg, 32, 5, seed=3).values()]
        model.eval()
        model.training = True
        for dense in (False, True):
            newsEncoders.DEDUP = not dense
            model._graphs.clear()

            def fwd():
                with torch.no_grad():
                    model(*batch)
            ms = timed(fwd, steps, warmup)
            res['%s_%s_impressions_per_s' % (enc.lower(), 'dense' if dense else 'compacted')] = 32 / (ms / 1e3)
            res['%s_%s_ms' % (enc.lower(), 'dense' if dense else 'compacted')] = ms
        newsEncoders.DEDUP = True
    return res


def bench_train(steps, warmup):
    res = {}
    for p in (0.0, 0.2):
        cfg, model = _model('CNN', dropout_rate=p)
        batch = [v.cuda() for v in synth.make_batch(cfg, 32, 5, seed=4).values()]
        model.train()
        torch.manual_seed(0)
        step = TrainStep(model, lr=1e-4, gradient_clip_norm=4.0)
        res['cnn_train_step_ms_dropout_%g' % p] = timed(lambda: step.step(*batch), steps, warmup)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='all', choices=['all', 'conv', 'score', 'train'])
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    out = {'device': torch.cuda.get_device_name(0)}
    if a.part in ('all', 'conv'):
        out.update(bench_conv(a.steps, a.warmup))
    if a.part in ('all', 'score'):
        out.update(bench_score(a.steps, a.warmup))
    if a.part in ('all', 'train'):
        out.update(bench_train(max(5, a.steps // 5), a.warmup))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
