"""Measurements of the NAML content encoder on one MI355X (the numbers behind DESIGN.md's NAML section).  Prints one JSON line.

    python tools/bench_naml.py [--part all|pool|score|train] [--steps N] [--warmup W]

pool   the fused attention pool (ops.attn_pool, W1 pack included) against ops.linear(act='tanh') + ops.additive_pool at 1760 x 32
       (titles), 1760 x 128 (bodies) and 1760 x 4 (views) rows, D = A = 400: ms, algorithmic GFLOP and MB, the max abs difference.
score  impressions/s of LIME-NAML-CROWN at the config-2 shape (batch 32, history 50, K = 1 + 4, title 32, body 128), compacted and
       dense (LIME_DENSE_TOKENS=1 form), next to LIME-CNN-CROWN in the same process (graph replay, eval mode).
train  training-step ms (TrainStep: forward + backward + clip + Adam) at dropout_rate 0 and 0.2.
For kernel times run ``--part score`` under ``rocprofv3 --kernel-trace --stats -- python tools/bench_naml.py --part score``.
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


def bench_pool(steps, warmup):
    """The fused attention pool against linear(tanh) + additive_pool at the NAML shapes (1760 news: titles, bodies, the four views)."""
    res = {}
    D, A = 400, 400
    g = torch.Generator().manual_seed(1)
    w1 = ((torch.rand(A, D, generator=g) * 2 - 1) * 0.1).cuda()
    b1 = ((torch.rand(A, generator=g) * 2 - 1) * 0.1).cuda()
    w2 = ((torch.rand(A, generator=g) * 2 - 1) * 0.2).cuda()
    for name, n, T in (('title', 1760, 32), ('body', 1760, 128), ('views', 1760, 4)):
        x = torch.rand(n * T, D, generator=g).cuda()
        out = torch.empty(n, D, device='cuda')
        hidden = torch.empty(n * T, A, device='cuda')
        out2 = torch.empty(n, D, device='cuda')
        t_fused = timed(lambda: ops.attn_pool(x, w1, b1, w2, n, T, out=out), steps, warmup)        # includes the W1 pack launch

        def two():
            ops.linear(x, w1, b1, act='tanh', out=hidden)
            ops.additive_pool(hidden, w2, x, n, T, out=out2)
        t_two = timed(two, steps, warmup)
        flop = 2.0 * n * T * D * A + 2.0 * n * T * A + 2.0 * n * T * D
        # algorithmic bytes: x read twice (GEMM + weighted sum) + out; the two-launch path adds the hidden write + read
        fused_bytes = 4.0 * (2 * n * T * D + n * D)
        res.update({'%s_fused_ms' % name: t_fused, '%s_two_launch_ms' % name: t_two, '%s_fused_over_two_launch' % name: t_fused / t_two,
                    '%s_gflop' % name: flop / 1e9, '%s_fused_tflops' % name: flop / t_fused / 1e9,
                    '%s_fused_mb' % name: fused_bytes / 1e6, '%s_two_launch_mb' % name: (fused_bytes + 8.0 * n * T * A) / 1e6,
                    '%s_max_abs_diff' % name: float((out - out2).abs().max())})
    return res


def _model(content_encoder, **over):
    cfg = make_config(content_encoder=content_encoder, vocabulary_size=50000, **over)
    m = Model(cfg)
    m.initialize()
    synth.fill_state_dict(m, 7)
    return cfg, m.cuda()


def bench_score(steps, warmup):
    res = {}
    for enc in ('NAML', 'CNN'):
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
        cfg, model = _model('NAML', dropout_rate=p)
        batch = [v.cuda() for v in synth.make_batch(cfg, 32, 5, seed=4).values()]
        model.train()
        torch.manual_seed(0)
        step = TrainStep(model, lr=1e-4, gradient_clip_norm=4.0)
        res['naml_train_step_ms_dropout_%g' % p] = timed(lambda: step.step(*batch), steps, warmup)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='all', choices=['all', 'pool', 'score', 'train'])
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    out = {'device': torch.cuda.get_device_name(0)}
    if a.part in ('all', 'pool'):
        out.update(bench_pool(a.steps, a.warmup))
    if a.part in ('all', 'score'):
        out.update(bench_score(a.steps, a.warmup))
    if a.part in ('all', 'train'):
        out.update(bench_train(max(5, a.steps // 5), a.warmup))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
