"""Measurements of the ATT and MHSA user encoders on one MI355X (the numbers behind DESIGN.md's "ATT and MHSA user encoders" section).
Prints one JSON line.

    python tools/bench_user.py [--part all|tail|score|train] [--steps N] [--warmup W] [--rounds R]

tail   lime_pool_match_f32 (ops.pool_match, one launch) against ops.additive_pool + ops.lifetime_score (two launches and the expanded
       copy of the user vector between them) at (B, N, H, D, A) = (32, 5, 50, 400, 400), a training batch, and (16384, 1, 50, 400, 400),
       one rows_per_pass chunk of the eval layout: ms, algorithmic MB moved and the GB/s that makes.
score  graph-replayed scoring (eval children, [B, K] shape) of LIME-NAML-ATT and LIME-MHSA-MHSA with the tail in both forms, next to
       LIME-NAML-CROWN and LIME-MHSA-CROWN, at batch 32, history 50, K = 1 + 4, title 32, body 128: ms and impressions/s.
train  one TrainStep (forward + backward + clip + Adam, dropouts on) of the same four models.
Everything runs in one process; the forms / models of a part are timed interleaved, ``--rounds`` times each, and the median is
reported, so clock and temperature drift hits them alike.
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


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps          # ms per call


def interleaved(fns, steps, warmup, rounds):
    """{name: median ms} of the callables ``fns`` timed round-robin."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, steps))
    return {k: statistics.median(v) for k, v in ms.items()}


def bench_tail(steps, warmup, rounds):
    res = {}
    g = torch.Generator(device='cuda').manual_seed(1)
    r = lambda *shape: torch.rand(*shape, generator=g, device='cuda') * 2 - 1
    for name, (B, N, H, D, A) in (('train', (32, 5, 50, 400, 400)), ('eval', (16384, 1, 50, 400, 400))):
        hidden, w2, x, cand, rem = torch.tanh(2 * r(B * H, A)), r(A) * 0.2, r(B * H, D), r(B, N, D), r(B, N) * 30
        kw = dict(cand=cand, remaining=rem, alpha=0.05, beta=0.3, use_weight=True, use_penalty=True, want_user=False)
        t = interleaved({'fused': lambda: ops.pool_match(hidden, w2, x, B, H, fused=True, **kw),
                         'two_launch': lambda: ops.pool_match(hidden, w2, x, B, H, fused=False, **kw)}, steps, warmup, rounds)
        # algorithmic bytes: hidden + x once, the candidates, the logits; the two-launch form adds the user vector's write and read and
        # the write + read of its copy expanded over N
        fused_b = 4.0 * (B * H * (A + D) + B * N * D + 2 * B * N)
        two_b = fused_b + 4.0 * (2 * B * D + 2 * B * N * D)
        _, l1 = ops.pool_match(hidden, w2, x, B, H, fused=True, **kw)
        _, l2 = ops.pool_match(hidden, w2, x, B, H, fused=False, **kw)
        res.update({'%s_fused_ms' % name: t['fused'], '%s_two_launch_ms' % name: t['two_launch'],
                    '%s_fused_over_two_launch' % name: t['fused'] / t['two_launch'],
                    '%s_fused_mb' % name: fused_b / 1e6, '%s_two_launch_mb' % name: two_b / 1e6,
                    '%s_fused_gb_per_s' % name: fused_b / t['fused'] / 1e6, '%s_two_launch_gb_per_s' % name: two_b / t['two_launch'] / 1e6,
                    '%s_max_abs_diff' % name: float((l1 - l2).abs().max())})
    return res


MODELS = (('NAML', 'ATT'), ('MHSA', 'MHSA'), ('NAML', 'CROWN'), ('MHSA', 'CROWN'))


def _model(content, user, **over):
    cfg = make_config(content_encoder=content, user_encoder=user, vocabulary_size=50000, **over)
    m = Model(cfg)
    m.initialize()
    synth.fill_state_dict(m, 7)
    return cfg, m.cuda()


def bench_score(steps, warmup, rounds):
    """Each form of the tail in a pass of its own (switching it re-captures the graphs); inside a pass the four models are interleaved.
    The CROWN yardsticks do not read the switch and are timed in both passes: their two figures show the spread between passes."""
    models = []
    for content, user in MODELS:
        cfg, model = _model(content, user)
        batch = [v.cuda() for v in synth.make_batch(cfg, 32, 5, seed=3).values()]
        model.eval()
        model.training = True
        models.append(('lime_%s_%s' % (content.lower(), user.lower()), user, model, batch))

    def fwd(model, batch):
        with torch.no_grad():
            model(*batch)

    default, res = ops.FUSED_POOL_MATCH, {}
    for form, tag in ((True, 'fused'), (False, 'two_launch')):
        ops.FUSED_POOL_MATCH = form
        for _, _, model, _ in models:
            model._graphs.clear()
        fns = {name + '_' + (tag if user != 'CROWN' else 'pass_' + tag): (lambda m=model, b=batch: fwd(m, b)) for name, user, model, batch in models}
        for k, ms in interleaved(fns, steps, warmup, rounds).items():
            res[k + '_ms'] = ms
            res[k + '_impressions_per_s'] = 32 / (ms / 1e3)
    ops.FUSED_POOL_MATCH = default
    return res


def bench_train(steps, warmup, rounds):
    fns = {}
    for content, user in MODELS:
        cfg, model = _model(content, user)
        batch = [v.cuda() for v in synth.make_batch(cfg, 32, 5, seed=4).values()]
        model.train()
        torch.manual_seed(0)
        step = TrainStep(model, lr=1e-4, gradient_clip_norm=4.0)
        fns['lime_%s_%s_train_step' % (content.lower(), user.lower())] = (lambda step=step, batch=batch: step.step(*batch))
    return {k + '_ms': v for k, v in interleaved(fns, steps, warmup, rounds).items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='all', choices=['all', 'tail', 'score', 'train'])
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    out = {'device': torch.cuda.get_device_name(0)}
    if a.part in ('all', 'tail'):
        out.update(bench_tail(4 * a.steps, a.warmup, a.rounds))        # short kernels: a longer window
    if a.part in ('all', 'score'):
        out.update(bench_score(a.steps, a.warmup, a.rounds))
    if a.part in ('all', 'train'):
        out.update(bench_train(max(5, a.steps // 5), a.warmup, a.rounds))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
