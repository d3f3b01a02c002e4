"""Measurements of the CNE content encoder on one MI355X (the numbers behind DESIGN.md's CNE section).  Prints one JSON line and, with
--out, writes it to a file (profiles/cne.json).

    python tools/bench_cne.py [--part all|step|score|train] [--steps N] [--warmup W] [--rounds R] [--out FILE]

step   the LSTM recurrence (ops.lstm: T launches of lime_lstm_step_f32) at R = 1760, h = 400, T = 32 and 128, against a yardstick built
       here only: per step and direction ops.linear(h_prev, W_hh) + torch gate arithmetic.  ms per recurrence, us per step, the ratio.
score  ms per batch-32 forward (graph replay, eval children, [B, K] shape) of LIME-CNE-CROWN beside LIME-CROWN-CROWN and LIME-NAML-CROWN.
train  TrainStep ms at batch 32 for the same three.
One process; the forms of a part are interleaved over --rounds rounds and the medians reported.  Run every part under its own time
limit, e.g. ``timeout -k 10 300 python tools/bench_cne.py --part step``.
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


def interleaved(forms, steps, warmup, rounds):
    """{name: median ms} of the callables in ``forms``, measured round-robin."""
    ms = {k: [] for k in forms}
    for r in range(rounds):
        for k, fn in forms.items():
            ms[k].append(timed(fn, steps, warmup if r == 0 else 1))
    return {k: statistics.median(v) for k, v in ms.items()}


def bench_step(steps, warmup, rounds):
    res = {}
    R, h = 1760, 400
    g = torch.Generator().manual_seed(1)
    whh = ((torch.rand(2, 4 * h, h, generator=g) * 2 - 1) * 0.05).cuda()
    for T in (32, 128):
        gi = ((torch.rand(R * T, 8 * h, generator=g) * 2 - 1)).cuda()
        lens = torch.randint(T // 2, T + 1, (R,), generator=g).to(torch.int32).cuda()
        hout = torch.zeros(R * T, 2 * h, device='cuda')
        c = torch.zeros(2, R, h, device='cuda')
        gi3 = gi.view(R, T, 8 * h)

        def kernel():
            hout.zero_()
            ops.lstm(gi, whh, lens, T, hout=hout, c=c)

        def yardstick():
            # full-length sequences only (no length handling): what a GEMM + element-wise gate arithmetic per step costs at least
            hp = [torch.zeros(R, h, device='cuda') for _ in (0, 1)]
            cc = [torch.zeros(R, h, device='cuda') for _ in (0, 1)]
            for s in range(T):
                for d in (0, 1):
                    t = s if d == 0 else T - 1 - s
                    pre = ops.linear(hp[d], whh[d]) + gi3[:, t, d * 4 * h:(d + 1) * 4 * h]
                    i, f, gg, o = pre.split(h, dim=1)
                    cc[d] = torch.sigmoid(f) * cc[d] + torch.sigmoid(i) * torch.tanh(gg)
                    hp[d] = torch.sigmoid(o) * torch.tanh(cc[d])

        ms = interleaved({'kernel': kernel, 'yardstick': yardstick}, max(3, steps // 5), warmup, rounds)
        res.update({'lstm_T%d_ms' % T: ms['kernel'], 'lstm_T%d_us_per_step' % T: 1e3 * ms['kernel'] / T,
                    'yardstick_T%d_ms' % T: ms['yardstick'], 'lstm_T%d_over_yardstick' % T: ms['kernel'] / ms['yardstick'],
                    'lstm_T%d_gflop' % T: 2.0 * 2 * R * T * h * 4 * h / 1e9})
        del gi, gi3
    return res


def _model(content_encoder, **over):
    cfg = make_config(content_encoder=content_encoder, vocabulary_size=50000, **over)
    m = Model(cfg)
    m.initialize()
    synth.fill_state_dict(m, 7)
    return cfg, m.cuda()


ENCODERS = ('CNE', 'CROWN', 'NAML')


def bench_score(steps, warmup, rounds):
    forms = {}
    for enc in ENCODERS:
        cfg, model = _model(enc)
        batch = [v.cuda() for v in synth.make_batch(cfg, 32, 5, seed=3).values()]
        model.eval()
        model.training = True

        def fwd(model=model, batch=batch):
            with torch.no_grad():
                model(*batch)
        forms['%s_score_ms' % enc.lower()] = fwd
    res = interleaved(forms, steps, warmup, rounds)
    res.update({k.replace('_ms', '_impressions_per_s'): 32 / (v / 1e3) for k, v in list(res.items())})
    return res


def bench_train(steps, warmup, rounds):
    forms = {}
    for enc in ENCODERS:
        cfg, model = _model(enc)
        batch = [v.cuda() for v in synth.make_batch(cfg, 32, 5, seed=4).values()]
        model.train()
        torch.manual_seed(0)
        step = TrainStep(model, lr=1e-4, gradient_clip_norm=4.0)
        forms['%s_train_step_ms' % enc.lower()] = lambda step=step, batch=batch: step.step(*batch)
    return interleaved(forms, max(3, steps // 5), min(warmup, 2), rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='all', choices=['all', 'step', 'score', 'train'])
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    out = {'device': torch.cuda.get_device_name(0), 'steps': a.steps, 'rounds': a.rounds}
    if a.part in ('all', 'step'):
        out.update(bench_step(a.steps, a.warmup, a.rounds))
    if a.part in ('all', 'score'):
        out.update(bench_score(a.steps, a.warmup, a.rounds))
    if a.part in ('all', 'train'):
        out.update(bench_train(a.steps, a.warmup, a.rounds))
    print(json.dumps(out))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write('\n')


if __name__ == '__main__':
    main()
