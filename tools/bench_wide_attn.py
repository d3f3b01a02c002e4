"""Measurements of the wide-head attention kernels (csrc/token_attn_wide_f32.hip) on one MI355X: the numbers behind DESIGN.md's "Wide
attention heads" section.  Writes profiles/wide_attn.json and prints the same JSON line.

    python tools/bench_wide_attn.py [--steps N] [--warmup W] [--rounds R] [--out PATH]

kernels  on the config-2b token shapes (1,760 sequences x 128 body tokens and x 32 title tokens, E = 300): the wide forward and backward
         at 3 heads x 100 and 5 heads x 60, next to the narrow kernels at 10 heads x 30 padded to 32 columns, on the same number of
         tokens.  ms per call and the FLOP/s of the ALGORITHMIC work (forward 4 S^2 hd per (sequence, head), backward 10 S^2 hd -- the
         wide backward computes 18 S^2 hd, its tiles three times) against the 157 TF of the fp32 MFMA.
models   one graph-replayed scoring step and one TrainStep (dropouts on) of Model at head_num 3, 5 and 10: batch 32, history 50,
         K = 1 + 4, title 32, body 128.
Everything runs in one process; the variants of a part are timed interleaved after warm-up with device events, ``--rounds`` times each,
and the median is reported, so clock and temperature drift hits them alike.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lime_cikm25_amd import Model, make_config, ops, synth  # noqa: E402
from lime_cikm25_amd.training import TrainStep  # noqa: E402

PEAK_FP32_MFMA = 157e12
N_SEQ = 1760                    # config 2b: 32 x (5 candidates + 50 clicked news)


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


def bench_kernels(steps, warmup, rounds):
    res = {}
    g = torch.Generator(device='cuda').manual_seed(1)
    for S in (128, 32):
        fns, flops = {}, {}
        for nh, hd, hs in ((3, 100, 100), (5, 60, 60), (10, 30, 32)):
            tok, W = N_SEQ * S, nh * hs
            qkv = torch.zeros(tok, 3, nh, hs, device='cuda')
            qkv[..., :hd] = torch.rand(tok, 3, nh, hd, generator=g, device='cuda') * 2 - 1
            qkv = qkv.view(tok, 3 * W)
            dout = torch.rand(tok, nh * hd, generator=g, device='cuda') * 2 - 1
            q, k, v = qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:]
            scale = 1.0 / math.sqrt(hd)
            out = torch.empty(tok, nh * hd, device='cuda')
            dqkv = torch.empty(tok, 3 * W, device='cuda')
            tag = 'S%d_%dx%d' % (S, nh, hd)
            fns[tag + '_fwd'] = lambda a=(q, k, v, N_SEQ, S, nh, hd, scale), hs=hs, out=out: ops.token_attention(*a, head_stride=hs, out=out)
            fns[tag + '_bwd'] = lambda a=(q, k, v, dout, N_SEQ, S, nh, hd, scale), hs=hs, out=out, d=dqkv: ops.token_attention_bwd(
                *a, head_stride=hs, out=out, dqkv=d)
            flops[tag + '_fwd'] = 4.0 * N_SEQ * nh * S * S * hd
            flops[tag + '_bwd'] = 10.0 * N_SEQ * nh * S * S * hd
        for name, ms in interleaved(fns, steps, warmup, rounds).items():
            res[name + '_ms'] = ms
            res[name + '_tflops'] = flops[name] / (ms * 1e-3) / 1e12
            res[name + '_of_fp32_mfma_peak'] = flops[name] / (ms * 1e-3) / PEAK_FP32_MFMA
    return res


def bench_models(steps, warmup, rounds):
    score, train = {}, {}
    for nh in (3, 5, 10):
        cfg = make_config(head_num=nh, vocabulary_size=50000)
        model = Model(cfg)
        model.initialize()
        synth.fill_state_dict(model, 7)
        model = model.cuda()
        batch = [v.cuda() for v in synth.make_batch(cfg, 32, 5, seed=3).values()]
        model.eval()
        model.training = True

        def fwd(m=model, b=batch):
            with torch.no_grad():
                m(*b)
        score['score_head_num_%d' % nh] = fwd
        cfg_t = make_config(head_num=nh, vocabulary_size=50000)
        tmodel = Model(cfg_t)
        tmodel.initialize()
        synth.fill_state_dict(tmodel, 7)
        tmodel = tmodel.cuda().train()
        torch.manual_seed(0)
        step = TrainStep(tmodel, lr=1e-4, gradient_clip_norm=4.0)
        train['train_step_head_num_%d' % nh] = (lambda step=step, b=batch: step.step(*b))
    res = {k + '_ms': v for k, v in interleaved(score, steps, warmup, rounds).items()}
    res.update({k + '_ms': v for k, v in interleaved(train, max(5, steps // 5), warmup, rounds).items()})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wide_attn.json'))
    a = ap.parse_args()
    out = {'device': torch.cuda.get_device_name(0), 'n_seq': N_SEQ, 'peak_fp32_mfma_tflops': PEAK_FP32_MFMA / 1e12,
           'steps': a.steps, 'warmup': a.warmup, 'rounds': a.rounds}
    out.update(bench_kernels(a.steps, a.warmup, a.rounds))
    out.update(bench_models(a.steps, a.warmup, a.rounds))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
