"""CNE's per-news recurrence cache on one MI355X (the numbers behind DESIGN.md "CNE content encoder", recurrence cache).  Prints one JSON
line and, with --json-out, writes it to a file (profiles/cne_cache.json).

    python tools/bench_cne_cache.py [--news 2000] [--impressions 540] [--rounds 3] [--json-out profiles/cne_cache.json]

A synthetic corpus and dev split from a seed (lime_cikm25_amd.synth, tools/bench_eval.py's split: about 37 candidate rows an
impression), LIME-CNE-CROWN at the default widths (hidden_dim 400, 32 + 128 token slots, history 50, 32 rows per forward).  Timed:
  * Model.build_recurrence_cache over the corpus (host clock around work that ends in a device synchronise), and the cache's nbytes;
  * util.compute_scores_cached without and with ``recurrence_cache`` (the cached pass includes its build), alternated ``--rounds``
    times; medians and spread, the largest score difference between the two;
  * util.evaluate_cached_on_device with ``recurrence_cache`` (many reference-sized chunks per launch chain);
  * lime_cne_gate_cached_f32 alone at cap = 1632 (32 candidates + 1600 history news), S = 32 and 128, C = 800, against the three launches
    it stands for: the packed rows gathered to a dense hout (a torch index_select), the H GEMM with the memory term as a residual, and
    lime_gate_mul_f32 (device events, medians).
The yardstick is the uncached pass of the same commit in the same run.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bench_eval import make_dev_split, say, spread, timed  # noqa: E402
from lime_cikm25_amd import DeviceCorpus, Model, formats, make_config, ops, synth, util  # noqa: E402


def event_ms(fn, steps=20, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def bench_gate(cap=1632, C=800, n_news=2000, seed=3):
    """The gate of one batch from the cache against the dense gather + H GEMM + gate_mul, per S."""
    res = {}
    g = torch.Generator().manual_seed(seed)
    H_w = ((torch.rand(C, C, generator=g) * 2 - 1) * 0.05).cuda()
    for S in (32, 128):
        lens = torch.randint(1, S + 1, (n_news,), generator=g)
        offsets = torch.zeros(n_news + 1, dtype=torch.int64)
        offsets[1:] = torch.cumsum(lens, 0)
        rows = int(offsets[-1])
        h = (torch.rand(rows, C, generator=g) * 2 - 1).cuda()
        hh = ops.linear(h, H_w, None)
        idx = torch.randint(0, n_news, (cap,), generator=g).to(torch.int32)
        tm = (torch.rand(cap, C, generator=g) * 2 - 1).cuda()
        t = torch.arange(S)[None, :]
        live = t < lens[idx.long()][:, None]                                                       # [cap, S]
        src = torch.where(live, offsets[idx.long()][:, None] + t, torch.full_like(t, rows)).reshape(-1).cuda()
        h_pad = torch.cat([h, torch.zeros(1, C, device='cuda')])                                   # row `rows`: the zeros behind a length
        d_lens, d_offs, d_idx = lens.int().cuda(), offsets.cuda(), idx.cuda()
        out = torch.empty(cap * S, C, device='cuda')

        def cached():
            ops.cne_gate_cached(h, hh, d_offs, d_lens, d_idx, tm, S, out=out)

        def three_launches():
            hout = h_pad.index_select(0, src)
            pre = ops.linear(hout, H_w, None, res=tm, res_div=S)
            ops.gate_mul(hout, pre, out=pre)
            return pre

        cached()
        diff = float((three_launches() - out).abs().max())
        a, b = event_ms(cached), event_ms(three_launches)
        live_rows = int(live.sum())
        moved = (2 * live_rows + cap * S) * C * 4 + cap * C * 4                                    # h, hh read; out written; tm read
        res['gate_S%d' % S] = {'cached_ms': round(a, 4), 'three_launches_ms': round(b, 4), 'ratio': round(b / a, 2), 'live_rows': live_rows,
                               'bytes_moved': moved, 'cached_GBps': round(moved / a / 1e6, 1), 'max_abs_diff': diff}
        say('gate S=%d: cached %.3f ms (%.0f GB/s over %d live rows), three launches %.3f ms' % (S, a, moved / a / 1e6, live_rows, b))
        del h, hh, h_pad, out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--news', type=int, default=2000)
    ap.add_argument('--impressions', type=int, default=540)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--json-out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_cne_cache.py measures on the GPU: there is no CPU path'

    cfg = make_config(content_encoder='CNE', vocabulary_size=50000)
    corpus = synth.synth_corpus(cfg, n_news=args.news, n_train=1, n_dev=1, seed=args.seed)
    dc = DeviceCorpus(corpus)
    beh, indices, labels, counts = make_dev_split(cfg, dc, args.impressions, args.news, args.seed)
    say('dev split: %d impressions, %d rows over %d news' % (len(labels), beh.num, args.news))
    model = Model(cfg)
    model.initialize()
    synth.fill_state_dict(model, seed=args.seed)
    model = model.cuda().eval()
    per = cfg.batch_size
    tmp = tempfile.mkdtemp(prefix='bench_cne_cache_')
    truth = formats.write_truth_file(os.path.join(tmp, 'truth.txt'), labels)
    plain_file, cached_file = os.path.join(tmp, 'plain.txt'), os.path.join(tmp, 'cached.txt')

    gate = bench_gate(cap=per + per * cfg.max_history_num, C=2 * cfg.hidden_dim, n_news=args.news)

    # the build on its own (the first call also loads the kernels: reported separately)
    dt_first, rc = timed(lambda: model.build_recurrence_cache(dc))
    build_t = [timed(lambda: model.build_recurrence_cache(dc))[0] for _ in range(args.rounds)]
    live, nbytes = int(rc.title.offsets[-1]) + int(rc.body.offsets[-1]), rc.nbytes
    say('build: first %.2f s, then %s; %.1f MB for %d live tokens' % (dt_first, build_t, rc.nbytes / 1e6, live))

    # one chunk through both routes, warm, and their difference on all rows of a short prefix
    warm = torch.arange(min(4 * per, beh.num), device='cuda')
    empty = model.build_news_cache(dc)
    a = torch.cat([model.score_behaviors(beh, warm[r:r + per], empty) for r in range(0, warm.numel(), per)])
    b = model.score_behaviors(beh, warm, empty, recurrence_cache=rc, rows_per_forward=per)
    prefix_diff = float((a - b).abs().max() / a.abs().mean())
    say('cached vs uncached scores over %d rows: max |diff| / mean |score| = %.2e' % (warm.numel(), prefix_diff))
    del rc

    plain_t, cached_t, device_t = [], [], []
    for r in range(args.rounds):
        dt, plain_metrics = timed(lambda: util.compute_scores_cached(model, beh, indices, plain_file, truth, rows_per_forward=per))
        plain_t.append(dt)
        dt, cached_metrics = timed(lambda: util.compute_scores_cached(model, beh, indices, cached_file, truth, rows_per_forward=per,
                                                                      recurrence_cache=True))
        cached_t.append(dt)
        dt, device_metrics = timed(lambda: util.evaluate_cached_on_device(model, beh, indices, labels, rows_per_forward=per,
                                                                          recurrence_cache=True))
        device_t.append(dt)
        say('round %d: uncached %.2f s, cached %.2f s, cached on the device %.2f s' % (r + 1, plain_t[-1], cached_t[-1], device_t[-1]))
    p, c, d = spread(plain_t), spread(cached_t), spread(device_t)
    result = {
        'bench': 'cne_cache', 'news': args.news, 'impressions': len(labels), 'rows': beh.num, 'rows_per_forward': per,
        'hidden_dim': cfg.hidden_dim, 'token_slots': [cfg.max_title_length, cfg.max_abstract_length], 'history': cfg.max_history_num,
        'rounds': args.rounds, 'build_first_s': round(dt_first, 3), 'build': spread(build_t), 'cache_nbytes': nbytes,
        'live_tokens': live, 'compute_scores_cached_uncached': p, 'compute_scores_cached_recurrence_cache': c,
        'evaluate_cached_on_device_recurrence_cache': d, 'rows_per_pass_on_device': util.CNE_CACHED_ROWS_PER_PASS,
        'speedup_median': round(p['median_s'] / c['median_s'], 2), 'speedup_median_on_device': round(p['median_s'] / d['median_s'], 2),
        'faster_beyond_spread': bool(c['max_s'] < p['min_s']), 'prefix_score_diff': prefix_diff,
        'metrics_uncached': [float(v) for v in plain_metrics], 'metrics_cached': [float(v) for v in cached_metrics],
        'metrics_cached_on_device': [float(v) for v in device_metrics],
        'metric_diff': float(np.abs(np.array(plain_metrics, dtype=np.float64) - np.array(cached_metrics, dtype=np.float64)).max()),
        'gate_kernel': gate, 'device': torch.cuda.get_device_name(0),
    }
    line = json.dumps(result)
    print(line)
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
