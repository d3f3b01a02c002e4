"""The dev pass at a size a user would run, both ways in one process: util.compute_scores_cached (config.batch_size rows per
forward, every chunk copied to the host, numpy ranks, rank file, evaluate.scoring over the files) against
util.evaluate_cached_on_device (large passes into one device score buffer, ranks and metrics in one lime_rank_metrics call).

A synthetic dev split from a seed (lime_cikm25_amd.synth): ``--impressions`` impressions with MIND-like candidate counts (log-normal,
2 .. 299, mean about 37), every impression with at least one positive and one negative.  Timed:
  * the host tail on its own: rank_impressions + write_rank_file + scoring (host clock);
  * the lime_rank_metrics call on its own (device events around the call: its three kernels);
  * the two whole passes, alternated ``--rounds`` times (host clock around work that ends in a device synchronise); medians and spread;
  * per ``--rows-per-pass`` value the whole device pass, and one score_behaviors pass of that many rows with its peak device memory.
The yardstick is compute_scores_cached in the same run.  Prints one JSON line; ``--json-out`` also writes it to a file.

    python tools/bench_eval.py --impressions 50000 --rounds 3 --json-out profiles/device_eval.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from lime_cikm25_amd import DeviceBehaviors, DeviceCorpus, Model, evaluate, formats, make_config, ops, synth, util  # noqa: E402


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def normal(tag, seed, n):
    u1, u2 = synth.uniform01(tag + '.a', seed, n), synth.uniform01(tag + '.b', seed, n)
    return np.sqrt(-2.0 * np.log(np.maximum(u1, 1e-12))) * np.cos(2.0 * np.pi * u2)


def log_uniform(tag, seed, n, lo, hi):
    return np.exp(np.log(lo) + synth.uniform01(tag, seed, n) * (np.log(hi) - np.log(lo)))


def make_dev_split(cfg, dc, n_imp, n_news, seed):
    """(DeviceBehaviors, indices, per-impression label lists): one history per impression, shared by its candidate rows."""
    H = cfg.max_history_num
    counts = np.clip(np.rint(np.exp(3.3 + 0.8 * normal('dev.count', seed, n_imp))), 2, 299).astype(np.int64)
    R = int(counts.sum())
    indices = np.repeat(np.arange(n_imp), counts)
    n_hist = synth.randint('dev.hn', seed, n_imp, 0, H + 1)
    hist = synth.randint('dev.h', seed, n_imp * H, 1, n_news).reshape(n_imp, H).astype(np.int32)
    mask = np.arange(H)[None, :] < n_hist[:, None]
    hist = np.where(mask, hist, 0).astype(np.int32)
    fr = np.where(mask, log_uniform('dev.fr', seed, n_imp * H, 60.0, 30 * 86400.0).reshape(n_imp, H), 0.0).astype(np.float32)
    lt = np.where(mask, log_uniform('dev.lt', seed, n_imp * H, 600.0, 14 * 86400.0).reshape(n_imp, H), 0.0).astype(np.float32)
    user = synth.randint('dev.uid', seed, n_imp, 0, cfg.user_num)
    cand = synth.randint('dev.cand', seed, R, 1, n_news).astype(np.int32).reshape(R, 1)
    cfr = log_uniform('dev.cfr', seed, R, 60.0, 30 * 86400.0).astype(np.float32).reshape(R, 1)
    clt = log_uniform('dev.clt', seed, R, 600.0, 14 * 86400.0).astype(np.float32).reshape(R, 1)
    beh = DeviceBehaviors(dc, user[indices], hist[indices], mask[indices], fr[indices], lt[indices], cand, cfr, clt, eval_shape=True)
    y = (synth.uniform01('dev.label', seed, R) < 0.04).astype(np.int64)
    starts = np.cumsum(counts) - counts
    a = (synth.uniform01('dev.pos', seed, n_imp) * counts).astype(np.int64) % counts
    b = (a + 1 + (synth.uniform01('dev.neg', seed, n_imp) * (counts - 1)).astype(np.int64) % (counts - 1)) % counts
    y[starts + a], y[starts + b] = 1, 0
    flat = y.tolist()
    labels = [flat[s:s + c] for s, c in zip(starts.tolist(), counts.tolist())]
    return beh, indices.tolist(), labels, counts


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def spread(xs):
    return {'median_s': round(statistics.median(xs), 4), 'min_s': round(min(xs), 4), 'max_s': round(max(xs), 4), 'runs': [round(x, 4) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--impressions', type=int, default=50000)
    ap.add_argument('--news', type=int, default=20000)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--rows-per-pass', type=int, nargs='*', default=[1024, 4096, 8192, 32768, 131072])
    ap.add_argument('--json-out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_eval.py measures on the GPU: there is no CPU path'

    cfg = make_config(vocabulary_size=50000)
    corpus = synth.synth_corpus(cfg, n_news=args.news, n_train=1, n_dev=1, seed=args.seed)
    dc = DeviceCorpus(corpus)
    t0 = time.perf_counter()
    beh, indices, labels, counts = make_dev_split(cfg, dc, args.impressions, args.news, args.seed)
    say('dev split: %d impressions, %d rows (candidates per impression: mean %.1f, max %d) in %.1f s' % (
        len(labels), beh.num, counts.mean(), counts.max(), time.perf_counter() - t0))
    model = Model(cfg)
    model.initialize()
    synth.fill_state_dict(model, seed=args.seed)
    model = model.cuda().eval()
    per = cfg.batch_size
    tmp = tempfile.mkdtemp(prefix='bench_eval_')
    truth = formats.write_truth_file(os.path.join(tmp, 'truth.txt'), labels)
    old_file, new_file = os.path.join(tmp, 'old.txt'), os.path.join(tmp, 'new.txt')

    def old_pass():
        return util.compute_scores_cached(model, beh, indices, old_file, truth, rows_per_forward=per)

    def new_pass(rows_per_pass=util.DEVICE_EVAL_ROWS_PER_PASS, **kw):
        return util.evaluate_cached_on_device(model, beh, indices, labels, result_file=new_file, rows_per_forward=per,
                                              rows_per_pass=rows_per_pass, **kw)

    # warm-up of every shape the timed windows use: a short prefix through both passes' forwards, then one whole device pass
    cache = model.build_news_cache(dc)
    for n in (per, util.DEVICE_EVAL_ROWS_PER_PASS // per * per):
        model.score_behaviors(beh, torch.arange(min(n, beh.num), device='cuda'), cache, n_src=per)
    del cache
    dt, (new_metrics, scores) = timed(lambda: new_pass(return_scores=True))
    say('device pass (warm-up): %.2f s' % dt)

    # the host tail on its own, on the scores of the device pass
    host_scores = scores.cpu().tolist()
    t0 = time.perf_counter()
    ranks = util.rank_impressions(host_scores, indices)
    t1 = time.perf_counter()
    util.write_rank_file(old_file, ranks)
    t2 = time.perf_counter()
    with open(truth) as tf, open(old_file) as rf:
        host_metrics = evaluate.scoring(tf, rf)
    t3 = time.perf_counter()
    host_tail = {'rank_impressions_s': round(t1 - t0, 3), 'write_rank_file_s': round(t2 - t1, 3), 'scoring_s': round(t3 - t2, 3),
                 'total_s': round(t3 - t0, 3)}
    say('host tail:', host_tail)
    same_file = open(old_file).read() == open(new_file).read()
    metric_diff = float(np.abs(np.array(host_metrics) - np.array(new_metrics)).max())
    say('device ranks == host ranks of the same scores: %s; metrics differ by %.2e' % (same_file, metric_diff))

    # the lime_rank_metrics call on its own: device events around the call
    off, row_labels, skip = evaluate.impression_layout(indices, labels)
    d_lab, d_skip, d_off = torch.from_numpy(row_labels).cuda(), torch.from_numpy(skip).cuda(), torch.from_numpy(off).cuda()
    for _ in range(3):
        ops.rank_metrics(scores, d_lab, off, d_skip)
    kernel_ms = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.rank_metrics(scores, d_lab, off, d_skip)
        e1.record()
        e1.synchronize()
        kernel_ms.append(e0.elapsed_time(e1))
    say('lime_rank_metrics (with the host-side offsets check and copy): median %.3f ms' % statistics.median(kernel_ms))
    del d_off

    # the two whole passes, alternated
    old_t, new_t, old_metrics = [], [], None
    for r in range(args.rounds):
        dt, old_metrics = timed(old_pass)
        old_t.append(dt)
        say('round %d: compute_scores_cached %.2f s' % (r + 1, dt))
        dt, m = timed(new_pass)
        new_t.append(dt)
        say('round %d: evaluate_cached_on_device %.2f s' % (r + 1, dt))
        assert m == new_metrics, 'the device pass is not reproducible run to run'
    old_lines, new_lines = open(old_file).read().split('\n'), open(new_file).read().split('\n')
    same_lines = sum(1 for a, b in zip(old_lines, new_lines) if a == b)

    # rows per pass: the whole device pass, and one score_behaviors pass of that many rows on its own with its peak device memory
    # (the news cache and the behaviour tables are resident in both)
    sweep = []
    cache = model.build_news_cache(dc)
    for rpp in args.rows_per_pass:
        n = min(rpp // per * per, beh.num)
        rows = torch.arange(n, device='cuda')
        model.score_behaviors(beh, rows, cache, n_src=per)                 # warm: kernels loaded, the allocator holds the blocks
        dt_one, _ = timed(lambda: model.score_behaviors(beh, rows, cache, n_src=per))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()                                           # the memory figure from a cold allocator, in a call of its own
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        model.score_behaviors(beh, rows, cache, n_src=per)
        torch.cuda.synchronize()
        peak = int(torch.cuda.max_memory_allocated() - base)
        dt, _ = timed(lambda: new_pass(rows_per_pass=rpp))
        sweep.append({'rows_per_pass': rpp, 'whole_pass_s': round(dt, 3), 'one_score_pass_rows': n, 'one_score_pass_ms': round(dt_one * 1e3, 3),
                      'one_score_pass_peak_bytes': peak, 'peak_bytes_per_row': round(peak / max(1, n))})
        say('rows_per_pass %d: whole pass %.2f s; one score pass of %d rows %.2f ms, peak %.3f GB (%.0f bytes a row)' % (
            rpp, dt, n, dt_one * 1e3, peak / 1e9, peak / max(1, n)))
    del cache

    o, n = spread(old_t), spread(new_t)
    result = {
        'bench': 'device_eval', 'impressions': len(labels), 'rows': beh.num, 'news': args.news, 'rows_per_forward': per,
        'rows_per_pass': util.DEVICE_EVAL_ROWS_PER_PASS, 'rounds': args.rounds,
        'host_tail': host_tail,
        'rank_metrics_call_ms': {'median': round(statistics.median(kernel_ms), 4), 'min': round(min(kernel_ms), 4), 'max': round(max(kernel_ms), 4)},
        'compute_scores_cached': o, 'evaluate_cached_on_device': n,
        'speedup_median': round(o['median_s'] / n['median_s'], 2),
        'faster_beyond_spread': bool(n['max_s'] < o['min_s']),
        'rank_file_of_device_ranks_equals_host_ranks_of_same_scores': same_file,
        'rank_lines_equal_between_passes': [same_lines, len(old_lines)],
        'metrics_old': [float(v) for v in old_metrics] if old_metrics else None, 'metrics_new': list(new_metrics),
        'rows_per_pass_sweep': sweep, 'device': torch.cuda.get_device_name(0),
    }
    line = json.dumps(result)
    print(line)
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
