"""lime_cached_occurrence_f32 and the cached dev pass of every fusion method, measured on the GPU from seeded synthetic data.

  --parts kernel   the kernel alone: R = 8192 * 51 occurrences of 20,000 news, D = 400 ('concat') and D = 900 ('add', 'gated'); device
                   events around each launch; algorithmic bytes 12 + 4 D (rows read + 1 written) an occurrence (table rows counted as
                   read) -> GB/s and the share of the 8 TB/s HBM figure, which bounds it.  For KERNEL time run this part under
                   ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_occurrence.py --parts kernel``
                   in a run of its own and hand the directory to a later run with ``--kernel-trace-dir DIR``.
  --parts concat   the default configuration on the split of profiles/device_eval.json (tools/bench_eval.py:make_dev_split, 50,000
                   impressions): util.evaluate_cached_on_device with LIME_FUSED_OCCURRENCE off and on, alternated; one score_behaviors
                   pass of 8192 rows both ways with its peak bytes a row; rel_err of the scores between the two.
  --parts fusion   'add' and 'gated': the cached device pass against util.compute_scores (the only pass these methods had), alternated,
                   on ``--fusion-impressions`` impressions; rel_err of the scores between the two passes.
Prints one JSON line; ``--json-out`` also writes it to a file.

    python tools/bench_occurrence.py --json-out profiles/cached_occurrence.json
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bench_eval import log_uniform, make_dev_split, say, spread, timed  # noqa: E402
from lime_cikm25_amd import DeviceCorpus, Model, formats, make_config, ops, synth, util  # noqa: E402

HBM_PEAK = 8.0e12               # bytes / s, MI355X


def rel_err(a, b):
    """tests/helpers.py rel_err: max |a - b| / max(|b|, mean |b| over the non-zero entries)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nz = np.abs(b[b != 0])
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), float(nz.mean()) if nz.size else 1.0)))


def occurrence_bytes(D, gated):
    return 12 + 4 * D * ((4 if gated else 2) + 1)


def kernel_part(args):
    R, n = 8192 * 51, args.news
    out = {'occurrences': R, 'news': n, 'iters': args.iters, 'cases': []}
    idx = torch.from_numpy(synth.randint('occ.idx', args.seed, R, 0, n).astype(np.int32)).cuda()
    fr = torch.from_numpy(log_uniform('occ.fr', args.seed, R, 60.0, 30 * 86400.0).astype(np.float32)).cuda()
    lt = torch.from_numpy(log_uniform('occ.lt', args.seed, R, 600.0, 14 * 86400.0).astype(np.float32)).cuda()
    g = torch.Generator().manual_seed(args.seed)
    for mode, D in (('concat', 400), ('add', 900), ('gated', 900)):
        gated = mode == 'gated'
        cache = torch.randn(n, 2 * D if gated else D, generator=g).cuda()
        A, P = (cache[:, :D], cache[:, D:]) if gated else (cache, None)
        T = torch.randn(100, D, generator=g).cuda()
        Q = torch.randn(100, D, generator=g).cuda() if gated else None
        dst = torch.empty(R, D, device='cuda')
        run = lambda: ops.cached_occurrence(mode, idx, fr, lt, A, T, P, Q, out=dst)
        for _ in range(3):
            run()
        ms = []
        for _ in range(args.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        nbytes = R * occurrence_bytes(D, gated)
        med = statistics.median(ms)
        case = {'mode': mode, 'D': D, 'bytes_per_occurrence': occurrence_bytes(D, gated), 'bytes': nbytes,
                'event_ms': {'median': round(med, 4), 'min': round(min(ms), 4), 'max': round(max(ms), 4)},
                'event_GBps': round(nbytes / (med * 1e-3) / 1e9, 1), 'event_share_of_hbm_peak': round(nbytes / (med * 1e-3) / HBM_PEAK, 3)}
        say('kernel %s D=%d: %.3f ms (events), %.0f GB/s, %.1f %% of 8 TB/s' % (mode, D, med, case['event_GBps'], 100 * case['event_share_of_hbm_peak']))
        out['cases'].append(case)
        del cache, A, P, T, Q, dst
    return out


def merge_kernel_trace(kernel, trace_dir):
    """Kernel times of a separate ``rocprofv3 --kernel-trace --stats --output-format csv`` run of ``--parts kernel`` into the cases:
    the median over the dispatches of each (instantiation, grid size) in the run's kernel_trace.csv."""
    ns = {}
    for path in glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True):
        for r in csv.DictReader(open(path)):
            if 'cached_occurrence_kernel' in r['Kernel_Name']:
                key = ('<true>' in r['Kernel_Name'], int(r['Grid_Size_X']))
                ns.setdefault(key, []).append(int(r['End_Timestamp']) - int(r['Start_Timestamp']))
    R = kernel['occurrences']
    for case in kernel['cases']:
        threads = (R * (case['D'] // 4) + 255) // 256 * 256
        t = ns.get((case['mode'] == 'gated', threads)) or ns.get((case['mode'] == 'gated', threads // 256))
        if not t:
            continue
        med = statistics.median(t)
        case['trace_us'] = {'median': round(med / 1e3, 1), 'min': round(min(t) / 1e3, 1), 'max': round(max(t) / 1e3, 1), 'dispatches': len(t)}
        case['trace_GBps'] = round(case['bytes'] / (med * 1e-9) / 1e9, 1)
        case['trace_share_of_hbm_peak'] = round(case['bytes'] / (med * 1e-9) / HBM_PEAK, 3)


def build(cfg, n_news, n_imp, seed):
    corpus = synth.synth_corpus(cfg, n_news=n_news, n_train=1, n_dev=1, seed=seed)
    dc = DeviceCorpus(corpus)
    beh, indices, labels, counts = make_dev_split(cfg, dc, n_imp, n_news, seed)
    model = Model(cfg)
    model.initialize()
    synth.fill_state_dict(model, seed=seed)
    return dc, beh, indices, labels, model.cuda().eval()


def one_score_pass(model, beh, cache, rows, per):
    model.score_behaviors(beh, rows, cache, n_src=per)
    dt, _ = timed(lambda: model.score_behaviors(beh, rows, cache, n_src=per))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    model.score_behaviors(beh, rows, cache, n_src=per)
    torch.cuda.synchronize()
    peak = int(torch.cuda.max_memory_allocated() - base)
    return {'rows': int(rows.numel()), 'ms': round(dt * 1e3, 3), 'peak_bytes': peak, 'peak_bytes_per_row': round(peak / max(1, rows.numel()))}


def concat_part(args):
    cfg = make_config(vocabulary_size=50000)
    dc, beh, indices, labels, model = build(cfg, args.news, args.impressions, args.seed)
    per, rpp = cfg.batch_size, util.DEVICE_EVAL_ROWS_PER_PASS
    say('concat: %d impressions, %d rows' % (len(labels), beh.num))

    def device_pass(flag, **kw):
        ops.FUSED_OCCURRENCE = flag
        try:
            return util.evaluate_cached_on_device(model, beh, indices, labels, rows_per_forward=per, rows_per_pass=rpp, **kw)
        finally:
            ops.FUSED_OCCURRENCE = False

    scores = {}
    for flag in (False, True):                                   # warm-up of both forms, and their scores
        dt, (_, s) = timed(lambda: device_pass(flag, return_scores=True))
        scores[flag] = s.cpu().numpy()
        say('concat warm-up, flag %s: %.2f s' % (flag, dt))
    t = {False: [], True: []}
    for r in range(args.rounds):
        for flag in (False, True):
            dt, _ = timed(lambda: device_pass(flag))
            t[flag].append(dt)
            say('concat round %d, flag %s: %.3f s' % (r + 1, flag, dt))
    cache = model.build_news_cache(dc)
    rows = torch.arange(min(rpp // per * per, beh.num), device='cuda')
    one = {}
    for flag in (False, True):
        ops.FUSED_OCCURRENCE = flag
        one['on' if flag else 'off'] = one_score_pass(model, beh, cache, rows, per)
        ops.FUSED_OCCURRENCE = False
    off, on = spread(t[False]), spread(t[True])
    gain = off['median_s'] - on['median_s']
    spreads = (off['max_s'] - off['min_s']) + (on['max_s'] - on['min_s'])
    return {'impressions': len(labels), 'rows': beh.num, 'news': args.news, 'rows_per_forward': per, 'rows_per_pass': rpp, 'rounds': args.rounds,
            'evaluate_cached_on_device_flag_off': off, 'evaluate_cached_on_device_flag_on': on,
            'median_gain_s': round(gain, 4), 'two_spreads_s': round(spreads, 4), 'faster_by_more_than_the_two_spreads': bool(gain > spreads),
            'one_score_behaviors_pass': one, 'scores_rel_err_on_vs_off': rel_err(scores[True], scores[False])}


def fusion_part(args):
    out = {}
    for fusion in ('add', 'gated'):
        cfg = make_config(vocabulary_size=50000, fusion_method=fusion)
        dc, beh, indices, labels, model = build(cfg, args.news, args.fusion_impressions, args.seed)
        per = cfg.batch_size
        tmp = tempfile.mkdtemp(prefix='bench_occurrence_')
        truth = formats.write_truth_file(os.path.join(tmp, 'truth.txt'), labels)
        rows = list(range(beh.num))
        say('%s: %d impressions, %d rows' % (fusion, len(labels), beh.num))

        def uncached():
            batches = (beh.assemble(rows[i:i + per]) for i in range(0, len(rows), per))
            return util.compute_scores(model, batches, indices, os.path.join(tmp, 'uncached.txt'), truth)

        def cached(**kw):
            return util.evaluate_cached_on_device(model, beh, indices, labels, result_file=os.path.join(tmp, 'cached.txt'), rows_per_forward=per, **kw)

        # the uncached scores, which compute_scores keeps to itself: its own loop, once, outside the timed windows (and its warm-up)
        ref = []
        with torch.no_grad():
            for i in range(0, len(rows), per):
                b = beh.assemble(rows[i:i + per])
                ref.append(model(*b, b[24] - b[23]).squeeze(1).float().cpu())
        ref = torch.cat(ref).numpy()
        dt, (m_cached, s) = timed(lambda: cached(return_scores=True))
        say('%s warm-up, cached device pass: %.2f s' % (fusion, dt))
        t_un, t_ca, m_un = [], [], None
        for r in range(args.fusion_rounds):
            dt, m_un = timed(uncached)
            t_un.append(dt)
            say('%s round %d: compute_scores %.2f s' % (fusion, r + 1, dt))
            dt, _ = timed(cached)
            t_ca.append(dt)
            say('%s round %d: evaluate_cached_on_device %.3f s' % (fusion, r + 1, dt))
        un, ca = spread(t_un), spread(t_ca)
        same = sum(1 for a, b in zip(open(os.path.join(tmp, 'uncached.txt')).read().split('\n'), open(os.path.join(tmp, 'cached.txt')).read().split('\n')) if a == b)
        out[fusion] = {'impressions': len(labels), 'rows': beh.num, 'news': args.news, 'rows_per_forward': per, 'rounds': args.fusion_rounds,
                       'compute_scores': un, 'evaluate_cached_on_device': ca, 'ratio_median': round(un['median_s'] / ca['median_s'], 1),
                       'scores_rel_err_cached_vs_uncached': rel_err(s.cpu().numpy(), ref), 'rank_lines_equal_between_passes': [same, len(labels)],
                       'metrics_uncached': [float(v) for v in m_un], 'metrics_cached': [float(v) for v in m_cached]}
        del dc, beh, model
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='kernel,concat,fusion')
    ap.add_argument('--news', type=int, default=20000)
    ap.add_argument('--impressions', type=int, default=50000)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--fusion-impressions', type=int, default=2000)
    ap.add_argument('--fusion-rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--kernel-trace-dir', default=None)
    ap.add_argument('--json-out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_occurrence.py measures on the GPU: there is no CPU path'
    parts = args.parts.split(',')
    result = {'bench': 'cached_occurrence', 'device': torch.cuda.get_device_name(0), 'hbm_peak_Bps': HBM_PEAK, 'seed': args.seed}
    if 'kernel' in parts:
        result['kernel'] = kernel_part(args)
        if args.kernel_trace_dir:
            merge_kernel_trace(result['kernel'], args.kernel_trace_dir)
    if 'concat' in parts:
        result['concat'] = concat_part(args)
    if 'fusion' in parts:
        result['fusion'] = fusion_part(args)
    line = json.dumps(result)
    print(line)
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
