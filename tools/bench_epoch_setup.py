"""The set-up phase of a training epoch at a size a user would run, both ways in one process: the host path of Trainer.train_epoch
(device_data.negative_sampling + DeviceBehaviors.from_train: a Python loop over every record, the fixed tables re-padded, re-stacked
and copied to the device again) against the resident path (DeviceBehaviors.train_resident once, then resample(seed, epoch): one launch
of lime_negative_sample into tables that keep their addresses).

A synthetic train split from a seed (lime_cikm25_amd.synth), built directly as arrays: ``--records`` records with 1 .. 71 non-clicked
news each, H = config.max_history_num (50), K = config.negative_sample_num (4).  Timed:
  * --parts setup   the two set-ups, alternated ``--rounds`` times (host clock around work that ends in a device synchronise); medians
                    and min .. max; the host path split into its two halves; after every set-up the FIRST batch's assemble (the host
                    path has thrown the plans away with the old DeviceBehaviors, the resident path kept them); once, the resident tables
                    against from_train(counter_negative_sampling(...)), bit for bit.
  * --parts kernel  the launch alone: device events around each resample; algorithmic bytes from the shapes (per record 20 read, 12 (1 + K)
                    written, 8 K gathered) -> GB/s.  For KERNEL time run this part under
                    ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_epoch_setup.py --parts kernel``
                    in a run of its own and hand the directory to a later run with ``--kernel-trace-dir DIR``.
The yardstick is the host path in the same run.  Prints one JSON line; ``--json-out`` also writes it to a file.

    python tools/bench_epoch_setup.py --json-out profiles/epoch_setup.json
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bench_eval import log_uniform, say, spread, timed  # noqa: E402
from lime_cikm25_amd import DeviceBehaviors, DeviceCorpus, make_config, synth  # noqa: E402
from lime_cikm25_amd.device_data import counter_negative_sampling, negative_sampling  # noqa: E402

HBM_PEAK = 8.0e12               # bytes / s, MI355X


def sample_bytes(N, K):
    """What the launch has to move: per record its two offsets' share, positive index, positive lifetime and freshness (8 + 12 bytes),
    three rows of 1 + K four-byte entries written, K (index, lifetime) pairs gathered."""
    return N * (20 + 12 * (1 + K) + 8 * K) + 8


def make_train_records(cfg, N, n_news, seed, lo=1, hi=71):
    """``N`` records in the layout of Corpus.train_behaviors (corpus.py:539-552), generated as arrays and cut into the per-record lists
    the host path reads."""
    H = cfg.max_history_num
    counts = synth.randint('train.nn', seed, N, lo, hi + 1)
    nnz = int(counts.sum())
    starts = np.cumsum(counts) - counts
    neg = synth.randint('train.neg', seed, nnz, 1, n_news).tolist()
    neg_lt = log_uniform('train.neglt', seed, nnz, 600.0, 14 * 86400.0).astype(np.float32).astype(np.float64).tolist()
    n_hist = synth.randint('train.hn', seed, N, 0, H + 1)
    mask = np.arange(H)[None, :] < n_hist[:, None]
    hist = np.where(mask, synth.randint('train.h', seed, N * H, 1, n_news).reshape(N, H), 0).astype(np.int32)
    fr = log_uniform('train.fr', seed, N * H, 60.0, 30 * 86400.0).reshape(N, H)
    lt = log_uniform('train.lt', seed, N * H, 600.0, 14 * 86400.0).reshape(N, H)
    uid = synth.randint('train.uid', seed, N, 0, cfg.user_num).tolist()
    pos = synth.randint('train.pos', seed, N, 1, n_news).tolist()
    cfr = log_uniform('train.cfr', seed, N, 60.0, 30 * 86400.0).tolist()
    plt = log_uniform('train.plt', seed, N, 600.0, 14 * 86400.0).tolist()
    out = []
    for i, (s, c, h) in enumerate(zip(starts.tolist(), counts.tolist(), n_hist.tolist())):
        out.append([uid[i], hist[i], mask[i], pos[i], neg[s:s + c], i, cfr[i], plt[i], neg_lt[s:s + c], fr[i, :h].tolist(), lt[i, :h].tolist()])
    return out, counts


def kernel_part(args, resident, N, K):
    for e in range(3):
        resident.resample(args.seed, e)
    ms = []
    for e in range(args.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        resident.resample(args.seed, 100 + e)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    med, nbytes = statistics.median(ms), sample_bytes(N, K)
    out = {'records': N, 'K': K, 'iters': args.iters, 'bytes': nbytes, 'bytes_per_record': 20 + 12 * (1 + K) + 8 * K,
           'event_ms': {'median': round(med, 4), 'min': round(min(ms), 4), 'max': round(max(ms), 4)},
           'event_GBps': round(nbytes / (med * 1e-3) / 1e9, 1)}
    say('lime_negative_sample, %d records: %.4f ms (events around the call), %.0f GB/s' % (N, med, out['event_GBps']))
    return out


def merge_kernel_trace(kernel, trace_dir):
    """Kernel times of a separate ``rocprofv3 --kernel-trace --stats --output-format csv`` run of ``--parts kernel``: the median over the
    dispatches of negative_sample_kernel in the run's kernel_trace.csv."""
    ns = []
    for path in glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True):
        for r in csv.DictReader(open(path)):
            if 'negative_sample_kernel' in r['Kernel_Name']:
                ns.append(int(r['End_Timestamp']) - int(r['Start_Timestamp']))
    if not ns:
        return
    med = statistics.median(ns)
    kernel['trace_us'] = {'median': round(med / 1e3, 2), 'min': round(min(ns) / 1e3, 2), 'max': round(max(ns) / 1e3, 2), 'dispatches': len(ns)}
    kernel['trace_GBps'] = round(kernel['bytes'] / (med * 1e-9) / 1e9, 1)
    kernel['trace_share_of_hbm_peak'] = round(kernel['bytes'] / (med * 1e-9) / HBM_PEAK, 4)
    kernel['bound'] = 'bytes over HBM bandwidth (integer hashing only: no floating-point work to count)'


def setup_part(args, cfg, corpus, dc, resident, N, K):
    beh = corpus.train_behaviors
    B = cfg.batch_size
    order = np.random.RandomState(args.seed).permutation(N)
    rows = [int(r) for r in order[:B]]

    def host_setup():
        t0 = time.perf_counter()
        samples = negative_sampling(beh, K)
        t1 = time.perf_counter()
        train = DeviceBehaviors.from_train(dc, corpus, *samples)
        torch.cuda.synchronize()
        return train, t1 - t0, time.perf_counter() - t1

    def first_batch(train):
        return timed(lambda: train.assemble(rows))[0]

    # warm-up of everything the timed windows use: both set-ups once, a batch of this size through both (the resident split builds
    # its plans HERE, in its "first epoch", and keeps them)
    np.random.seed(args.seed)
    train, _, _ = host_setup()
    first_batch(train)
    del train
    resident.resample(args.seed, 1)
    first_batch(resident)
    first_batch(resident)

    # once: the resident tables against the host twin's, bit for bit
    twin = DeviceBehaviors.from_train(dc, corpus, *counter_negative_sampling(beh, K, args.seed, 1))
    same = all(torch.equal(getattr(resident, n), getattr(twin, n)) for n in
               ('user_id', 'hist_index', 'hist_mask', 'user_freshness', 'user_lifetime', 'cand_index', 'cand_freshness', 'cand_lifetime'))
    say('resident tables == from_train(counter_negative_sampling): %s' % same)
    del twin

    host_t, host_ns, host_ft, dev_t, host_fb, dev_fb = [], [], [], [], [], []
    for r in range(args.rounds):
        dt, (train, t_ns, t_ft) = timed(host_setup)
        host_t.append(dt)
        host_ns.append(t_ns)
        host_ft.append(t_ft)
        host_fb.append(first_batch(train))
        del train
        dt, _ = timed(lambda: resident.resample(args.seed, 2 + r))
        dev_t.append(dt)
        dev_fb.append(first_batch(resident))
        say('round %d: host set-up %.3f s (sampling %.3f + tables %.3f), first batch %.2f ms; resample %.3f ms, first batch %.2f ms' % (
            r + 1, host_t[-1], t_ns, t_ft, host_fb[-1] * 1e3, dev_t[-1] * 1e3, dev_fb[-1] * 1e3))
    ms = lambda xs: {'median_ms': round(statistics.median(xs) * 1e3, 4), 'min_ms': round(min(xs) * 1e3, 4), 'max_ms': round(max(xs) * 1e3, 4),
                     'runs_ms': [round(x * 1e3, 4) for x in xs]}
    h, d = spread(host_t), ms(dev_t)
    gain = h['median_s'] - d['median_ms'] * 1e-3
    spreads = (h['max_s'] - h['min_s']) + (d['max_ms'] - d['min_ms']) * 1e-3
    return {'rounds': args.rounds, 'batch_rows': B,
            'host_setup': h, 'host_negative_sampling': spread(host_ns), 'host_from_train': spread(host_ft),
            'host_us_per_record': round(h['median_s'] / N * 1e6, 2),
            'device_resample': d, 'device_us_per_record': round(d['median_ms'] * 1e3 / N, 5),
            'median_gain_s': round(gain, 4), 'two_spreads_s': round(spreads, 4), 'faster_by_more_than_the_two_spreads': bool(gain > spreads),
            'ratio_median': round(h['median_s'] / (d['median_ms'] * 1e-3), 1),
            'first_batch_assemble_plans_rebuilt': ms(host_fb), 'first_batch_assemble_plans_kept': ms(dev_fb),
            'resident_tables_equal_host_twin': bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='kernel,setup')
    ap.add_argument('--records', type=int, default=200000)
    ap.add_argument('--news', type=int, default=20000)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--kernel-trace-dir', default=None)
    ap.add_argument('--json-out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_epoch_setup.py measures on the GPU: there is no CPU path'
    parts = args.parts.split(',')

    cfg = make_config(vocabulary_size=50000)
    K, N = cfg.negative_sample_num, args.records
    corpus = synth.synth_corpus(cfg, n_news=args.news, n_train=1, n_dev=1, seed=args.seed)
    t0 = time.perf_counter()
    corpus.train_behaviors, counts = make_train_records(cfg, N, args.news, args.seed)
    say('train split: %d records, %d non-clicked news (1 .. %d a record), H = %d, K = %d, in %.1f s' % (
        N, int(counts.sum()), int(counts.max()), cfg.max_history_num, K, time.perf_counter() - t0))
    dc = DeviceCorpus(corpus)
    dt, resident = timed(lambda: DeviceBehaviors.train_resident(dc, corpus, K))
    say('train_resident (once a run): %.3f s' % dt)
    result = {'bench': 'epoch_setup', 'device': torch.cuda.get_device_name(0), 'seed': args.seed, 'records': N, 'news': args.news,
              'non_clicked_total': int(counts.sum()), 'non_clicked_per_record': [int(counts.min()), int(counts.max())],
              'H': cfg.max_history_num, 'K': K, 'hbm_peak_Bps': HBM_PEAK, 'train_resident_once_s': round(dt, 3)}
    if 'kernel' in parts:
        result['kernel'] = kernel_part(args, resident, N, K)
        if args.kernel_trace_dir:
            merge_kernel_trace(result['kernel'], args.kernel_trace_dir)
    if 'setup' in parts:
        result['setup'] = setup_part(args, cfg, corpus, dc, resident, N, K)
    line = json.dumps(result)
    print(line)
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
