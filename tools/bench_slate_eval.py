"""The slate sweep at a size a user would run: util.evaluate_slates_on_device on the synthetic dev split of tools/bench_eval.py
(``--impressions`` impressions, MIND-like candidate counts) with a sweep of 8 selection settings -- plain, max_per_topic 1 / 2 / 3,
mmr_lambda 0.3 / 0.5 / 0.7, and max_per_topic 2 with mmr_lambda 0.5 -- at k = 10.  Timed, all in one process:
  * the scoring pass (evaluate_cached_on_device, return_scores), host clock around work that ends in a device synchronise;
  * per setting the selection (serving.select_segments) and the metrics call (ops.slate_metrics: lime_slate_metrics_f32's two launches);
  * beside the metrics call the SAME metrics composed in torch (gather, normalise, bmm, masked means), the two alternated
    ``--rounds`` times on the same slates; medians and spread; the two results are compared;
  * the whole entry with the 8 settings against the scoring pass alone: what a sweep costs on top of the pass.
Prints one JSON line; ``--json-out`` also writes it to a file.

    python tools/bench_slate_eval.py --impressions 50000 --rounds 5 --json-out profiles/slate_eval.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bench_eval import make_dev_split, say, spread, timed  # noqa: E402
from lime_cikm25_amd import DeviceCorpus, Model, evaluate, make_config, ops, serving, synth, util  # noqa: E402
from lime_cikm25_amd.device_data import topic_table_of  # noqa: E402

SETTINGS = [{}, {'max_per_topic': 1}, {'max_per_topic': 2}, {'max_per_topic': 3}, {'mmr_lambda': 0.3}, {'mmr_lambda': 0.5}, {'mmr_lambda': 0.7},
            {'max_per_topic': 2, 'mmr_lambda': 0.5}]


def torch_slate_means(positions, k, offsets, news, labels, skip, value, table, keys, disc):
    """The eight means of ops.slate_metrics composed of torch operators -> fp64 [8] on the device (the yardstick of the kernel's time;
    its sums are torch's, in torch's order)."""
    beg, length = offsets[:-1], offsets[1:] - offsets[:-1]
    pos = positions[:, :k].long()
    filled = (pos >= 0) & (pos < length[:, None])
    row = torch.where(filled, beg[:, None] + pos, torch.zeros_like(pos))
    nid = news[row].long()
    filled &= (nid >= 0) & (nid < table.shape[0])
    nid = torch.where(filled, nid, torch.zeros_like(nid))
    m = filled.sum(1)
    live = skip == 0
    # relevance
    run = torch.cat([labels.new_zeros(1, dtype=torch.int64), (labels != 0).long().cumsum(0)])
    n_pos = run[offsets[1:]] - run[offsets[:-1]]
    counted = live & (n_pos > 0) & (n_pos < length)
    gain = (filled & (labels[row] != 0)).double()
    ideal = torch.cat([disc.new_zeros(1), disc[:k].cumsum(0)])[n_pos.clamp(max=k)]
    ndcg = (gain * disc[:k]).sum(1) / ideal
    rr = (gain / torch.arange(1, k + 1, device=gain.device, dtype=torch.float64)).max(1).values
    hit = gain.max(1).values
    recall = gain.sum(1) / n_pos
    rel = torch.stack([ndcg, rr, hit, recall], 1)[counted].sum(0) / counted.sum()
    # diversity
    unit = torch.nn.functional.normalize(table[nid] * filled.unsqueeze(2), dim=2, eps=0.0).nan_to_num_(0.0)
    cos = torch.bmm(unit, unit.transpose(1, 2)).double()
    upper = torch.triu(torch.ones((k, k), dtype=torch.bool, device=cos.device), 1)
    pairs = (m * (m - 1) // 2).double()
    ild = 1.0 - (cos * upper).sum((1, 2)) / pairs
    two = live & (m >= 2)
    ild = ild[two].sum() / two.sum()
    key = torch.where(filled, keys[nid].long(), torch.full_like(nid, 1 << 40)).sort(1).values
    distinct = ((key[:, 1:] != key[:, :-1]) & (key[:, 1:] < (1 << 40))).sum(1) + (key[:, 0] < (1 << 40)).long()
    one = live & (m >= 1)
    mean_value = (value[row].double() * filled).sum(1) / m
    rest = torch.stack([distinct.double(), m.double(), mean_value], 1)[one].sum(0) / one.sum()
    return torch.cat([rel, ild.reshape(1), rest])


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def ms(xs):
    return {'median_ms': round(statistics.median(xs), 4), 'min_ms': round(min(xs), 4), 'max_ms': round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--impressions', type=int, default=50000)
    ap.add_argument('--news', type=int, default=20000)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5, help='calls per round and side')
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--json-out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_slate_eval.py measures on the GPU: there is no CPU path'
    k = args.k

    cfg = make_config(vocabulary_size=50000)
    corpus = synth.synth_corpus(cfg, n_news=args.news, n_train=1, n_dev=1, seed=args.seed)
    dc = DeviceCorpus(corpus)
    beh, indices, labels, counts = make_dev_split(cfg, dc, args.impressions, args.news, args.seed)
    say('dev split: %d impressions, %d rows' % (len(labels), beh.num))
    model = Model(cfg)
    model.initialize()
    synth.fill_state_dict(model, seed=args.seed)
    model = model.cuda().eval()
    per = cfg.batch_size

    def score_pass():
        return util.evaluate_cached_on_device(model, beh, indices, labels, rows_per_forward=per, return_scores=True)

    def sweep():
        return util.evaluate_slates_on_device(model, beh, indices, labels, SETTINGS, k=k, value='remaining', rows_per_forward=per)

    dt, (metrics, scores) = timed(score_pass)                               # warm-up of both entries
    say('scoring pass (warm-up): %.2f s' % dt)
    dt, (m2, results) = timed(sweep)
    say('sweep (warm-up): %.2f s' % dt)
    assert m2 == metrics
    pass_t, sweep_t = [], []
    for r in range(args.rounds):                                            # alternated
        pass_t.append(timed(score_pass)[0])
        sweep_t.append(timed(sweep)[0])
        say('round %d: pass %.3f s, pass + sweep of %d settings %.3f s' % (r + 1, pass_t[-1], len(SETTINGS), sweep_t[-1]))

    # the pieces of a setting on the pass's scores
    cache = model.build_news_cache(dc)
    off32, row_labels, skip = evaluate.impression_layout(indices, labels)
    offsets = torch.from_numpy(off32.astype(np.int64)).cuda()
    d_labels, d_skip = torch.from_numpy(row_labels).cuda(), torch.from_numpy(skip).cuda()
    cand = beh.cand_index.reshape(-1)
    news = cand.to(torch.int32).contiguous()
    value = (beh.cand_lifetime - beh.cand_freshness).reshape(-1).float().contiguous()
    table = serving.content_columns(model, cache)
    keys, cat_t, _ = topic_table_of(dc, 'category')
    disc = torch.from_numpy(1.0 / np.log2(np.arange(128) + 2.0)).cuda()
    per_setting = []
    for setting, res in zip(SETTINGS, results):
        quota = serving.topic_quota(dc, setting.get('max_per_topic'), 'category')
        div = serving.diversity(model, cache, k, setting.get('mmr_lambda'), None, None)
        select = lambda: serving.select_segments(scores, offsets, None, quota, div, cand, k)
        kernel = lambda: ops.slate_metrics(positions, k, offsets, news, d_labels, d_skip, value, table, keys, n_keys=cat_t.numel())
        composed = lambda: torch_slate_means(positions, k, offsets, news, d_labels, d_skip, value, table, keys, disc)
        positions, _ = select()
        got, want = kernel(), composed()
        means = torch.cat([got.sums[:4] / got.counts[0], got.sums[4:5] / got.counts[1], got.sums[5:] / got.counts[2]])
        apart = float((means - want).abs().max())
        sel_ms, ker_ms, tor_ms = [], [], []
        for _ in range(args.rounds):                                        # alternated: selection, kernel, torch
            sel_ms += [event_ms(select)[0] for _ in range(args.reps)]
            ker_ms += [event_ms(kernel)[0] for _ in range(args.reps)]
            tor_ms += [event_ms(composed)[0] for _ in range(args.reps)]
        entry = {'setting': setting, 'selection': ms(sel_ms), 'slate_metrics': ms(ker_ms), 'torch_composition': ms(tor_ms),
                 'torch_over_kernel_median': round(statistics.median(tor_ms) / statistics.median(ker_ms), 2),
                 'kernel_faster_beyond_spread': bool(max(ker_ms) < min(tor_ms)), 'means_apart': apart,
                 'result': {name: res[name] for name in ('ndcg', 'rr', 'hit', 'recall', 'ild', 'topics', 'filled', 'value', 'n_relevance',
                                                         'n_diversity', 'n_slates')}}
        per_setting.append(entry)
        say('%s: selection %.3f ms, slate_metrics %.3f ms, torch %.3f ms (x%.1f); means apart %.2e; nDCG@%d %.4f ILD %.4f topics %.2f' % (
            setting, entry['selection']['median_ms'], entry['slate_metrics']['median_ms'], entry['torch_composition']['median_ms'],
            entry['torch_over_kernel_median'], apart, k, res['ndcg'], res['ild'], res['topics']))

    p, s = spread(pass_t), spread(sweep_t)
    result = {
        'bench': 'slate_eval', 'impressions': len(labels), 'rows': beh.num, 'news': args.news, 'k': k, 'similarity_columns': int(table.shape[1]),
        'rows_per_forward': per, 'rounds': args.rounds, 'reps': args.reps, 'settings': len(SETTINGS),
        'scoring_pass': p, 'pass_and_sweep': s,
        'sweep_over_pass_median': round((s['median_s'] - p['median_s']) / p['median_s'], 4),
        'pass_metrics': list(metrics), 'per_setting': per_setting, 'device': torch.cuda.get_device_name(0),
    }
    line = json.dumps(result)
    print(line)
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
