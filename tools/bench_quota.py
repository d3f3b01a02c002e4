"""What a topic quota costs at a size a user would serve: Model.recommend with ``max_per_topic=2`` against the same call without it,
alternated in one process after warm-up, and the bare selection -- lime_topk_rows_quota_f32 -- against lime_topk_rows_f32 on the same
scores, each repeated ``--inner`` times between two device events (one selection is tens of microseconds).

32 users, H = 50, the full-size model with synthetic weights, pools of 2,000 and 65,536 synthetic news over MIND's topic counts
(18 categories, 270 subcategories), k = 10, quota by category.  The selection is timed on three sets of scores: the model's own; those
with the quota binding nowhere (quota = k); and a crowded row -- one category owns the 300 best scores of every chunk of 4096, the
walk's worst case.  Device-event medians.  Prints one JSON line per pool and writes them to ``--json-out`` (default
profiles/recommend_quota.json).

    python tools/bench_quota.py --rounds 5
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from lime_cikm25_amd import DeviceCorpus, Model, make_config, ops, recommend, synth  # noqa: E402
from lime_cikm25_amd.device_data import topic_table_of  # noqa: E402


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def event_ms(fn, inner=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner, out


def stat(v):
    return {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4)}


def alternate(forms, rounds, inner=1):
    """{name: fn} alternated after two warm-up rounds -> ({name: [ms per call]}, {name: last result})."""
    for _ in range(2):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms, out = {name: [] for name in forms}, {}
    for _ in range(rounds):
        for name, fn in forms.items():
            dt, out[name] = event_ms(fn, inner)
            ms[name].append(dt)
    return ms, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=32)
    ap.add_argument('--pools', type=int, nargs='*', default=[2000, 65536])
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--quota', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--inner', type=int, default=200, help='selections between two device events')
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--json-out', default=os.path.join(ROOT, 'profiles', 'recommend_quota.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_quota.py measures on the GPU: there is no CPU path'

    cfg = make_config()
    U, H, k, q = args.users, cfg.max_history_num, args.k, args.quota
    n_news = max(args.pools) + 1
    corpus = synth.synth_corpus(cfg, n_news=n_news, n_train=1, n_dev=1, seed=args.seed)
    # MIND's subcategories each sit under one category: about 270 topics in all (independent draws would give 18 x 270)
    corpus.news_category[1:] = 1 + corpus.news_subCategory[1:] % (cfg.category_num - 1)
    dc = DeviceCorpus(corpus)
    model = Model(cfg)
    model.initialize()
    synth.fill_state_dict(model, seed=args.seed)
    model = model.cuda().eval()
    cache = model.build_news_cache(dc)
    torch.cuda.synchronize()
    say('corpus of %d news, cache %s' % (n_news, tuple(cache.shape)))

    rng = np.random.default_rng(args.seed)
    n_hist = rng.integers(5, H + 1, size=U)
    mask = np.arange(H)[None, :] < n_hist[:, None]
    hist = np.where(mask, rng.integers(1, n_news, size=(U, H)), 0).astype(np.int32)
    ufr = np.where(mask, np.exp(rng.uniform(np.log(60.0), np.log(30 * 86400.0), size=(U, H))), 0.0).astype(np.float32)
    ult = np.where(mask, np.exp(rng.uniform(np.log(600.0), np.log(14 * 86400.0), size=(U, H))), 0.0).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    topic_of_news, cat_t, _ = topic_table_of(dc, 'category')
    lines = []
    for C in args.pools:
        pool = rng.permutation(np.arange(1, n_news))[:C].astype(np.int32)
        cfr = np.exp(rng.uniform(np.log(60.0), np.log(3 * 86400.0), size=C)).astype(np.float32)
        clt = (cfr[None, :] * np.exp(rng.uniform(-1.0, 1.0, size=(U, C)))).astype(np.float32)
        pool_args = dict(news_cache=cache, corpus=dc, hist_index=t(hist), hist_mask=t(mask), user_freshness=t(ufr), user_lifetime=t(ult),
                         cand_index=t(pool), cand_freshness=t(cfr), cand_lifetime=t(clt))
        n_src = min(U * C, H + cfg.batch_size)
        # the whole call, with and without the quota
        ms, out = alternate({'plain': lambda: model.recommend(**pool_args, k=k, n_src=n_src),
                             'quota': lambda: model.recommend(**pool_args, k=k, n_src=n_src, max_per_topic=q)}, args.rounds)
        scores = model.score_pool(**pool_args, n_src=n_src)
        keys = topic_of_news[t(pool).long()]
        n_keys = cat_t.numel()
        want = recommend.quota_topk(scores.cpu().numpy(), keys.cpu().numpy(), k, q)
        assert np.array_equal(out['quota'][0].cpu().numpy(), want[0]), 'the quota slate is not the host walk\'s'
        plain_pos = out['plain'][0].cpu().numpy()
        crowd = [int(np.bincount(keys.cpu().numpy()[plain_pos[u]]).max()) for u in range(U)]
        changed = float((out['quota'][0] != out['plain'][0]).any(dim=1).float().mean())
        # the bare selection on the model's scores, with a quota that binds nowhere, and on crowded rows
        hard = torch.rand((U, C), device='cuda')
        hard_keys = torch.randint(1, n_keys, (C,), dtype=torch.int32, device='cuda')
        for c0 in range(0, C, 4096):
            at = c0 + torch.randperm(min(4096, C - c0), device='cuda')[:300]
            hard[:, at] += 2.0
            hard_keys[at] = 0
        sel, _ = alternate({'topk_rows': lambda: ops.topk_rows(scores, k),
                            'quota': lambda: ops.topk_rows_quota(scores, keys, q, k, n_keys=n_keys),
                            'quota_loose': lambda: ops.topk_rows_quota(scores, keys, k, k, n_keys=n_keys),
                            'topk_rows_crowded': lambda: ops.topk_rows(hard, k),
                            'quota_crowded': lambda: ops.topk_rows_quota(hard, hard_keys, q, k, n_keys=n_keys)}, args.rounds, args.inner)
        med = {name: statistics.median(v) for name, v in sel.items()}
        line = {'bench': 'recommend_quota', 'model': model.model_name, 'users': U, 'H': H, 'pool': C, 'k': k, 'max_per_topic': q,
                'quota_by': 'category', 'groups': n_keys, 'rounds': args.rounds,
                'recommend_ms': stat(ms['plain']), 'recommend_quota_ms': stat(ms['quota']),
                'quota_over_plain': round(statistics.median(ms['quota']) / statistics.median(ms['plain']), 4),
                'users_whose_slate_changed': round(changed, 4), 'largest_group_in_a_plain_slate': max(crowd),
                'selection_inner': args.inner, 'selection_ms': {name: stat(v) for name, v in sel.items()},
                'selection_quota_over_topk': round(med['quota'] / med['topk_rows'], 3),
                'selection_loose_over_topk': round(med['quota_loose'] / med['topk_rows'], 3),
                'selection_crowded_quota_over_topk': round(med['quota_crowded'] / med['topk_rows_crowded'], 3),
                'device': torch.cuda.get_device_name(0)}
        say(line)
        lines.append(json.dumps(line))
    print('\n'.join(lines))
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
