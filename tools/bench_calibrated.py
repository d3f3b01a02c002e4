"""What a calibrated slate costs and what it buys, at a size a user would serve: the recommend entries with ``calibrate_lambda`` against
the same call without it and against the same selection as a torch composition on the device -- the entry's own scores and shortlist,
the history's topic distribution by a scatter-add over a dense [rows, groups] table, then a k-round loop of about a dozen launches a
round: the yardstick --, alternated in one process after warm-up.  The selection alone -- lime_calibrate_rows_f32 against that torch
loop on the same shortlist -- is repeated ``--inner`` times between two device events.  The kernel's picks are asserted equal to
``recommend.calibrated_select``'s on the rows whose fp64 gap exceeds twice the derived tolerance.  Also reported: the mean
miscalibration (KL of the history's topic mix against the slate's) and nDCG@10 of the plain and the calibrated slate, through
``util.evaluate_slates_on_device`` on tools/bench_eval.py's synthetic dev split.

32 users, H = 50, the full-size model with synthetic weights, k = 10, groups by category; Model.recommend over pools of 2,000 and
65,536 synthetic news with shortlists of 64 and 128; Model.recommend_schedule over 24 slots of the first pool; Model.recommend_lists
over 1,024 lists of 100.  Device-event medians.  Prints one JSON line per shape and writes them to ``--json-out`` (default
profiles/recommend_calibrated.json).

    python tools/bench_calibrated.py --rounds 5
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from lime_cikm25_amd import DeviceCorpus, Model, make_config, ops, recommend, serving, synth, util  # noqa: E402
from lime_cikm25_amd.device_data import topic_table_of  # noqa: E402
from bench_eval import make_dev_split  # noqa: E402
from bench_quota import alternate, say, stat  # noqa: E402


def tolerance(H, alpha, log_ulp=4.0):
    """The bound of DESIGN.md "Calibrated slates" on the fp32 kernel's error in a difference of two v (tests/calibrate_cases.py)."""
    u, L = 2.0 ** -24, math.log(1.0 / alpha)
    dp = 2.0 * max(H, 1)
    gain = dp + 4.0 + 4.0 * log_ulp * (1.0 + 1.0 / (math.e * L)) + 2.0 * (dp + 3.0) / L
    return 2.0 * (max(5.0, gain) + 2.0) * u


def torch_calibrated(top, ids, keys, n_keys, hist_keys, lam, alpha, k):
    """``recommend.calibrated_select`` (unit weights) as a torch composition on the device: top fp32 [R, M], ids int32 [R, M] (-1:
    none), hist_keys int32 [U, H] with row r reading r % U -> picks int32 [R, k]."""
    R, M = top.shape
    live = (ids >= 0) & torch.isfinite(top)
    rank = torch.arange(M, device=top.device).expand(R, M)
    first = torch.where(live, rank, M).min(dim=1, keepdim=True).values.clamp(max=M - 1)
    last = torch.where(live, rank, -1).max(dim=1, keepdim=True).values.clamp(min=0)
    s_last = top.gather(1, last)
    span = top.gather(1, first) - s_last
    rel = torch.where(live & (span != 0), (top - s_last) / span, torch.zeros_like(top))
    hk = hist_keys[torch.arange(R, device=top.device) % hist_keys.shape[0]].long()
    on = (hk >= 0) & (hk < n_keys)
    hist = torch.zeros((R, n_keys + 1), dtype=torch.float32, device=top.device).scatter_add_(1, torch.where(on, hk, n_keys), on.float())[:, :n_keys]
    p = hist / hist.sum(dim=1, keepdim=True).clamp_min(1.0)
    key = keys[ids.clamp(min=0).long()].long()
    grouped = live & (key >= 0) & (key < n_keys)
    key = key.clamp(0, n_keys - 1)
    pe = torch.where(grouped, p.gather(1, key), torch.zeros_like(top))
    has = pe > 0
    counts = torch.zeros((R, n_keys), dtype=torch.float32, device=top.device)
    open_ = live.clone()
    picks = torch.full((R, k), -1, dtype=torch.int32, device=top.device)
    neg, one = torch.full_like(top, float('-inf')), torch.ones_like(top)
    scale = 1.0 / math.log(1.0 / alpha)
    for t in range(k):
        ce = counts.gather(1, key)
        q1 = torch.where(has, (1.0 - alpha) * (ce + 1.0) / (t + 1.0) + alpha * pe, one)
        q0 = torch.where(has, (1.0 - alpha) * ce / (t + 1.0) + alpha * pe, one)
        v = lam * rel + (1.0 - lam) * pe * (torch.log(q1) - torch.log(q0)) * scale
        best = torch.where(open_, v, neg).argmax(dim=1, keepdim=True)
        took = open_.any(dim=1, keepdim=True)
        picks[:, t:t + 1] = torch.where(took, best, -1).int()
        open_.scatter_(1, best, False)
        counts.scatter_add_(1, key.gather(1, best), (took & grouped.gather(1, best)).float())
    return picks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=32)
    ap.add_argument('--pools', type=int, nargs='*', default=[2000, 65536])
    ap.add_argument('--shortlists', type=int, nargs='*', default=[64, 128])
    ap.add_argument('--slots', type=int, default=24)
    ap.add_argument('--lists', type=int, nargs=2, default=[1024, 100], help='lists and candidates per list')
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--lam', type=float, default=0.1)
    ap.add_argument('--alpha', type=float, default=recommend.CALIBRATE_ALPHA)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--inner', type=int, default=50, help='selections between two device events')
    ap.add_argument('--impressions', type=int, default=5000, help='impressions of the synthetic dev split of the sweep (0: no sweep)')
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--json-out', default=os.path.join(ROOT, 'profiles', 'recommend_calibrated.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_calibrated.py measures on the GPU: there is no CPU path'

    cfg = make_config()
    U, H, k, lam, alpha = args.users, cfg.max_history_num, args.k, args.lam, args.alpha
    n_news = max(args.pools) + 1
    corpus = synth.synth_corpus(cfg, n_news=n_news, n_train=1, n_dev=1, seed=args.seed)
    corpus.news_category[1:] = 1 + corpus.news_subCategory[1:] % (cfg.category_num - 1)
    dc = DeviceCorpus(corpus)
    model = Model(cfg)
    model.initialize()
    synth.fill_state_dict(model, seed=args.seed)
    model = model.cuda().eval()
    cache = model.build_news_cache(dc)
    torch.cuda.synchronize()
    keys, cat_t, _ = topic_table_of(dc, 'category')
    n_keys = cat_t.numel()
    say('corpus of %d news in %d categories, cache %s' % (n_news, n_keys, tuple(cache.shape)))
    rng = np.random.default_rng(args.seed)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def users(n):
        n_hist = rng.integers(5, H + 1, size=n)
        mask = np.arange(H)[None, :] < n_hist[:, None]
        hist = np.where(mask, rng.integers(1, n_news, size=(n, H)), 0).astype(np.int32)
        ufr = np.where(mask, np.exp(rng.uniform(np.log(60.0), np.log(30 * 86400.0), size=(n, H))), 0.0).astype(np.float32)
        ult = np.where(mask, np.exp(rng.uniform(np.log(600.0), np.log(14 * 86400.0), size=(n, H))), 0.0).astype(np.float32)
        return dict(news_cache=cache, corpus=dc, hist_index=t(hist), hist_mask=t(mask), user_freshness=t(ufr), user_lifetime=t(ult))

    lines = []
    tol = tolerance(H, alpha)

    def measure(shape, call, side, ids_of, M, **more):
        """One shape: ``call(**kw)`` the entry over the users ``side``; ``ids_of(positions)`` the news ids of shortlist positions."""
        hist_keys = serving.history_keys(keys, side['hist_index'], side['hist_mask'])

        def composed():
            pos, top = call(k=M)
            pos, top = pos.reshape(-1, M), top.reshape(-1, M).contiguous()
            picks = torch_calibrated(top, ids_of(pos), keys, n_keys, hist_keys, lam, alpha, k)
            return torch.gather(pos, 1, picks.clamp(min=0).long())
        cal_kw = dict(calibrate_lambda=lam, calibrate_alpha=alpha, shortlist=M)
        ms, out = alternate({'plain': lambda: call(k=k), 'calibrated': lambda: call(k=k, **cal_kw), 'torch': composed}, args.rounds)
        pos, top = (x.reshape(-1, M) for x in call(k=M))
        top, ids = top.contiguous(), ids_of(pos).contiguous()
        sel, got = alternate({'calibrate_rows': lambda: ops.calibrate_rows(top, ids, keys, n_keys, hist_keys, None, lam, alpha, k),
                              'torch_loop': lambda: torch_calibrated(top, ids, keys, n_keys, hist_keys, lam, alpha, k)}, args.rounds, args.inner)
        want, gap = recommend.calibrated_select(top.cpu().numpy(), ids.cpu().numpy(), keys.cpu().numpy(), n_keys, hist_keys.cpu().numpy(), None,
                                                lam, alpha, k, return_gap=True)
        sure = gap > 2.0 * tol
        assert np.array_equal(got['calibrate_rows'].cpu().numpy()[sure], want[sure]), 'the kernel\'s picks are not the host statement\'s'
        rows = top.shape[0]
        news = torch.arange(n_news, dtype=torch.int32, device='cuda')          # a pool of every news: a position is a news id
        miss = {}
        for name in ('plain', 'calibrated'):
            value, status = ops.slate_miscalibration(ids_of(out[name][0].reshape(-1, k)).contiguous(), k, None, news, keys, n_keys, hist_keys,
                                                     None, alpha)
            miss[name] = round(float(value[status == 0].mean()), 4)
        med = {name: statistics.median(v) for name, v in {**ms, **sel}.items()}
        line = {'bench': 'recommend_calibrated', 'shape': shape, 'model': model.model_name, 'H': H, 'k': k, 'calibrate_lambda': lam,
                'calibrate_alpha': alpha, 'calibrate_by': 'category', 'groups': n_keys, 'shortlist': M, 'rows': int(rows), 'rounds': args.rounds,
                **more, 'entry_ms': stat(ms['plain']), 'entry_calibrated_ms': stat(ms['calibrated']), 'entry_torch_calibrated_ms': stat(ms['torch']),
                'calibrated_over_plain': round(med['calibrated'] / med['plain'], 4), 'torch_over_plain': round(med['torch'] / med['plain'], 4),
                'selection_inner': args.inner, 'selection_ms': {name: stat(v) for name, v in sel.items()},
                'selection_torch_over_kernel': round(med['torch_loop'] / med['calibrate_rows'], 2),
                'tolerance': tol, 'rows_with_a_clear_gap': int(sure.sum()),
                'torch_loop_rows_equal_to_kernel': int((got['torch_loop'] == got['calibrate_rows']).all(dim=1).sum()),
                'slates_changed': round(float((out['calibrated'][0] != out['plain'][0]).reshape(-1, k).any(dim=1).float().mean()), 4),
                'mean_miscalibration': miss, 'device': torch.cuda.get_device_name(0)}
        say(line)
        lines.append(json.dumps(line))

    side = users(U)
    first_pool = None
    for C in args.pools:
        pool = rng.permutation(np.arange(1, n_news))[:C].astype(np.int32)
        cfr = np.exp(rng.uniform(np.log(60.0), np.log(3 * 86400.0), size=C)).astype(np.float32)
        clt = (cfr[None, :] * np.exp(rng.uniform(-1.0, 1.0, size=(U, C)))).astype(np.float32)
        pool_args = dict(side, cand_index=t(pool), cand_freshness=t(cfr), cand_lifetime=t(clt), n_src=min(U * C, H + cfg.batch_size))
        first_pool = first_pool or pool_args
        cidx = pool_args['cand_index']
        ids_of = lambda pos, cidx=cidx: torch.where(pos >= 0, cidx[pos.clamp(min=0).long()], torch.full_like(pos, -1))
        for M in args.shortlists:
            measure('recommend', lambda pool_args=pool_args, **kw: model.recommend(**pool_args, **kw), side, ids_of, M, users=U, pool=C)
    if args.slots:
        slots = torch.arange(args.slots, dtype=torch.float32, device='cuda') * 3600.0
        cidx = first_pool['cand_index']
        ids_of = lambda pos: torch.where(pos >= 0, cidx[pos.clamp(min=0).long()], torch.full_like(pos, -1))
        measure('recommend_schedule', lambda **kw: model.recommend_schedule(**first_pool, slot_offsets=slots, **kw), side, ids_of,
                args.shortlists[0], users=U, pool=int(cidx.numel()), slots=args.slots)
    if args.lists[0]:
        UL, L = args.lists
        cands = rng.integers(1, n_news, size=UL * L).astype(np.int32)
        cfr = np.exp(rng.uniform(np.log(60.0), np.log(3 * 86400.0), size=UL * L)).astype(np.float32)
        clt = (cfr * np.exp(rng.uniform(-1.0, 1.0, size=UL * L))).astype(np.float32)
        list_side = users(UL)
        list_args = dict(list_side, cand_offsets=t((np.arange(UL + 1) * L).astype(np.int64)), cand_index=t(cands), cand_freshness=t(cfr),
                         cand_lifetime=t(clt))
        cidx, base = list_args['cand_index'], torch.arange(UL, device='cuda').unsqueeze(1) * L
        ids_of = lambda pos: torch.where(pos >= 0, cidx[(base + pos.clamp(min=0).long())], torch.full_like(pos, -1))
        measure('recommend_lists', lambda **kw: model.recommend_lists(**list_args, **kw), list_side, ids_of, args.shortlists[0], lists=UL,
                list_length=L)
    if args.impressions:
        # what a setting costs in nDCG@k and buys in calibration, on the labelled impressions of bench_eval's synthetic dev split
        beh, indices, labels, counts = make_dev_split(cfg, dc, args.impressions, n_news, args.seed)
        settings = [{}, {'calibrate_lambda': lam, 'calibrate_alpha': alpha}, {'calibrate_lambda': 0.0, 'calibrate_alpha': alpha}]
        metrics, results = util.evaluate_slates_on_device(model, beh, indices, labels, settings, k=k, rows_per_forward=cfg.batch_size,
                                                          calibration='category')
        line = {'bench': 'recommend_calibrated', 'shape': 'sweep', 'model': model.model_name, 'impressions': len(labels), 'rows': int(beh.num),
                'k': k, 'calibration': 'category', 'pass_metrics': [round(m, 6) for m in metrics],
                'settings': [dict(setting=s, ndcg=round(r['ndcg'], 6), miscalibration=round(r['miscalibration'], 6), topics=round(r['topics'], 4),
                                  n_relevance=r['n_relevance'], n_calibration=r['n_calibration']) for s, r in zip(settings, results)],
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
