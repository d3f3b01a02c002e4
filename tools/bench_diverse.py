"""What a diverse slate costs and what it buys, at a size a user would serve: the recommend entries with ``mmr_lambda=0.5`` against
the same call without it and against the same selection as a torch composition on the device -- the entry's own scores and shortlist,
then a gather of the shortlist's similarity rows, their normalisation and a k-round loop of about six launches a round: the yardstick
--, alternated in one process after warm-up.  The selection alone -- lime_mmr_rows_f32 against that torch loop on the same shortlist --
is repeated ``--inner`` times between two device events.  Also reported: the mean pairwise cosine within the slates with and without
MMR, the quantity the feature exists to lower.

32 users, H = 50, the full-size model with synthetic weights, k = 10; Model.recommend over pools of 2,000 and 65,536 synthetic news with
shortlists of 64 and 128; Model.recommend_schedule over 24 slots of the first pool; Model.recommend_lists over 1,024 lists of 100.
Device-event medians.  Prints one JSON line per shape and writes them to ``--json-out`` (default profiles/recommend_diverse.json).

    python tools/bench_diverse.py --rounds 5
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
from lime_cikm25_amd import DeviceCorpus, Model, make_config, ops, recommend, serving, synth  # noqa: E402
from bench_quota import alternate, say, stat  # noqa: E402


def torch_mmr(top, ids, table, lam, k):
    """``recommend.mmr_select`` as a torch composition on the device: top fp32 [R, M], ids int32 [R, M] (-1: none) -> picks [R, k]."""
    R, M = top.shape
    live = (ids >= 0) & torch.isfinite(top)
    x = table[ids.clamp(min=0).long()]                                        # [R, M, E]
    norm = x.norm(dim=2, keepdim=True)
    x = torch.where(norm > 0, x / norm.clamp_min(1e-30), torch.zeros_like(x))
    rank = torch.arange(M, device=top.device).expand(R, M)
    first = torch.where(live, rank, M).min(dim=1, keepdim=True).values.clamp(max=M - 1)
    last = torch.where(live, rank, -1).max(dim=1, keepdim=True).values.clamp(min=0)
    s_first, s_last = top.gather(1, first), top.gather(1, last)
    span = s_first - s_last
    rel = torch.where(live & (span != 0), (top - s_last) / span, torch.zeros_like(top))
    pen, open_ = torch.zeros_like(top), live.clone()
    picks = torch.full((R, k), -1, dtype=torch.int32, device=top.device)
    neg = torch.full_like(top, float('-inf'))
    for r in range(k):
        best = torch.where(open_, lam * rel - (1.0 - lam) * pen, neg).argmax(dim=1, keepdim=True)
        picks[:, r:r + 1] = torch.where(open_.any(dim=1, keepdim=True), best, -1).int()
        open_.scatter_(1, best, False)
        cos = torch.bmm(x, x.gather(1, best.unsqueeze(2).expand(R, 1, x.shape[2])).transpose(1, 2)).squeeze(2)
        pen = torch.maximum(pen, cos)
    return picks


def slate_cosine(news, table):
    """The mean cosine over the pairs of distinct news of a slate, averaged over the slates; news int [R, k], all >= 0."""
    x = torch.nn.functional.normalize(table[news.long()], dim=2)
    gram = torch.bmm(x, x.transpose(1, 2))
    k = news.shape[1]
    return float(((gram.sum(dim=(1, 2)) - gram.diagonal(dim1=1, dim2=2).sum(dim=1)) / (k * (k - 1))).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=32)
    ap.add_argument('--pools', type=int, nargs='*', default=[2000, 65536])
    ap.add_argument('--shortlists', type=int, nargs='*', default=[64, 128])
    ap.add_argument('--slots', type=int, default=24)
    ap.add_argument('--lists', type=int, nargs=2, default=[1024, 100], help='lists and candidates per list')
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--lam', type=float, default=0.5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--inner', type=int, default=50, help='selections between two device events')
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--json-out', default=os.path.join(ROOT, 'profiles', 'recommend_diverse.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_diverse.py measures on the GPU: there is no CPU path'

    cfg = make_config()
    U, H, k, lam = args.users, cfg.max_history_num, args.k, args.lam
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
    say('corpus of %d news, cache %s' % (n_news, tuple(cache.shape)))
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

    def measure(shape, call, ids_of, M, **more):
        """One shape: ``call(**kw)`` the entry; ``ids_of(positions)`` the news ids of shortlist positions (-1 stays -1)."""
        table = serving.diversity(model, cache, k, lam, M, None).table

        def composed():
            pos, top = call(k=M)
            pos, top = pos.reshape(-1, M), top.reshape(-1, M).contiguous()
            picks = torch_mmr(top, ids_of(pos), table, lam, k)
            return torch.gather(pos, 1, picks.clamp(min=0).long())
        ms, out = alternate({'plain': lambda: call(k=k), 'mmr': lambda: call(k=k, mmr_lambda=lam, shortlist=M), 'torch': composed},
                            args.rounds)
        pos, top = (x.reshape(-1, M) for x in call(k=M))
        top, ids = top.contiguous(), ids_of(pos).contiguous()
        sel, got = alternate({'mmr_rows': lambda: ops.mmr_rows(top, ids, table, lam, k), 'torch_loop': lambda: torch_mmr(top, ids, table, lam, k)},
                             args.rounds, args.inner)
        want, gap = recommend.mmr_select(top.cpu().numpy(), ids.cpu().numpy(), table.cpu().numpy(), lam, k, return_gap=True)
        sure = gap > 16.0 * (table.shape[1] + 8) * 2.0 ** -24
        assert np.array_equal(got['mmr_rows'].cpu().numpy()[sure], want[sure]), 'the kernel\'s picks are not the host statement\'s'
        full = (out['plain'][0].reshape(-1, k) >= 0).all(dim=1) & (out['mmr'][0].reshape(-1, k) >= 0).all(dim=1)
        cos = {name: slate_cosine(ids_of(out[name][0].reshape(-1, k))[full], table) for name in ('plain', 'mmr')}
        med = {name: statistics.median(v) for name, v in {**ms, **sel}.items()}
        line = {'bench': 'recommend_diverse', 'shape': shape, 'model': model.model_name, 'H': H, 'k': k, 'mmr_lambda': lam, 'shortlist': M,
                'similarity_columns': table.shape[1], 'rows': int(top.shape[0]), 'rounds': args.rounds, **more,
                'entry_ms': stat(ms['plain']), 'entry_mmr_ms': stat(ms['mmr']), 'entry_torch_mmr_ms': stat(ms['torch']),
                'mmr_over_plain': round(med['mmr'] / med['plain'], 4), 'torch_over_plain': round(med['torch'] / med['plain'], 4),
                'selection_inner': args.inner, 'selection_ms': {name: stat(v) for name, v in sel.items()},
                'selection_torch_over_kernel': round(med['torch_loop'] / med['mmr_rows'], 2),
                'rows_with_a_clear_gap': int(sure.sum()),
                'torch_loop_rows_equal_to_kernel': int((got['torch_loop'] == got['mmr_rows']).all(dim=1).sum()),
                'slates_changed': round(float((out['mmr'][0] != out['plain'][0]).reshape(-1, k).any(dim=1).float().mean()), 4),
                'mean_pairwise_cosine': {name: round(v, 4) for name, v in cos.items()}, 'device': torch.cuda.get_device_name(0)}
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
            measure('recommend', lambda pool_args=pool_args, **kw: model.recommend(**pool_args, **kw), ids_of, M, users=U, pool=C)
    if args.slots:
        slots = torch.arange(args.slots, dtype=torch.float32, device='cuda') * 3600.0
        cidx = first_pool['cand_index']
        ids_of = lambda pos: torch.where(pos >= 0, cidx[pos.clamp(min=0).long()], torch.full_like(pos, -1))
        measure('recommend_schedule', lambda **kw: model.recommend_schedule(**first_pool, slot_offsets=slots, **kw), ids_of, args.shortlists[0],
                users=U, pool=int(cidx.numel()), slots=args.slots)
    if args.lists[0]:
        UL, L = args.lists
        cands = rng.integers(1, n_news, size=UL * L).astype(np.int32)
        cfr = np.exp(rng.uniform(np.log(60.0), np.log(3 * 86400.0), size=UL * L)).astype(np.float32)
        clt = (cfr * np.exp(rng.uniform(-1.0, 1.0, size=UL * L))).astype(np.float32)
        list_args = dict(users(UL), cand_offsets=t((np.arange(UL + 1) * L).astype(np.int64)), cand_index=t(cands), cand_freshness=t(cfr),
                         cand_lifetime=t(clt))
        cidx, base = list_args['cand_index'], torch.arange(UL, device='cuda').unsqueeze(1) * L
        ids_of = lambda pos: torch.where(pos >= 0, cidx[(base + pos.clamp(min=0).long())], torch.full_like(pos, -1))
        measure('recommend_lists', lambda **kw: model.recommend_lists(**list_args, **kw), ids_of, args.shortlists[0], lists=UL, list_length=L)
    print('\n'.join(lines))
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
