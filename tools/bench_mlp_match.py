"""The MLP click predictor's match on one launch (lime_grouped_mlp_match_f32, ops.FUSED_MLP_MATCH on) against the composed form on
existing launches (off), alternated in one process after warm-up, on the full-size LIME-CROWN-CROWN model with synthetic weights:

  * the forward shape: batch 32, K = 1 + 4 candidates, history 50 -- Model.forward by graph replay (every group has N = 5 pairs; the
    composed form is lime_interest_match_f32's user rows, one [160, 800] -> [160, 200] GEMM and the product with ``out``);
  * the pool shape of tools/bench_recommend.py: 32 users against pools of 2,000 and 65,536 news over MIND's topic counts --
    Model.score_pool (groups of a topic's news: the composed form gives every pair its own copy of its group's H history rows, in
    steps of 1,024 pairs, to get the pair's user row from lime_interest_match_f32, then writes the [pairs, 800] and [pairs, 200] rows).

Device-event medians and the call's peak memory above what is resident.  Prints one JSON line per shape and writes them to
``--json-out`` (default profiles/mlp_match.json).

    python tools/bench_mlp_match.py --rounds 5
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
from lime_cikm25_amd import DeviceCorpus, Model, make_config, ops, synth  # noqa: E402


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def alternate(call, rounds, head):
    """``call()`` under both forms, alternated after warm-up -> the result line."""
    def form(fused):
        ops.FUSED_MLP_MATCH = fused
        try:
            return call()
        finally:
            ops.FUSED_MLP_MATCH = True

    for _ in range(2):
        form(True)
        form(False)
    torch.cuda.synchronize()
    ms, out = {True: [], False: []}, {}
    for _ in range(rounds):
        for fused in (True, False):
            dt, out[fused] = event_ms(lambda: form(fused))
            ms[fused].append(dt)
    diff = float((out[True] - out[False]).abs().max())
    peak = {}
    for fused in (True, False):                                            # the call's own peak above what is resident
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        form(fused)
        torch.cuda.synchronize()
        peak[fused] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    stat = lambda v: {'median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}
    line = dict(head, rounds=rounds, fused_ms=stat(ms[True]), composed_ms=stat(ms[False]),
                composed_over_fused=round(statistics.median(ms[False]) / statistics.median(ms[True]), 3),
                fused_peak_mib=round(peak[True], 1), composed_peak_mib=round(peak[False], 1), max_abs_difference=diff,
                device=torch.cuda.get_device_name(0))
    say(line)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=32)
    ap.add_argument('--pools', type=int, nargs='*', default=[2000, 65536])
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--candidates', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--json-out', default=os.path.join(ROOT, 'profiles', 'mlp_match.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mlp_match.py measures on the GPU: there is no CPU path'

    cfg = make_config(click_predictor='mlp')
    U, H = args.users, cfg.max_history_num
    n_news = max(args.pools + [1]) + 1
    corpus = synth.synth_corpus(cfg, n_news=n_news, n_train=1, n_dev=1, seed=args.seed)
    # MIND's subcategories each sit under one category: about 270 topics in all (independent draws would give 18 x 270)
    corpus.news_category[1:] = 1 + corpus.news_subCategory[1:] % (cfg.category_num - 1)
    dc = DeviceCorpus(corpus)
    model = Model(cfg)
    model.initialize()
    synth.fill_state_dict(model, seed=args.seed)
    model = model.cuda().eval()
    lines = []

    # the forward shape, by graph replay: one captured graph per form (the key holds nothing of the form, so the graphs are dropped)
    batch = [v.cuda() for v in synth.make_batch(cfg, args.batch, args.candidates, seed=args.seed).values()]
    model.training = True                                                  # the [B, K] shape with every child in eval mode
    graphs = {}

    def forward():
        model._graphs = graphs.setdefault(ops.FUSED_MLP_MATCH, {})
        with torch.no_grad():
            return model(*batch)
    lines.append(json.dumps(alternate(forward, args.rounds, dict(bench='mlp_match', shape='forward', model=model.model_name, batch=args.batch,
                                                                 candidates=args.candidates, H=H, pairs=args.batch * args.candidates))))
    model.training = False
    model._graphs = {}

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
    for C in args.pools:
        pool = rng.permutation(np.arange(1, n_news))[:C].astype(np.int32)
        cfr = np.exp(rng.uniform(np.log(60.0), np.log(3 * 86400.0), size=C)).astype(np.float32)
        clt = (cfr[None, :] * np.exp(rng.uniform(-1.0, 1.0, size=(U, C)))).astype(np.float32)
        pool_args = dict(news_cache=cache, corpus=dc, hist_index=t(hist), hist_mask=t(mask), user_freshness=t(ufr), user_lifetime=t(ult),
                         cand_index=t(pool), cand_freshness=t(cfr), cand_lifetime=t(clt))
        n_src = min(U * C, H + cfg.batch_size)
        topics = len(set(zip(corpus.news_category[pool].tolist(), corpus.news_subCategory[pool].tolist())))
        lines.append(json.dumps(alternate(lambda: model.score_pool(**pool_args, n_src=n_src), args.rounds, dict(
            bench='mlp_match', shape='pool', model=model.model_name, users=U, H=H, pool=C, topics_in_pool=topics, pairs=U * C))))
        torch.cuda.empty_cache()
    print('\n'.join(lines))
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
