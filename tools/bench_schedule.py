"""A schedule of time slots at a size a user would serve: Model.recommend_schedule against the existing way to get the same answer,
three forms of one model alternated in one process after warm-up:

    (a) calls       S calls of Model.recommend, one per slot, at ``cand_freshness + slot_offsets[s]`` -- code this change does not touch;
    (b) shared      recommend_schedule on the shared-user-side route (LIME_SCHEDULE_MATCH=0): the user side once, the existing match
                    once per slot;
    (c) factorised  recommend_schedule on lime_grouped_match_schedule_f32 (the default where Model.schedule_match_applicable()).

32 users, H = 50, the full-size model with synthetic weights, pools of 2,000 and 65,536 synthetic news over MIND's topic counts,
k = 10, S in {1, 4, 24} hourly slots.  Models: LIME-CROWN-CROWN at the default fusion, LIME-NAML-ATT and the baseline NAML-ATT.
Device-event times; per form the median, min and max over the rounds.  One JSON line per (model, pool, S), written to ``--json-out``
(default profiles/recommend_schedule.json).

    python tools/bench_schedule.py --rounds 5
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
from lime_cikm25_amd import DeviceCorpus, Model, make_config, synth  # noqa: E402
from lime_cikm25_amd import model as model_module  # noqa: E402

MODELS = {'LIME-CROWN-CROWN': dict(), 'LIME-NAML-ATT': dict(content_encoder='NAML', user_encoder='ATT'),
          'NAML-ATT': dict(news_encoder='NAML', user_encoder='ATT')}


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=32)
    ap.add_argument('--pools', type=int, nargs='*', default=[2000, 65536])
    ap.add_argument('--slots', type=int, nargs='*', default=[1, 4, 24])
    ap.add_argument('--models', nargs='*', default=list(MODELS), choices=list(MODELS))
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--json-out', default=os.path.join(ROOT, 'profiles', 'recommend_schedule.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_schedule.py measures on the GPU: there is no CPU path'
    lines = []
    for name in args.models:
        cfg = make_config(**MODELS[name])
        U, H, k = args.users, cfg.max_history_num, args.k
        n_news = max(args.pools) + 1
        corpus = synth.synth_corpus(cfg, n_news=n_news, n_train=1, n_dev=1, seed=args.seed)
        # MIND's subcategories each sit under one category: about 270 topics in all (independent draws would give 18 x 270)
        corpus.news_category[1:] = 1 + corpus.news_subCategory[1:] % (cfg.category_num - 1)
        dc = DeviceCorpus(corpus)
        model = Model(cfg)
        model.initialize()
        synth.fill_state_dict(model, seed=args.seed)
        model = model.cuda().eval()
        assert model.model_name == name
        cache = model.build_news_cache(dc)
        torch.cuda.synchronize()
        say('%s: corpus of %d news, cache %s' % (name, n_news, tuple(cache.shape)))
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
            clt = (cfr[None, :] * np.exp(rng.uniform(-1.0, 1.0, size=(U, C)))).astype(np.float32)     # remaining lifetime of either sign
            pool_args = dict(news_cache=cache, corpus=dc, hist_index=t(hist), hist_mask=t(mask), user_freshness=t(ufr), user_lifetime=t(ult),
                             cand_index=t(pool), cand_lifetime=t(clt))
            fresh = t(cfr)
            n_src = min(U * C, H + cfg.batch_size)
            for S in args.slots:
                offsets = torch.arange(S, dtype=torch.float32, device='cuda') * 3600.0               # hourly slots
                host_offsets = offsets.tolist()

                def calls():
                    out = [model.recommend(**pool_args, cand_freshness=fresh + o, k=k, n_src=n_src) for o in host_offsets]
                    return torch.stack([p for p, _ in out]), torch.stack([s for _, s in out])

                def schedule(on):
                    model_module.SCHEDULE_MATCH = on
                    try:
                        return model.recommend_schedule(**pool_args, cand_freshness=fresh, slot_offsets=offsets, k=k, n_src=n_src)
                    finally:
                        model_module.SCHEDULE_MATCH = True
                forms = {'calls': calls, 'shared': lambda: schedule(False), 'factorised': lambda: schedule(True)}
                routes = {}
                for on in (False, True):
                    model_module.SCHEDULE_MATCH = on
                    routes['factorised' if on else 'shared'] = model.schedule_route(S, H)
                model_module.SCHEDULE_MATCH = True
                for _ in range(args.warmup):                                   # kernels loaded, the allocator holds the blocks
                    for f in forms.values():
                        f()
                torch.cuda.synchronize()
                ms, pos = {n: [] for n in forms}, {}
                for _ in range(args.rounds):                                   # alternated: a drift of the clocks falls on all three
                    for n, f in forms.items():
                        dt, out = event_ms(f)
                        ms[n].append(dt)
                        pos[n] = out[0]
                stat = lambda v: {'median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}
                med = {n: statistics.median(v) for n, v in ms.items()}
                line = dict(bench='recommend_schedule', model=name, users=U, H=H, pool=C, k=k, slots=S, rounds=args.rounds,
                            calls_ms=stat(ms['calls']), shared_ms=stat(ms['shared']), factorised_ms=stat(ms['factorised']),
                            route_of_shared=routes['shared'], route_of_factorised=routes['factorised'],
                            calls_over_shared=round(med['calls'] / med['shared'], 3), calls_over_factorised=round(med['calls'] / med['factorised'], 3),
                            same_positions_fraction_shared=round(float((pos['shared'] == pos['calls']).float().mean()), 4),
                            same_positions_fraction_factorised=round(float((pos['factorised'] == pos['calls']).float().mean()), 4),
                            device=torch.cuda.get_device_name(0))
                say(line)
                lines.append(json.dumps(line))
            torch.cuda.empty_cache()
        del model, cache, dc
        torch.cuda.empty_cache()
    print('\n'.join(lines))
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
