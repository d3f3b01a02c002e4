"""Pool recommendation at a size a user would serve: Model.recommend against the existing way to get the same answer --
Model.score_behaviors over the (user, candidate) pairs written out as rows, then torch.topk -- alternated in one process after warm-up.

32 users, H = 50, the full-size model with synthetic weights, pools of 2,000 and 65,536 synthetic news over MIND's topic counts
(18 categories, 270 subcategories), k = 10.  The second form materialises a history per row, so it runs over as many of the U x C pairs as
``--old-pairs`` allows (whole users first, in calls of ``--old-rows`` rows) and the result says how many; the per-pair times are what
compare.  Device-event medians.  Prints one JSON line per pool and writes them to ``--json-out`` (default profiles/recommend.json).

    python tools/bench_recommend.py --rounds 5

``--news-encoder X`` (with ``--user-encoder Y``) measures a baseline model -- X as the news encoder itself, no LIME -- instead: its
candidates depend on the news alone, and Model.recommend on lime_grouped_match_indexed_f32 (the pool's rows and their Q once per call,
read in place) is alternated with the same model on the gather form (LIME_INDEXED_MATCH=0: one materialised row and one Q row per pair,
the kernel LIME models take).  One JSON line per pool, appended to profiles/plain_recommend.json.

    python tools/bench_recommend.py --news-encoder CROWN --user-encoder CROWN --rounds 5

``--occurrence-match`` (with ``--content-encoder X --user-encoder Y``) measures a LIME model with its candidates composed in the
kernel (LIME_OCCURRENCE_MATCH=1: lime_grouped_match_occurrence_f32 on the pool's cache rows and the occurrence tables) alternated
with the same model on the materialised path (the switch off: one encode_cached row, one Q row per pair).  One JSON line per pool,
appended to profiles/occurrence_match.json.

    python tools/bench_recommend.py --occurrence-match --content-encoder NAML --user-encoder ATT --rounds 5
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
from lime_cikm25_amd import DeviceBehaviors, DeviceCorpus, Model, make_config, synth  # noqa: E402
from lime_cikm25_amd import model as model_module  # noqa: E402


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def switch_forms(model, call_args, k, n_src, rounds, head, entry, switch, default, names):
    """``entry`` of one model with the module switch ``switch`` of lime_cikm25_amd.model on and off, alternated after warm-up -> the
    result line; ``names``: what the two forms are called in it (on, off); ``default``: the value the switch is left at."""
    def form(on):
        setattr(model_module, switch, on)
        try:
            return getattr(model, entry)(**call_args, k=k, n_src=n_src)
        finally:
            setattr(model_module, switch, default)

    for _ in range(2):
        form(True)
        form(False)
    torch.cuda.synchronize()
    ms, pos = {True: [], False: []}, {}
    for _ in range(rounds):
        for on in (True, False):
            dt, out = event_ms(lambda: form(on))
            ms[on].append(dt)
            pos[on] = out[0]
    agree = float((pos[True] == pos[False]).float().mean())
    peak = {}
    for on in (True, False):                                               # the call's own peak above what is resident
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        form(on)
        torch.cuda.synchronize()
        peak[on] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    stat = lambda v: {'median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}
    new, old = names
    line = dict(head, rounds=rounds, **{new + '_ms': stat(ms[True]), old + '_ms': stat(ms[False]),
                                        '%s_over_%s' % (old, new): round(statistics.median(ms[False]) / statistics.median(ms[True]), 3),
                                        new + '_peak_mib': round(peak[True], 1), old + '_peak_mib': round(peak[False], 1)},
                same_positions_fraction=round(agree, 4), device=torch.cuda.get_device_name(0))
    say(line)
    return line


def plain_forms(model, call_args, k, n_src, rounds, head, entry='recommend'):
    """A baseline model's ``entry`` on the indexed match and on the gather form."""
    return switch_forms(model, call_args, k, n_src, rounds, head, entry, 'INDEXED_MATCH', True, ('indexed', 'gather'))


def occurrence_forms(model, call_args, k, n_src, rounds, head, entry='recommend'):
    """A LIME model's ``entry`` with its candidates composed in the kernel and on the materialised path (the parent's code)."""
    assert model.occurrence_match_applicable(), '%s keeps the materialised path: nothing to alternate' % model.model_name
    return switch_forms(model, call_args, k, n_src, rounds, head, entry, 'OCCURRENCE_MATCH', False, ('composed', 'materialised'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=32)
    ap.add_argument('--pools', type=int, nargs='*', default=[2000, 65536])
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--old-pairs', type=int, default=131072, help='pairs the score_behaviors form runs over, at the most')
    ap.add_argument('--old-rows', type=int, default=16384, help='rows per score_behaviors call')
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--news-encoder', default='LIME', help="'LIME' (default) or a baseline: CROWN, CNN, NAML, MHSA, KCNN")
    ap.add_argument('--user-encoder', default='CROWN')
    ap.add_argument('--content-encoder', default='CROWN', help="LIME's content encoder (read with --occurrence-match)")
    ap.add_argument('--occurrence-match', action='store_true', help='a LIME model composed in the kernel against its materialised path')
    ap.add_argument('--json-out', default=None, help='default: profiles/recommend.json (LIME, rewritten), profiles/plain_recommend.json '
                                                     '(a baseline, appended to), profiles/occurrence_match.json (--occurrence-match, '
                                                     'appended to)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_recommend.py measures on the GPU: there is no CPU path'
    plain = args.news_encoder != 'LIME'
    assert not (plain and args.occurrence_match), 'a baseline model has no occurrence: --occurrence-match measures LIME models'
    forms = plain_forms if plain else occurrence_forms if args.occurrence_match else None
    if args.json_out is None:
        args.json_out = os.path.join(ROOT, 'profiles', 'plain_recommend.json' if plain else
                                     'occurrence_match.json' if args.occurrence_match else 'recommend.json')

    cfg = make_config(news_encoder=args.news_encoder, user_encoder=args.user_encoder, content_encoder=args.content_encoder)
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
    lines = []
    for C in args.pools:
        pool = rng.permutation(np.arange(1, n_news))[:C].astype(np.int32)
        cfr = np.exp(rng.uniform(np.log(60.0), np.log(3 * 86400.0), size=C)).astype(np.float32)
        clt = (cfr[None, :] * np.exp(rng.uniform(-1.0, 1.0, size=(U, C)))).astype(np.float32)     # remaining lifetime of either sign
        pool_args = dict(news_cache=cache, corpus=dc, hist_index=t(hist), hist_mask=t(mask), user_freshness=t(ufr), user_lifetime=t(ult),
                         cand_index=t(pool), cand_freshness=t(cfr), cand_lifetime=t(clt))
        n_src = min(U * C, H + cfg.batch_size)
        topics = len(set(zip(corpus.news_category[pool].tolist(), corpus.news_subCategory[pool].tolist())))
        if forms is not None:
            lines.append(json.dumps(forms(model, pool_args, k, n_src, args.rounds, dict(
                bench='recommend', model=model.model_name, users=U, H=H, pool=C, topics_in_pool=topics, k=k, pairs=U * C))))
            continue
        # the second form: whole users, as many as --old-pairs allows
        u_old = max(1, min(U, args.old_pairs // C))
        R = u_old * C
        beh = DeviceBehaviors(dc, np.repeat(np.arange(u_old), C), np.repeat(hist[:u_old], C, axis=0), np.repeat(mask[:u_old], C, axis=0),
                              np.repeat(ufr[:u_old], C, axis=0), np.repeat(ult[:u_old], C, axis=0), np.tile(pool, u_old).reshape(R, 1),
                              np.tile(cfr, u_old).reshape(R, 1), clt[:u_old].reshape(R, 1), eval_shape=True)
        rows = torch.arange(R, device='cuda')

        def new_form():
            return model.recommend(**pool_args, k=k, n_src=n_src)

        def old_form():
            scores = torch.cat([model.score_behaviors(beh, rows[r0:r0 + args.old_rows], cache, n_src=n_src)
                                for r0 in range(0, R, args.old_rows)]).view(u_old, C)
            top, pos = torch.topk(scores, k, dim=1)
            return pos, top

        for _ in range(2):                                                 # warm-up: kernels loaded, the allocator holds the blocks
            new_form()
            old_form()
        torch.cuda.synchronize()
        new_ms, old_ms = [], []
        for _ in range(args.rounds):
            dt, (pos, top) = event_ms(new_form)
            new_ms.append(dt)
            dt, (pos_old, top_old) = event_ms(old_form)
            old_ms.append(dt)
        agree = float((pos[:u_old].long() == pos_old).float().mean())
        score_ms = statistics.median(event_ms(lambda: model.score_pool(**pool_args, n_src=n_src))[0] for _ in range(args.rounds))
        new_med, old_med = statistics.median(new_ms), statistics.median(old_ms)
        line = {'bench': 'recommend', 'users': U, 'H': H, 'pool': C, 'topics_in_pool': topics, 'k': k, 'rounds': args.rounds,
                'recommend_ms': {'median': round(new_med, 3), 'min': round(min(new_ms), 3), 'max': round(max(new_ms), 3)},
                'score_pool_ms_median': round(score_ms, 3), 'recommend_pairs': U * C,
                'score_behaviors_topk_ms': {'median': round(old_med, 3), 'min': round(min(old_ms), 3), 'max': round(max(old_ms), 3)},
                'score_behaviors_pairs': R, 'score_behaviors_users': u_old, 'score_behaviors_rows_per_call': args.old_rows,
                'us_per_pair_recommend': round(1e3 * new_med / (U * C), 4), 'us_per_pair_score_behaviors': round(1e3 * old_med / R, 4),
                'per_pair_ratio_old_over_new': round((old_med / R) / (new_med / (U * C)), 2),
                'same_positions_fraction_on_shared_users': round(agree, 4), 'device': torch.cuda.get_device_name(0)}
        say(line)
        lines.append(json.dumps(line))
        del beh
        torch.cuda.empty_cache()
    print('\n'.join(lines))
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, 'a' if forms is not None else 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
