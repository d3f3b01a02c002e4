"""What an explanation costs: Model.explain_lists against the call it rides on and against the same quantities composed in torch,
alternated in one process after warm-up.  Full-size models, synthetic weights, H = 50, top = 3, LIME-CROWN-CROWN and LIME-NAML-ATT.

  * slate: 32 users x the k = 10 news ``recommend`` picked for them from a pool of 2,000;
  * lists: 1,024 users x 10 candidates of their own.

Per shape and model, device-event medians of
  (a) ``explain_lists`` (lime_grouped_match_explain_f32 as the last launch of every pass);
  (b) ``score_lists`` on the same pairs -- the scores alone, the path that exists without this tool's subject;
  (c) ``explain_lists`` with its last launch replaced by torch: the groups' rows gathered per pair ([pairs, H, A] and [pairs, H, D]),
      two ``bmm``, ``softmax``, the weight and ``topk`` under the mask.
Prints one JSON line per (shape, model) and writes them to ``--json-out`` (default profiles/explain.json).

    python tools/bench_explain.py --rounds 5
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

MODELS = {'LIME-CROWN-CROWN': dict(content_encoder='CROWN', user_encoder='CROWN'), 'LIME-NAML-ATT': dict(content_encoder='NAML', user_encoder='ATT')}


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def spread(xs):
    return {'median': round(statistics.median(xs), 3), 'min': round(min(xs), 3), 'max': round(max(xs), 3)}


def composed_terms(kp, g, qp, cand, remaining, offsets, H, scale, alpha=0.0, beta=0.0, use_weight=False, use_penalty=False, mask=None,
                   hist_div=1, m=3, by='contribution', dense=True, index=None, n=None, occ=None, qt=None, ct=None, n_occ=None):
    """``ops.grouped_match_explain`` on torch launches: every pair gets its own copy of its group's H rows."""
    G = kp.shape[0] // H
    if index is not None:
        qp, cand = qp[index.long()], cand[index.long()]
        if occ is not None:
            qp, cand = qp + qt[occ.long()], cand + ct[occ.long()]
    P = qp.shape[0]
    group = torch.repeat_interleave(torch.arange(G, device=kp.device), offsets[1:] - offsets[:-1], output_size=P)
    s = torch.bmm(kp.view(G, H, -1)[group], qp.unsqueeze(2)).squeeze(2) * scale
    a = torch.softmax(s, dim=1)
    mm = torch.bmm(g.view(G, H, -1)[group], cand.unsqueeze(2)).squeeze(2)
    if not use_weight:
        w = torch.ones((P,), dtype=torch.float32, device=kp.device)
    elif use_penalty:
        w = torch.sigmoid(alpha * remaining) * torch.where(remaining >= 0, 1.0, beta)
    else:
        w = torch.sigmoid(alpha * remaining.abs())
    terms = a * mm
    base, contrib = terms.sum(dim=1), terms * w.unsqueeze(1)
    values = contrib if by == 'contribution' else a
    if mask is not None:
        values = values.masked_fill(~mask.bool().view(-1, H)[group // hist_div], float('-inf'))
    top, slot = values.topk(m, dim=1)
    none = torch.isinf(top) & (top < 0)
    return ops.PairTerms(base * w, base, w, a if dense else None, contrib if dense else None,
                         slot.to(torch.int32).masked_fill(none, -1), top.masked_fill(none, 0.0))


def measure(model, list_args, n_src, top, rounds):
    explain = lambda: model.explain_lists(**list_args, top=top, n_src=n_src)
    score = lambda: model.score_lists(**list_args, n_src=n_src)
    kernel = ops.grouped_match_explain

    def in_torch():
        ops.grouped_match_explain = composed_terms
        try:
            return model.explain_lists(**list_args, top=top, n_src=n_src)
        finally:
            ops.grouped_match_explain = kernel
    forms = (('explain_lists', explain), ('score_lists', score), ('composed_in_torch', in_torch))
    for _ in range(2):                                                     # warm-up: kernels loaded, the allocator holds the blocks
        for _, f in forms:
            f()
    torch.cuda.synchronize()
    ms, out = {n: [] for n, _ in forms}, {}
    for _ in range(rounds):                                                # alternating: a drift of the clocks hits all three alike
        for n, f in forms:
            dt, out[n] = event_ms(f)
            ms[n].append(dt)
    a, b, c = (statistics.median(ms[n]) for n, _ in forms)
    ex, ref = out['explain_lists'], out['composed_in_torch']
    filled = (ex.slots >= 0) & (ref.slots >= 0)
    return {'rounds': rounds, **{n + '_ms': spread(v) for n, v in ms.items()}, 'explain_over_score': round(a / b, 3),
            'torch_over_explain': round(c / a, 3), 'score_bits_equal_score_lists': bool(torch.equal(ex.score, out['score_lists'])),
            'same_slots_as_torch_fraction': round(float((ex.slots == ref.slots)[filled].float().mean()), 4),
            # where the two name another slot at a rank, near-equal terms changed places under the two roundings: the values at the rank agree
            'max_value_difference_at_a_rank_over_mean_magnitude': float(((ex.values - ref.values).abs()[filled].max()
                                                                         / ex.values[filled].abs().mean()).cpu())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--news', type=int, default=20000)
    ap.add_argument('--pool', type=int, default=2000)
    ap.add_argument('--pool-users', type=int, default=32)
    ap.add_argument('--lists', type=int, default=1024)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--top', type=int, default=3)
    ap.add_argument('--models', nargs='*', default=list(MODELS))
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--json-out', default=os.path.join(ROOT, 'profiles', 'explain.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_explain.py measures on the GPU: there is no CPU path'
    lines = []
    for name in args.models:
        cfg = make_config(vocabulary_size=50000, **MODELS[name])
        H = cfg.max_history_num
        corpus = synth.synth_corpus(cfg, n_news=args.news, n_train=1, n_dev=1, seed=args.seed)
        corpus.news_category[1:] = 1 + corpus.news_subCategory[1:] % (cfg.category_num - 1)      # MIND: a subcategory sits under one category
        dc = DeviceCorpus(corpus)
        model = Model(cfg)
        model.initialize()
        synth.fill_state_dict(model, seed=args.seed)
        model = model.cuda().eval()
        cache = model.build_news_cache(dc)
        rng = np.random.default_rng(args.seed)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

        def users(U):
            mask = np.arange(H)[None, :] < rng.integers(5, H + 1, size=U)[:, None]
            hist = np.where(mask, rng.integers(1, args.news, size=(U, H)), 0).astype(np.int32)
            ufr = np.where(mask, np.exp(rng.uniform(np.log(60.0), np.log(30 * 86400.0), size=(U, H))), 0.0).astype(np.float32)
            ult = np.where(mask, np.exp(rng.uniform(np.log(600.0), np.log(14 * 86400.0), size=(U, H))), 0.0).astype(np.float32)
            return dict(news_cache=cache, corpus=dc, hist_index=t(hist), hist_mask=t(mask), user_freshness=t(ufr), user_lifetime=t(ult))

        def candidates(n):
            cfr = np.exp(rng.uniform(np.log(60.0), np.log(3 * 86400.0), size=n)).astype(np.float32)
            return rng.integers(1, args.news, size=n).astype(np.int32), cfr, (cfr * np.exp(rng.uniform(-1.0, 1.0, size=n))).astype(np.float32)

        for shape in ('slate', 'lists'):
            if shape == 'slate':                                           # the lists are what recommend picked from the pool
                U, (pool, cfr, clt) = args.pool_users, candidates(args.pool)
                who = users(U)
                pos, _ = model.recommend(**who, cand_index=t(pool), cand_freshness=t(cfr), cand_lifetime=t(clt), k=args.k)
                at = pos.long().reshape(-1)
                assert (at >= 0).all()
                idx, fr, lt = t(pool)[at], t(cfr)[at], t(clt)[at]
            else:
                U = args.lists
                who = users(U)
                idx, fr, lt = (t(x) for x in candidates(U * args.k))
            P = U * args.k
            list_args = dict(who, cand_offsets=t((np.arange(U + 1) * args.k).astype(np.int64)), cand_index=idx, cand_freshness=fr,
                             cand_lifetime=lt)
            line = dict(bench='explain', shape=shape, model=name, users=U, k=args.k, pairs=P, H=H, top=args.top, news=args.news,
                        **measure(model, list_args, min(P, H + cfg.batch_size), args.top, args.rounds),
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
