"""Grouped serving from the news cache, behind ``Model.score_pool`` / ``recommend`` / ``score_schedule`` / ``recommend_schedule`` /
``score_lists`` / ``recommend_lists``: the host refusals, the once-per-call user side, the passes of a grouped match over a plan, the
top-k tails -- and ``click_logits``, which the forward under the MLP predictor reaches too (``Model._row_logits``).  Every function
takes the model as its first argument and this module never imports ``model.py``: the switches and the methods that read them
(``schedule_route``, ``_candidate_tables``), the predicates, the lifetime rule and the offsets cache stay on the model."""
import collections
import numbers

import torch

from . import newsEncoders, ops, recommend as rec

# What every pass of a call reads of the users (``user_side``): hist [U, H, D], ucat / usub / hist_mask [U, H], gate_y: the gate's
# projection of every history row or None, n_src: the GraphSAGE source count.
Users = collections.namedtuple('Users', 'hist ucat usub hist_mask gate_y n_src')
# A call's candidates, one entry per pair: news index, freshness, lifetime, remaining lifetime; ``tables``: what
# ``Model._candidate_tables`` gave (None: a row is materialised per pair) and ``position``: the pair's row of them.  ``slots``: None, or S
# where freshness and remaining carry a leading slot axis [S, ...] that ONE launch matches (the factorised schedule).
Candidates = collections.namedtuple('Candidates', 'index freshness lifetime remaining tables position slots')
# The candidate tables the grouped match reads in place: cand [n, D], qp [n, A], nw [n, D // 2] or None (the MLP predictor's news
# half), and ``occurrence``: a LIME model's Occurrence tables (ct, qt, nt -- as many rows as bucket pairs) or None (a baseline).
Tables = collections.namedtuple('Tables', 'cand qp nw occurrence')
Occurrence = collections.namedtuple('Occurrence', 'ct qt nt')
# The user side of a grouped match over G groups: g [G H, D], kp [G H, A], qp [pairs, A] or None (it is the tables', or made from the
# candidates), H: the history rows the match sees, scale: of its scores.
Operands = collections.namedtuple('Operands', 'g kp qp H scale')
TopicQuota = collections.namedtuple('TopicQuota', 'q topic_of_news n_keys')


def match_operands(model, hist, *topics, cand=None, pairs=None, **kw):
    """``user_encoder.match_operands(hist, *topics, **kw)`` as one Operands record, whichever the user encoder.  CROWN: (g, kp, qp =
    Q(``cand``) or None without ``cand``) over the H history rows.  ATT / MHSA: the pooled vector [G, D] is a history of ONE row whose
    softmax weight is 1, so kp and qp are never felt: four zero columns, qp for ``pairs`` rows (None: the tables bring theirs)."""
    ue = model.user_encoder
    if hasattr(ue, 'user_node_embedding'):
        g, kp, qp = ue.match_operands(hist, *topics, cand=cand, **kw)
        return Operands(g.reshape(-1, g.shape[-1]), kp, qp, hist.shape[1], 1.0 / ue.attention_scalar)
    g = ue.match_operands(hist, *topics, **kw)
    zeros = lambda rows: torch.zeros((rows, 4), dtype=torch.float32, device=g.device)
    return Operands(g, zeros(g.shape[0]), None if pairs is None else zeros(pairs), 1, 1.0)


def click_logits(model, operands, cand, remaining, offsets, tables=None, index=None, occ=None, regular=None):
    """The ONE place that turns (user-side operands, candidates) into logits, for either click predictor -> fp32 [pairs].
    ``operands``: the Operands of G groups (``match_operands``).  ``cand`` [pairs, D] in group order and ``offsets`` int64 [G + 1]
    their CSR; or ``tables`` (``Model._candidate_tables``) read in place through ``index`` int32 [pairs] -- and, where the tables carry
    occurrence tables (a LIME model), composed with the row ``occ`` int32 [pairs] of those in the kernel
    (lime_grouped_match_occurrence_f32 / lime_grouped_mlp_match_occurrence_f32).  ``remaining`` [pairs]: read by the dot product's
    lifetime weight alone.  ``regular``: the pairs per group where every group has as many (the [B, N] shape).  A schedule on the
    factorised route (dot product over tables): ``remaining`` (and ``occ``) [S, pairs] -> fp32 [S, pairs], every slot in one
    lime_grouped_match_schedule_f32 launch.

    dot_product (model.py:179-181): lime_grouped_match_f32.  mlp (:182-184): with mlp.weight split into its user half W_u and its
    news half W_n, gu = g W_u^T once per history row and nw = cand W_n^T + mlp.bias once per candidate row (a table for a baseline
    model), then lime_grouped_mlp_match_f32 keeps a pair's pooled hidden row in registers; ops.FUSED_MLP_MATCH off: the composed
    form -- the pairs' user rows, ``linear(cat, mlp, act='relu')``, the product with ``out`` -- on existing launches."""
    ue, w = model.user_encoder, model.remaining_lifetime_weighting
    g, kp, H, scale = operands.g, operands.kp, operands.H, operands.scale
    D = g.shape[-1]
    if tables is not None:
        cand, qp = tables.cand, tables.qp
    else:
        qp = operands.qp if operands.qp is not None else ops.linear(cand, ue.Q.weight, ue.Q.bias)        # userEncoders.py:162
    occurrence = None if tables is None else tables.occurrence
    if model.click_predictor == 'dot_product':
        composed = dict(occ=occ, qt=occurrence.qt, ct=occurrence.ct) if occurrence is not None else {}
        if remaining.dim() == 2:                                 # a schedule over the tables: remaining (and occ) [S, pairs], one launch
            return ops.grouped_match_schedule(kp, g, qp, cand, remaining, offsets, index, H, scale, w.alpha, w.beta,
                                              bool(w.use_remaining_lifetime_weighting), bool(w.use_expired_penalty),
                                              slots=remaining.shape[0], **composed)
        return ops.grouped_match(kp, g, qp, cand, remaining, offsets, H, scale, w.alpha, w.beta,
                                 bool(w.use_remaining_lifetime_weighting), bool(w.use_expired_penalty), index=index, **composed)
    mlp, out = model.mlp, model.out
    if ops.FUSED_MLP_MATCH:
        gu = ops.linear(g, mlp.weight[:, :D], None)
        nw = tables.nw if tables is not None else ops.linear(cand, mlp.weight[:, D:], mlp.bias)
        composed = dict(occ=occ, qt=occurrence.qt, nt=occurrence.nt) if occurrence is not None and occurrence.nt is not None else {}
        return ops.grouped_mlp_match(kp, gu, qp, nw, out.weight, out.bias, offsets, H, scale, index=index, **composed)
    return _composed_mlp_logits(model, kp, g, qp, cand, offsets, H, scale, index, regular)


def _composed_mlp_logits(model, kp, g, qp, cand, offsets, H, scale, index, regular):
    """The MLP predictor on existing launches (ops.FUSED_MLP_MATCH off; the yardstick of the fused kernel): the user row of every
    pair -- lime_interest_match_f32's, or the group's pooled vector -- then ops.mlp_predictor on the [pairs, 2 D] rows.  Irregular
    groups go through in steps of pairs, each with its own copy of its group's H history rows."""
    mlp, out = model.mlp, model.out
    D, G = g.shape[1], g.shape[0] // H
    P = index.numel() if index is not None else cand.shape[0]
    predict = lambda user, news: ops.mlp_predictor(user, news, mlp.weight, mlp.bias, out.weight, out.bias)
    if regular is not None and index is None and H > 1:
        user, _ = ops.interest_match(kp.reshape(-1), qp.reshape(-1), g.reshape(-1), cand.reshape(-1), None, G, regular, H, kp.shape[1], D,
                                     scale, 0.0, 0.0, False, False, want_logits=False, want_user=True)
        return predict(user.view(P, D), cand)
    group = torch.repeat_interleave(torch.arange(G, device=g.device), offsets[1:] - offsets[:-1], output_size=P)
    logits = torch.empty((P,), dtype=torch.float32, device=g.device)
    slots = torch.arange(H, device=g.device)
    step = 1024 if H > 1 else 1 << 16
    for p0 in range(0, P, step):
        p1 = min(P, p0 + step)
        at = slice(p0, p1) if index is None else index[p0:p1].long()
        news = cand[at].contiguous()
        if H > 1:
            rows = (group[p0:p1].unsqueeze(1) * H + slots).reshape(-1)
            user, _ = ops.interest_match(kp[rows].reshape(-1), qp[at].reshape(-1), g[rows].reshape(-1), news.reshape(-1), None, p1 - p0, 1,
                                         H, kp.shape[1], D, scale, 0.0, 0.0, False, False, want_logits=False, want_user=True)
            user = user.view(p1 - p0, D)
        else:
            user = g[group[p0:p1]]
        logits[p0:p1] = predict(user, news)
    return logits


def check_grouped(model, news_cache, hist_index, hist_mask, user_freshness, user_lifetime, cand_index, bad_index, check_candidates,
                  pairs_per_pass, k, top_k):
    """The host-side refusals (ValueError, before any launch) that the pool and the lists share, in their order -> (U, H, what
    ``check_candidates`` returned).  The form's own stand in between: ``bad_index``: its words when cand_index is not shaped as it
    wants, or None; ``check_candidates(U)`` raises over its other candidate arguments; ``top_k``: (its recommend entry, its kernel)."""
    if model.reads_content_mask:
        raise ValueError(model._NO_CONTENT_CACHE)
    if news_cache.dim() != 2 or news_cache.shape[1] == 0:
        raise ValueError('news_cache must be the [n_news, width] tensor of build_news_cache, got %s' % (tuple(news_cache.shape),))
    if hist_index.dim() != 2:
        raise ValueError('hist_index must be [U, H], got %s' % (tuple(hist_index.shape),))
    U, H = hist_index.shape
    for t, name in ((hist_mask, 'hist_mask'), (user_freshness, 'user_freshness'), (user_lifetime, 'user_lifetime')):
        if tuple(t.shape) != (U, H):
            raise ValueError('%s must be [U, H] = [%d, %d] like hist_index, got %s' % (name, U, H, tuple(t.shape)))
    if bad_index:
        raise ValueError('%s got %s' % (bad_index, tuple(cand_index.shape)))
    if hist_index.dtype not in (torch.int32, torch.int64) or cand_index.dtype not in (torch.int32, torch.int64):
        raise ValueError('hist_index and cand_index must be int32 or int64 news indices, got %s and %s' % (hist_index.dtype, cand_index.dtype))
    own = check_candidates(U)
    if int(pairs_per_pass) < 1:
        raise ValueError('pairs_per_pass must be positive, got %r' % (pairs_per_pass,))
    if k is not None and not 1 <= int(k) <= 128:
        raise ValueError('%s keeps 1 <= k <= 128 news per user (%s), got k = %r' % (top_k + (k,)))
    return U, H, own


def user_side(model, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, n_src, n_pairs):
    """What every pass of a call reads of the users, once per call -> Users (n_src: its default from the call's ``n_pairs``)."""
    ue, (U, H) = model.user_encoder, hist_index.shape
    hist = model.news_encoder.encode_cached(news_cache, hist_index, user_freshness, user_lifetime).view(U, H, -1)
    flat_h = hist_index.reshape(-1).long()
    ucat, usub = corpus.news_category[flat_h].view(U, H), corpus.news_subCategory[flat_h].view(U, H)
    if n_src is None and hasattr(ue, 'user_node_embedding'):
        n_src = min(n_pairs, H + ue.user_node_embedding.shape[0])
    return Users(hist, ucat, usub, hist_mask, ue.gate_projection(hist), n_src)    # the gate's projection: once for every pass's histories


def pass_operands(model, users, u0, u1, slots, category, subCategory, pairs=None):
    """The user side of one pass -> Operands: the users u0:u1 of ``users``, each with ``slots`` groups, user-major (hist_div = slots: a
    user's groups share one history, never repeated in memory before the refinement); category / subCategory [n slots, 1]: what the
    user side reads of a group; ``pairs``: the pass's pairs where a row is materialised for each (None: tables).  Once per pass,
    whatever the number of candidate sets (time slots) matched against it."""
    H = users.hist.shape[1]
    return match_operands(model, users.hist[u0:u1], category, subCategory, users.ucat[u0:u1], users.usub[u0:u1], users.hist_mask[u0:u1],
                          pairs=pairs, n_src=users.n_src, hist_div=slots,
                          gate_y=None if users.gate_y is None else users.gate_y[u0 * H:u1 * H])


def pass_logits(model, news_cache, operands, cands, pick, group_offsets):
    """The candidate side of one pass and its match against ``operands`` -> the logits fp32 [pairs] in group order ([S, pairs] with
    ``cands.slots`` = S: one lime_grouped_match_schedule_f32 launch for all slots).  ``pick(t)``: the pass's part, in group order, of
    one of ``cands``' per-pair tensors; group_offsets int64 [groups + 1]: the groups' CSR over the pass's pairs, on the device or still
    on the host (the copy waits for the stream, so it stands behind the launches that do not read it).  Without tables a row is
    materialised per pair; with them the pair's table row is read in place and, for a LIME model, composed with its bucket pair's."""
    cand, at, occ, remaining = pass_candidates(model, news_cache, cands, pick)
    return click_logits(model, operands, cand, remaining, torch.as_tensor(group_offsets, device=news_cache.device),
                        tables=cands.tables, index=at, occ=occ)


def pass_candidates(model, news_cache, cands, pick):
    """The candidate side of one pass -> (cand [pairs, D] or None, index int32 [pairs] or None, occ or None, remaining): without
    tables a row is materialised per pair; with them the pair's table row is named and, for a LIME model, its bucket pair's."""
    ne, tables = model.news_encoder, cands.tables
    per_slot = (-1,) if cands.slots is None else (cands.slots, -1)
    cand = at = occ = None
    if tables is None:
        cand = ne.encode_cached(news_cache, pick(cands.index), pick(cands.freshness), pick(cands.lifetime))       # [pairs, D]
    else:
        at = newsEncoders._i32(pick(cands.position).reshape(-1)).contiguous()                 # int32 [pairs]: the pair's table row
        if tables.occurrence is not None:
            occ = ne.occurrence_ids_schedule(pick(cands.freshness).reshape(cands.slots or 1, -1), pick(cands.lifetime)).reshape(per_slot)
    return cand, at, occ, pick(cands.remaining).reshape(per_slot)


def score_pool(model, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_index, cand_freshness, cand_lifetime,
               n_src, pairs_per_pass, exclude_history, k=None, slot_offsets=None):
    """score_pool -> (scores [U, C], bool [U, C] "excluded" or None): the passes over recommend.pool_plan's ONE host plan.
    With ``slot_offsets`` [S] (score_schedule): scores [S, U, C], slot s at freshness ``cand_freshness + slot_offsets[s]`` (the sum
    made in fp32), by ``schedule_route(S, H)`` -- 'single': this very path at that freshness; 'shared': the user side once per
    call, the operands once per pass, the candidate side and the match once per slot; 'factorised': the call's tables
    (whatever LIME_INDEXED_MATCH / LIME_OCCURRENCE_MATCH say) and one lime_grouped_match_schedule_f32 launch per pass for all
    slots; 'expand': one slot, repeated."""
    C = cand_index.numel()
    entry = 'recommend' if slot_offsets is None else 'recommend_schedule'

    def check_candidates(U):
        for t, name in ((cand_freshness, 'cand_freshness'), (cand_lifetime, 'cand_lifetime')):
            if tuple(t.shape) not in ((C,), (U, C)):
                raise ValueError('%s must be [C] = [%d] or [U, C] = [%d, %d], got %s' % (name, C, U, C, tuple(t.shape)))
        if slot_offsets is not None and (slot_offsets.dim() != 1 or slot_offsets.numel() < 1 or not slot_offsets.is_floating_point()):
            raise ValueError('slot_offsets must be a float [S] with S >= 1 -- the slots\' offsets in the unit of the freshness --, got %s %s'
                             % (slot_offsets.dtype, tuple(slot_offsets.shape)))
    bad_index = 'cand_index must be [C] with C >= 1 -- ONE pool for all users --' if cand_index.dim() != 1 or C < 1 else None
    U, H, _ = check_grouped(model, news_cache, hist_index, hist_mask, user_freshness, user_lifetime, cand_index, bad_index, check_candidates,
                            pairs_per_pass, k, (entry, 'lime_topk_rows_f32'))
    c, dev = corpus, news_cache.device
    S = 1 if slot_offsets is None else slot_offsets.numel()
    route = 'single' if slot_offsets is None else model.schedule_route(S, H)
    factorised = route == 'factorised'
    offs = None if slot_offsets is None else slot_offsets.to(dev).float()
    if offs is not None and route in ('single', 'expand'):                 # one slot is computed (no slot is felt under 'expand')
        cand_freshness, offs = cand_freshness.to(dev).float() + offs[0], None
    sets = 1 if offs is None else S                                         # the candidate sets that are matched
    cidx = cand_index.to(dev).long()
    cat_c, sub_c = c.news_category[cidx], c.news_subCategory[cidx]
    plan = rec.pool_plan(cat_c.cpu().numpy(), sub_c.cpu().numpy(), model.grouped_by())
    T, order = plan.category.shape[0], torch.as_tensor(plan.order, device=dev)
    fresh, life = cand_freshness.to(dev).float().expand(U, C), cand_lifetime.to(dev).float().expand(U, C)
    fresh = fresh.unsqueeze(0) if offs is None else fresh.unsqueeze(0) + offs.view(S, 1, 1)            # [sets, U, C]
    remaining = model._lifetime_rule(fresh, lambda: life.unsqueeze(0).expand(sets, U, C),
                                     lambda: cat_c.view(1, 1, C).expand(sets, U, C)).float()
    # the pool in plan (topic) order: what every pass reads
    # (a baseline model: the pool's C rows and their Q, once per call)
    tables = model._candidate_tables(news_cache, cidx[order], always=factorised)
    index, life = cidx[order].unsqueeze(0).expand(U, C), life[:, order]
    fresh, remaining = fresh[:, :, order], remaining[:, :, order]
    position = None if tables is None else torch.arange(C, dtype=torch.int32, device=dev).unsqueeze(0).expand(U, C)
    users = user_side(model, news_cache, c, hist_index, hist_mask, user_freshness, user_lifetime, n_src, U * C)
    # (read in place, the candidates take no rows of a pass: the refined rows alone bound its users)
    per = rec.users_per_pass(U, C if tables is None else 0, T, H, int(pairs_per_pass))
    cat_t = torch.as_tensor(plan.category, device=dev).to(c.news_category.dtype)
    sub_t = torch.as_tensor(plan.subCategory, device=dev).to(c.news_subCategory.dtype)
    out = torch.empty((sets, U, C), dtype=torch.float32, device=dev)
    for u0 in range(0, U, per):
        u1 = min(U, u0 + per)
        n = u1 - u0
        operands = pass_operands(model, users, u0, u1, T, cat_t.repeat(n).view(n * T, 1), sub_t.repeat(n).view(n * T, 1),
                                 pairs=n * C if tables is None else None)
        goff = rec.group_offsets(plan.segments, n)
        of_pass = lambda t: t[..., u0:u1, :]                                # the pass's users, of [U, C] or [sets, U, C]
        for s in ([slice(None)] if factorised else range(sets)):            # every slot of the pass in one launch, or a launch each
            cands = Candidates(index, fresh[s], life, remaining[s], tables, position, sets if factorised else None)
            logits, part = pass_logits(model, news_cache, operands, cands, of_pass, goff), of_pass(out[s])
            part.index_copy_(-1, order, logits.view(part.shape))
    gone = _in_history(news_cache.shape[0], hist_index, hist_mask, cidx) if exclude_history else None
    if exclude_history:
        out.masked_fill_(gone.unsqueeze(0), float('-inf'))
    if slot_offsets is None:
        return out[0], gone
    return (out.repeat(S, 1, 1) if sets != S else out), gone


def topic_quota(corpus, max_per_topic, quota_by):
    """The refusals of ``max_per_topic`` / ``quota_by`` (ValueError, before any launch) -> None without a quota, or (q, the corpus'
    topic_of_news int32 [n_news] under ``quota_by`` -- device_data.topic_table_of --, its number of groups)."""
    if max_per_topic is None:
        return None
    if isinstance(max_per_topic, bool) or not isinstance(max_per_topic, numbers.Integral) or max_per_topic < 1:
        raise ValueError('max_per_topic must be an integer >= 1 (or None: no quota), got %r' % (max_per_topic,))
    if quota_by not in ('category', 'topic'):
        raise ValueError("quota_by must be 'category' or 'topic' (the (category, subCategory) pair), got %r" % (quota_by,))
    from .device_data import topic_table_of
    topic_of_news, cat_t, _ = topic_table_of(corpus, quota_by)
    if cat_t.numel() > rec.MAX_TOPICS:
        raise ValueError('the corpus has %d groups by %s, lime_topk_rows_quota_f32 counts up to %d' % (cat_t.numel(), quota_by, rec.MAX_TOPICS))
    return TopicQuota(int(max_per_topic), topic_of_news, cat_t.numel())


def _in_history(n_news, hist_index, hist_mask, cidx):
    """bool [U, C]: candidate j sits in a masked-in slot of user u's history."""
    U, H = hist_index.shape
    seen = torch.zeros((U, n_news), dtype=torch.bool, device=cidx.device)
    live = hist_mask.to(cidx.device).bool()
    users = torch.arange(U, device=cidx.device).unsqueeze(1).expand(U, H)
    seen[users[live], hist_index.to(cidx.device).long()[live]] = True
    return seen[:, cidx]


def _without(positions, gone):
    """The rule of every recommend entry without a quota (the quota kernels drop the excluded themselves): a returned position whose
    candidate is excluded -- ``gone``, bool like ``positions`` -- becomes -1; a slot that holds -1 already stays."""
    return torch.where(gone & (positions >= 0), torch.full_like(positions, -1), positions)


Diversity = collections.namedtuple('Diversity', 'lam shortlist table')
MMR_ROWS_MAX = 65535                  # lime_mmr_rows_f32's rows per launch


def content_columns(model, news_cache):
    """The default similarity table: the content columns of ``news_cache`` -- the whole row, under 'gated' its first c columns as a
    column view -- or None where the cache has none to offer (CNE, a malformed cache)."""
    if news_cache.dim() != 2 or news_cache.shape[1] == 0 or model.reads_content_mask:
        return None
    gated = not model.plain and model.news_encoder.fusion_method == 'gated'
    return news_cache[:, :model.news_encoder.base_news_encoder.news_embedding_dim] if gated else news_cache


def diversity(model, news_cache, k, mmr_lambda, shortlist, similarity):
    """The refusals of ``mmr_lambda`` / ``shortlist`` / ``similarity`` (ValueError, before any launch) -> None without MMR, or
    Diversity(lam, the shortlist's length -- default min(128, max(k, 64)) --, the similarity table fp32 [n_news, E] -- default the
    content columns of ``news_cache``: the whole row, under 'gated' its first c columns as a column view)."""
    if mmr_lambda is None:
        if shortlist is not None or similarity is not None:
            raise ValueError('shortlist and similarity are read with mmr_lambda alone: give mmr_lambda, or neither of them')
        return None
    if isinstance(mmr_lambda, bool) or not isinstance(mmr_lambda, numbers.Real) or not 0.0 <= mmr_lambda <= 1.0:
        raise ValueError('mmr_lambda must be a real number in [0, 1] (or None: no MMR), got %r' % (mmr_lambda,))
    k = int(k) if isinstance(k, numbers.Integral) and 1 <= k <= 128 else None     # (a bad k is check_grouped's to refuse)
    if shortlist is None:
        shortlist = min(128, max(k or 1, 64))
    elif isinstance(shortlist, bool) or not isinstance(shortlist, numbers.Integral) or not (k or 1) <= shortlist <= 128:
        raise ValueError('shortlist must be an integer in [k, 128] = [%s, 128], got %r' % (k if k else 'k', shortlist))
    table = similarity if similarity is not None else content_columns(model, news_cache)
    if table is not None:                                                         # (a bad cache is check_grouped's to refuse)
        if (not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or table.dim() != 2 or table.shape[0] != news_cache.shape[0]
                or table.shape[1] < 1 or table.shape[1] % 4 or table.device != news_cache.device
                or (table.shape[1] > 1 and table.stride(1) != 1)):
            raise ValueError('similarity must be fp32 [n_news, E] = [%d, E] on the cache\'s device with E a multiple of 4 and unit column '
                             'stride, got %s' % (news_cache.shape[0], '%s %s on %s' % (table.dtype, tuple(table.shape), table.device)
                                                 if isinstance(table, torch.Tensor) else repr(table)))
    return Diversity(float(mmr_lambda), int(shortlist), table)


def _reranked(select, positions, top, ids, k, rows_per_launch):
    """The tail that the re-ranked slates share: ``select(top rows, ids rows)`` -> picks int32 [rows, k] in launches of
    ``rows_per_launch`` rows (None: one launch), then the two gathers that turn the picks into positions and score bits."""
    top = top.contiguous()
    step = rows_per_launch or max(top.shape[0], 1)
    picks = torch.cat([select(top[r0:r0 + step], ids[r0:r0 + step].contiguous())
                       for r0 in range(0, top.shape[0], step)]) if top.shape[0] else top.new_empty((0, k), dtype=torch.int32)
    at, none = picks.clamp(min=0).long(), picks < 0
    return (torch.gather(positions, 1, at).masked_fill(none, -1), torch.gather(top, 1, at).masked_fill(none, float('-inf')))


def _diverse(div, positions, top, ids, k):
    """The tail of every recommend entry under MMR: ``positions`` / ``top`` [R, shortlist] the shortlist's (an entry that takes no
    part holds position -1), ``ids`` int32 [R, shortlist] the similarity row of each entry (-1: none) -> (positions int32 [R, k],
    scores fp32 [R, k]): ops.mmr_rows in launches of 65535 rows, then its picks turned into positions and score bits."""
    return _reranked(lambda s, i: ops.mmr_rows(s, i, div.table, div.lam, k), positions, top, ids, k, MMR_ROWS_MAX)


Calibration = collections.namedtuple('Calibration', 'lam shortlist by alpha weights topic_of_news n_keys')
CALIBRATE_MAX_H = 128                 # lime_calibrate_rows_f32's history slots


def calibration(k, calibrate_lambda, calibrate_by, calibrate_alpha, calibrate_weights, mmr_lambda, shortlist):
    """The refusals of ``calibrate_lambda`` / ``calibrate_by`` / ``calibrate_alpha`` / ``calibrate_weights`` that read nothing but
    their arguments (ValueError, before any launch and before the corpus is touched) -> None without calibration, or a Calibration
    whose corpus-bound fields ``bind_calibration`` fills (shortlist: the default is ``diversity``'s, min(128, max(k, 64)))."""
    if calibrate_lambda is None:
        if calibrate_by != 'category' or calibrate_alpha != rec.CALIBRATE_ALPHA or calibrate_weights is not None \
                or isinstance(calibrate_alpha, bool):
            raise ValueError('calibrate_by, calibrate_alpha and calibrate_weights are read with calibrate_lambda alone: give '
                             'calibrate_lambda, or leave them at their defaults')
        return None
    if isinstance(calibrate_lambda, bool) or not isinstance(calibrate_lambda, numbers.Real) or not 0.0 <= calibrate_lambda <= 1.0:
        raise ValueError('calibrate_lambda must be a real number in [0, 1] (or None: no calibration), got %r' % (calibrate_lambda,))
    if calibrate_by not in ('category', 'topic'):
        raise ValueError("calibrate_by must be 'category' or 'topic' (the (category, subCategory) pair), got %r" % (calibrate_by,))
    if isinstance(calibrate_alpha, bool) or not isinstance(calibrate_alpha, numbers.Real) or not 0.0 < calibrate_alpha < 1.0:
        raise ValueError('calibrate_alpha must be a real number in (0, 1), got %r' % (calibrate_alpha,))
    if calibrate_weights is not None and (not isinstance(calibrate_weights, torch.Tensor) or calibrate_weights.dtype != torch.float32
                                          or calibrate_weights.dim() != 2):
        raise ValueError('calibrate_weights must be an fp32 tensor [U, H] like hist_index, got %s'
                         % ('%s %s' % (calibrate_weights.dtype, tuple(calibrate_weights.shape))
                            if isinstance(calibrate_weights, torch.Tensor) else repr(calibrate_weights)))
    if mmr_lambda is not None:
        raise ValueError('calibrate_lambda together with mmr_lambda is out of scope: one selection trades relevance against either the '
                         'content similarity (mmr_lambda) or the topic mix (calibrate_lambda), not both')
    k = int(k) if isinstance(k, numbers.Integral) and 1 <= k <= 128 else None     # (a bad k is check_grouped's to refuse)
    if shortlist is None:
        shortlist = min(128, max(k or 1, 64))
    elif isinstance(shortlist, bool) or not isinstance(shortlist, numbers.Integral) or not (k or 1) <= shortlist <= 128:
        raise ValueError('shortlist must be an integer in [k, 128] = [%s, 128], got %r' % (k if k else 'k', shortlist))
    return Calibration(float(calibrate_lambda), int(shortlist), calibrate_by, float(calibrate_alpha), calibrate_weights, None, 0)


def bind_calibration(cal, corpus, hist_index, device):
    """The refusals of a calibrated call that read the corpus and the histories' shape (ValueError, before any launch) -> ``cal`` with
    the corpus' topic_of_news int32 [n_news] under ``cal.by`` and its number of groups; None stays None."""
    if cal is None:
        return None
    from .device_data import topic_table_of
    topic_of_news, cat_t, _ = topic_table_of(corpus, cal.by)
    if cat_t.numel() > rec.MAX_TOPICS:
        raise ValueError('the corpus has %d groups by %s, lime_calibrate_rows_f32 counts up to %d' % (cat_t.numel(), cal.by, rec.MAX_TOPICS))
    if isinstance(hist_index, torch.Tensor) and hist_index.dim() == 2:            # (another shape is check_grouped's to refuse)
        if hist_index.shape[1] > CALIBRATE_MAX_H:
            raise ValueError('a calibrated slate reads up to %d history slots (lime_calibrate_rows_f32), got H = %d'
                             % (CALIBRATE_MAX_H, hist_index.shape[1]))
        w = cal.weights
        if w is not None and (tuple(w.shape) != tuple(hist_index.shape) or w.device != torch.device(device)):
            raise ValueError('calibrate_weights must be fp32 [U, H] = %s on %s like the histories, got %s on %s'
                             % (list(hist_index.shape), device, list(w.shape), w.device))
    return cal._replace(topic_of_news=topic_of_news, n_keys=cat_t.numel())


def history_keys(topic_of_news, hist_index, hist_mask):
    """hist_keys int32 [U, H] of a calibrated call: the group (``topic_of_news`` int32 [n_news], Calibration's) of every history
    news, -1 where ``hist_mask`` is off."""
    dev = topic_of_news.device
    keys = topic_of_news[hist_index.to(dev).long()]
    return torch.where(hist_mask.to(dev).bool(), keys, torch.full_like(keys, -1)).to(torch.int32).contiguous()


def _calibrated(cal, hist_keys, positions, top, ids, k):
    """The tail of every recommend entry under calibration: as ``_diverse``, with ops.calibrate_rows in ONE launch (its grid strides
    over any number of rows, and row r reads history row r % U whatever the launch's first row would be)."""
    weights = None if cal.weights is None else cal.weights.contiguous()
    return _reranked(lambda s, i: ops.calibrate_rows(s, i, cal.topic_of_news, cal.n_keys, hist_keys, weights, cal.lam, cal.alpha, k),
                     positions, top, ids, k, None)


_NO_SLOTS = object()         # (not None: recommend_schedule hands ``slot_offsets`` to torch.as_tensor whatever it is)


def recommend(model, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_index, cand_freshness, cand_lifetime, k,
              n_src, pairs_per_pass, exclude_history, max_per_topic, quota_by, slot_offsets=_NO_SLOTS, mmr_lambda=None, shortlist=None,
              similarity=None, calibrate_lambda=None, calibrate_by='category', calibrate_alpha=rec.CALIBRATE_ALPHA, calibrate_weights=None):
    """recommend -> (positions int32 [U, k], scores fp32 [U, k]); with ``slot_offsets`` recommend_schedule -> [S, U, k] each:
    ``score_pool``, then the top k of every row of its scores -- for a schedule the rows of the [S U, C] view, in chunks of slots that
    keep the kernel's 65535 rows.  With ``mmr_lambda``: the top ``shortlist`` of every row the same way, then ``_diverse`` picks k of
    them (the similarity row of a shortlist entry is its news id; -1 for an empty or excluded one).  With ``calibrate_lambda``: the
    same shortlist and ids, of which ``_calibrated`` picks k against the topic mix of the row's history (row s U + u reads user u's)."""
    quota = topic_quota(corpus, max_per_topic, quota_by)
    cal = calibration(k, calibrate_lambda, calibrate_by, calibrate_alpha, calibrate_weights, mmr_lambda, shortlist)
    div = diversity(model, news_cache, k, mmr_lambda, shortlist if cal is None else None, similarity)
    cal = bind_calibration(cal, corpus, hist_index, news_cache.device)
    scores, gone = score_pool(model, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_index, cand_freshness,
                              cand_lifetime, n_src, pairs_per_pass, exclude_history, k=k,
                              slot_offsets=None if slot_offsets is _NO_SLOTS else torch.as_tensor(slot_offsets))
    if div is not None or cal is not None:
        M = div.shortlist if div is not None else cal.shortlist
        positions, top = _top_rows(scores, gone, quota, cand_index, M)
        cidx = newsEncoders._i32(cand_index.to(scores.device))
        ids = torch.where(positions >= 0, cidx[positions.clamp(min=0).long()], torch.full_like(positions, -1))
        positions, top, ids = positions.view(-1, M), top.view(-1, M), ids.view(-1, M)
        positions, top = (_diverse(div, positions, top, ids, int(k)) if div is not None else
                          _calibrated(cal, history_keys(cal.topic_of_news, hist_index, hist_mask), positions, top, ids, int(k)))
        return positions.view(scores.shape[:-1] + (int(k),)), top.view(scores.shape[:-1] + (int(k),))
    return _top_rows(scores, gone, quota, cand_index, int(k))


def _top_rows(scores, gone, quota, cand_index, k):
    """The k best of every row of ``score_pool``'s scores [U, C] or [S, U, C], under ``quota`` where one is given -> (positions,
    scores) [.., k]; an excluded candidate (``gone``) is never returned: its slot holds position -1."""
    (U, C), whole = scores.shape[-2:], scores.dim() == 2               # whole: the unscheduled pool, its rows as they are, no copy
    step = max(1, 65535 // max(U, 1))
    rows = [scores] if whole else [scores[s0:s0 + step].view(-1, C) for s0 in range(0, scores.shape[0], step)]
    if quota is not None:                                      # the kernel drops the excluded: nothing to replace afterwards
        keys = quota.topic_of_news[cand_index.to(scores.device).long()]
        found = [ops.topk_rows_quota(r, keys, quota.q, k, drop=gone, n_keys=quota.n_keys) for r in rows]
    else:
        found = [ops.topk_rows(r, k) for r in rows]
    positions, top = found[0] if whole else (torch.cat([f[i] for f in found]).view(scores.shape[0], U, k) for i in (0, 1))
    if gone is not None and quota is None:
        positions = _without(positions, gone.expand(scores.shape).gather(-1, positions.clamp(min=0).long()))
    return positions, top


def score_lists(model, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_offsets, cand_index, cand_freshness,
                cand_lifetime, n_src, pairs_per_pass, exclude_history, k=None):
    """score_lists -> (scores [P], the offsets on the device, bool [P] "excluded" or None): the passes over ops.list_plan's plan."""
    dev = news_cache.device
    call = list_call(model, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_offsets, cand_index,
                     cand_freshness, cand_lifetime, n_src, pairs_per_pass, k)
    if call.passes is None:
        return torch.empty((0,), dtype=torch.float32, device=dev), call.offsets, None
    out = torch.empty((cand_index.numel(),), dtype=torch.float32, device=dev)
    for t in call.passes:
        operands = pass_operands(model, call.users, t.u0, t.u1, t.slots, t.category, t.subCategory,
                                 pairs=t.rows.numel() if call.cands.tables is None else None)
        out.index_copy_(0, t.rows, pass_logits(model, news_cache, operands, call.cands, lambda x: x[t.rows], t.group_offsets))
    gone = _in_own_history(hist_index.to(dev), hist_mask.to(dev), call.offsets, call.cands.index) if exclude_history else None
    if exclude_history:
        out.masked_fill_(gone, float('-inf'))
    return out, call.offsets, gone


# A call over per-user lists, behind its host checks: the lists' offsets on the device, what every pass reads of the users and of the
# candidates, and the passes (None: no pair at all) -- each ListPass the users u0:u1 with ``slots`` groups each, the pass's pairs in
# group order (``rows`` into the call's [P] arrays), their groups' CSR and the topic (category, subCategory [groups, 1]) of every group.
ListCall = collections.namedtuple('ListCall', 'offsets users cands passes')
ListPass = collections.namedtuple('ListPass', 'u0 u1 slots rows group_offsets category subCategory')


def list_call(model, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_offsets, cand_index, cand_freshness,
              cand_lifetime, n_src, pairs_per_pass, k=None):
    """What ``score_lists`` and ``explain_lists`` share: the host refusals, the plan of the lists (ops.list_plan), the once-per-call
    user side and candidate tables, and the passes over the plan -> ListCall (``passes`` a generator: a pass with fewer slots than
    the call plans itself when it is reached)."""
    import numpy as np
    from .device_data import topic_table_of
    P = cand_index.numel()

    def check_candidates(U):
        off = cand_offsets.detach().cpu().numpy() if isinstance(cand_offsets, torch.Tensor) else np.asarray(cand_offsets)
        if off.ndim != 1 or off.shape[0] != U + 1 or off.dtype.kind not in 'iu':
            raise ValueError('cand_offsets must be U + 1 = %d integers (the CSR of the lists), got %s %s' % (U + 1, off.dtype, off.shape))
        off = off.astype(np.int64)
        if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != P:
            raise ValueError('cand_offsets must start at 0, not decrease and end at P = %d, got %d .. %d%s'
                             % (P, off[0], off[-1], ' (decreasing)' if (np.diff(off) < 0).any() else ''))
        for t, name in ((cand_freshness, 'cand_freshness'), (cand_lifetime, 'cand_lifetime')):
            if tuple(t.shape) != (P,):
                raise ValueError('%s must be [P] = [%d], got %s' % (name, P, tuple(t.shape)))
        return off
    bad_index = 'cand_index must be [P], the lists one behind the other,' if cand_index.dim() != 1 else None
    U, H, off = check_grouped(model, news_cache, hist_index, hist_mask, user_freshness, user_lifetime, cand_index, bad_index,
                              check_candidates, pairs_per_pass, k, ('recommend_lists', 'lime_topk_segments_f32'))
    dev = news_cache.device
    offsets = torch.from_numpy(off).to(dev)
    if P == 0:
        return ListCall(offsets, None, None, None)
    topic_of_news, cat_t, sub_t = topic_table_of(corpus, model.grouped_by())
    if cat_t.numel() > rec.MAX_TOPICS:
        raise ValueError('the corpus has %d topics, lime_list_plan groups up to %d' % (cat_t.numel(), rec.MAX_TOPICS))
    cidx = cand_index.to(dev).long()
    fresh, life = cand_freshness.to(dev).float(), cand_lifetime.to(dev).float()
    remaining = model._lifetime_rule(fresh, lambda: life, lambda: corpus.news_category[cidx]).float()
    keys = topic_of_news[cidx]
    plan = ops.list_plan(keys, offsets, n_keys=cat_t.numel())                      # the call's one device -> host read
    S = (plan.slot_key.numel() // U) if U else 1
    users = user_side(model, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, n_src, P)
    tables = model._candidate_tables(news_cache)                  # (a baseline model: the cache itself, and Q of every news once)
    cands = Candidates(cidx, fresh, life, remaining, tables, cidx, None)           # (a pair's table row is its news id)

    def passes():
        for u0, u1, S_pass in rec.list_passes(off, plan.n_distinct, H, int(pairs_per_pass)):
            p0, p1 = int(off[u0]), int(off[u1])
            if p1 == p0:
                continue
            if S_pass == S:                                                       # the pass's plan is a slice of the call's
                rows, goff, skey = plan.order[p0:p1], plan.group_offsets[u0 * S:u1 * S + 1] - p0, plan.slot_key[u0 * S:u1 * S]
            else:                                                                 # fewer slots suffice: no slot count is read again
                sub = ops.list_plan(keys[p0:p1], offsets[u0:u1 + 1] - p0, slots=S_pass, n_keys=cat_t.numel(),
                                    n_distinct=plan.n_distinct[u0:u1])
                rows, goff, skey = sub.order + p0, sub.group_offsets, sub.slot_key
            skey = skey.long()
            yield ListPass(u0, u1, S_pass, rows, goff.contiguous(), cat_t[skey].view(-1, 1), sub_t[skey].view(-1, 1))
    return ListCall(offsets, users, cands, passes())


def _in_own_history(hist_index, hist_mask, offsets, cidx, pairs_per_step=1 << 18):
    """bool [P]: the candidate of pair p sits in a masked-in slot of ITS user's history -- per pair against the user's H slots."""
    U, P = hist_index.shape[0], cidx.numel()
    user = torch.repeat_interleave(torch.arange(U, device=cidx.device), offsets[1:] - offsets[:-1], output_size=P)
    hist, live = hist_index.long(), hist_mask.bool()
    gone = torch.empty((P,), dtype=torch.bool, device=cidx.device)
    for p0 in range(0, P, pairs_per_step):
        u = user[p0:p0 + pairs_per_step]
        gone[p0:p0 + pairs_per_step] = ((hist[u] == cidx[p0:p0 + pairs_per_step].unsqueeze(1)) & live[u]).any(dim=1)
    return gone


def recommend_lists(model, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_offsets, cand_index, cand_freshness,
                    cand_lifetime, k, n_src, pairs_per_pass, exclude_history, max_per_topic, quota_by, mmr_lambda=None, shortlist=None,
                    similarity=None, calibrate_lambda=None, calibrate_by='category', calibrate_alpha=rec.CALIBRATE_ALPHA,
                    calibrate_weights=None):
    """recommend_lists -> (positions int32 [U, k] into the user's list, scores fp32 [U, k]): ``score_lists``, then the top k of every
    segment of its scores.  With ``mmr_lambda``: the top ``shortlist`` of every segment the same way, then ``_diverse`` picks k of
    them (the similarity row of a shortlist entry is the news id at its place in the user's list).  With ``calibrate_lambda``: the
    same shortlist and ids, of which ``_calibrated`` picks k against the topic mix of the user's history."""
    quota = topic_quota(corpus, max_per_topic, quota_by)
    cal = calibration(k, calibrate_lambda, calibrate_by, calibrate_alpha, calibrate_weights, mmr_lambda, shortlist)
    div = diversity(model, news_cache, k, mmr_lambda, shortlist if cal is None else None, similarity)
    cal = bind_calibration(cal, corpus, hist_index, news_cache.device)
    scores, offsets, gone = score_lists(model, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_offsets,
                                        cand_index, cand_freshness, cand_lifetime, n_src, pairs_per_pass, exclude_history, k=k)
    return select_segments(scores, offsets, gone, quota, div, cand_index, k, cal=cal,
                           hist_keys=None if cal is None else history_keys(cal.topic_of_news, hist_index, hist_mask))


def select_segments(scores, offsets, gone, quota, div, cand_index, k, cal=None, hist_keys=None):
    """The slates of a score buffer, the tail of ``recommend_lists`` and the selection ``util.evaluate_slates_on_device`` sweeps:
    ``scores`` fp32 [P] and ``offsets`` int64 [U + 1] (device) the lists' CSR, ``gone`` bool [P] or None the excluded pairs, ``quota``
    a TopicQuota or None, ``div`` a Diversity or None, ``cand_index`` [P] the news of every pair -> (positions int32 [U, k] into the
    user's list, scores fp32 [U, k]): the top k of every segment, under the quota where one is given; with ``div`` the top
    ``div.shortlist`` the same way, of which ``_diverse`` picks k (the similarity row of a shortlist entry is the news id at its
    place in the user's list); with ``cal`` (a Calibration whose target fields are filled; not together with ``div``) and
    ``hist_keys`` int32 [U, H] (``history_keys``) the top ``cal.shortlist``, of which ``_calibrated`` picks k.  Without a pair every
    slot holds -1 / -inf."""
    U, k = offsets.numel() - 1, int(k)
    if div is not None and cal is not None:
        raise ValueError('select_segments takes a Diversity or a Calibration, not both')
    if scores.numel() == 0:
        return (torch.full((U, k), -1, dtype=torch.int32, device=scores.device),
                torch.full((U, k), float('-inf'), dtype=torch.float32, device=scores.device))
    if div is None and cal is None:
        return _top_segments(scores, offsets, gone, quota, cand_index, k)
    positions, top = _top_segments(scores, offsets, gone, quota, cand_index, div.shortlist if div is not None else cal.shortlist)
    pair = (offsets[:-1].unsqueeze(1) + positions.clamp(min=0).long()).clamp(max=scores.numel() - 1)
    ids = torch.where(positions >= 0, newsEncoders._i32(cand_index.to(scores.device))[pair], torch.full_like(positions, -1))
    return _diverse(div, positions, top, ids, k) if div is not None else _calibrated(cal, hist_keys, positions, top, ids, k)


def _top_segments(scores, offsets, gone, quota, cand_index, k):
    """The k best of every segment of ``score_lists``' scores, under ``quota`` where one is given -> (positions, scores) [U, k]; an
    excluded candidate (``gone``) is never returned: its slot holds position -1."""
    if quota is not None:
        return ops.topk_segments_quota(scores, offsets, quota.topic_of_news[cand_index.to(scores.device).long()], quota.q, k, drop=gone,
                                       n_keys=quota.n_keys)
    positions, top = ops.topk_segments(scores, offsets, k)
    if gone is not None:
        positions = _without(positions, gone[(offsets[:-1].unsqueeze(1) + positions.clamp(min=0).long()).clamp(max=scores.numel() - 1)])
    return positions, top


# ---- explanations: why a news is in the slate (Model.explain_lists / Model.explain) ----------------------------------------------------
# Per pair, in the caller's order: score [P] (what ``score_lists`` gives the pair), base and weight [P] (score = base weight: the
# match before the remaining-lifetime weight, and that weight), slots int32 / values fp32 [P, top] (positions into the user's history
# row, best first, -1 / 0 behind the last masked-in one), attention / contribution fp32 [P, H] or None.
Explanation = collections.namedtuple('Explanation', 'score base weight slots values attention contribution')


def check_explain(model, hist_index, top, by):
    """The refusals of ``top`` / ``by`` (ValueError, before any launch and before the shared checks), behind CNE's."""
    if model.reads_content_mask:
        raise ValueError(model._NO_CONTENT_CACHE)
    if by not in rec.EXPLAIN_BY:
        raise ValueError("by must be 'contribution' or 'attention', got %r" % (by,))
    if by == 'contribution' and model.click_predictor == 'mlp':
        raise ValueError("by='contribution' needs the dot-product click predictor: behind the MLP predictor's ReLU the logit is no sum "
                         "over the history slots -- by='attention' is served")
    H = hist_index.shape[1] if isinstance(hist_index, torch.Tensor) and hist_index.dim() == 2 else None     # (else check_grouped's to refuse)
    most = rec.EXPLAIN_MAX_TOP if H is None else min(rec.EXPLAIN_MAX_TOP, H)
    if isinstance(top, bool) or not isinstance(top, numbers.Integral) or not 1 <= top <= most:
        raise ValueError('top must be an integer in 1 .. min(%d, H)%s, got %r' % (rec.EXPLAIN_MAX_TOP, '' if H is None else ' = %d' % most, top))


def _first_one(rows, device):
    """[rows, 4] rows (1, 0, 0, 0): the pair's side of a score that sits in column 0 of kp."""
    q = torch.zeros((rows, 4), dtype=torch.float32, device=device)
    q[:, 0] = 1.0
    return q


def explain_operands(model, users, u0, u1, slots, category, subCategory, pairs=None):
    """``pass_operands`` with the history slots kept apart -> Operands over H rows per group, whichever the user encoder.  CROWN: the
    operands of the match as they are.  ATT / MHSA: the user vector is the additive pool sum_h beta[h] x[h], so g = x, the rows
    ``_pool_inputs`` pools; kp [G H, 4] holds the pool's logit affine2 . hidden[h] in column 0 and zeros behind it, and a pair's qp is
    (1, 0, 0, 0) with scale 1: the match's softmax IS beta, and its per-slot term beta[h] (x[h] . cand).  Under MHSA x[h] is the
    self-attended row of slot h -- a term belongs to the click in the context of the others."""
    ue = model.user_encoder
    if hasattr(ue, 'user_node_embedding'):
        return pass_operands(model, users, u0, u1, slots, category, subCategory, pairs=pairs)
    H = users.hist.shape[1]
    x, hidden, rows = ue._pool_inputs(users.hist[u0:u1], category, subCategory, users.ucat[u0:u1], users.usub[u0:u1], users.hist_mask[u0:u1],
                                      None, slots, None if users.gate_y is None else users.gate_y[u0 * H:u1 * H], None)
    if rows != (u1 - u0) * slots:
        raise ValueError('the user side gave %d histories for %d groups' % (rows, (u1 - u0) * slots))
    w = ue.attention.affine2.weight
    w4 = torch.zeros((4, w.shape[1]), dtype=torch.float32, device=w.device)
    w4[0] = w[0]
    return Operands(x, ops.linear(hidden, w4, None), None if pairs is None else _first_one(pairs, x.device), H, 1.0)


def explain_lists(model, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_offsets, cand_index, cand_freshness,
                  cand_lifetime, top, by, dense, n_src, pairs_per_pass):
    """explain_lists -> Explanation: ``score_lists``' plan, passes, user side and candidate tables, with the terms of every pair kept
    by the last launch (lime_grouped_match_explain_f32).  Under the MLP predictor (``by`` 'attention' alone) the score is the existing
    MLP match's, weight is 1 and base the score."""
    check_explain(model, hist_index, top, by)
    call = list_call(model, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_offsets, cand_index,
                     cand_freshness, cand_lifetime, n_src, pairs_per_pass)
    ue, w, dev = model.user_encoder, model.remaining_lifetime_weighting, news_cache.device
    (U, H), P, top = hist_index.shape, cand_index.numel(), int(top)
    crown, mlp = hasattr(ue, 'user_node_embedding'), model.click_predictor == 'mlp'
    new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
    out = Explanation(new(P), new(P), new(P), new(P, top, dtype=torch.int32), new(P, top), new(P, H) if dense else None,
                      new(P, H) if dense and not mlp else None)
    if call.passes is None:
        return out
    cands = call.cands
    tables = cands.tables
    if tables is not None and not crown:                      # the pooled encoders' score column: (1, 0, 0, 0) + the occurrence's zeros
        tables = tables._replace(qp=_first_one(tables.cand.shape[0], dev))
    occurrence = None if tables is None else tables.occurrence
    mask = hist_mask.to(dev).bool()
    for t in call.passes:
        pairs = t.rows.numel() if tables is None else None
        operands = explain_operands(model, call.users, t.u0, t.u1, t.slots, t.category, t.subCategory, pairs=pairs)
        cand, at, occ, remaining = pass_candidates(model, news_cache, cands, lambda x: x[t.rows])
        goff = torch.as_tensor(t.group_offsets, device=dev)
        if tables is not None:
            rows_c, qp = tables.cand, tables.qp
        else:
            rows_c, qp = cand, operands.qp if operands.qp is not None else ops.linear(cand, ue.Q.weight, ue.Q.bias)
        composed = dict(occ=occ, qt=occurrence.qt, ct=occurrence.ct) if occurrence is not None else {}
        terms = ops.grouped_match_explain(operands.kp, operands.g, qp, rows_c, remaining, goff, operands.H, operands.scale, w.alpha, w.beta,
                                          bool(w.use_remaining_lifetime_weighting) and not mlp, bool(w.use_expired_penalty),
                                          mask=mask[t.u0:t.u1].contiguous(), hist_div=t.slots, m=top, by=by, dense=dense, index=at, **composed)
        if mlp:                                               # the score is the existing MLP match's, on ITS operands
            scored = operands if crown else pass_operands(model, call.users, t.u0, t.u1, t.slots, t.category, t.subCategory, pairs=pairs)
            score = click_logits(model, scored, cand, remaining, goff, tables=cands.tables, index=at, occ=occ)
            terms = terms._replace(logits=score, base=score, weight=torch.ones_like(score), contrib=None)
        for dst, src in zip(out, (terms.logits, terms.base, terms.weight, terms.top_slot, terms.top_value, terms.attn, terms.contrib)):
            if dst is not None:
                dst.index_copy_(0, t.rows, src)
    return out


def explain(model, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_index, cand_freshness, cand_lifetime,
            positions, top, by, dense, n_src, pairs_per_pass):
    """explain -> Explanation shaped [U, k, ...]: ``explain_lists`` over the lists that ``positions`` int [U, k] (``recommend``'s, or a
    slot of ``recommend_schedule``'s at that slot's freshness) name in the pool, unfilled entries (-1) left out of them and returned as
    score -inf, base -inf, weight 1, slots -1, zeros elsewhere.  ``n_src`` defaults as in ``score_pool``, so a score has its bits."""
    check_explain(model, hist_index, top, by)
    if not isinstance(hist_index, torch.Tensor) or hist_index.dim() != 2:
        raise ValueError('hist_index must be [U, H], got %s' % (tuple(getattr(hist_index, 'shape', ())),))
    (U, H), C, dev, ue = hist_index.shape, cand_index.numel(), news_cache.device, model.user_encoder
    if cand_index.dim() != 1 or C < 1:
        raise ValueError('cand_index must be [C] with C >= 1 -- ONE pool for all users -- got %s' % (tuple(cand_index.shape),))
    if (not isinstance(positions, torch.Tensor) or positions.dim() != 2 or positions.shape[0] != U
            or positions.dtype not in (torch.int32, torch.int64)):
        raise ValueError('positions must be the int [U, k] = [%d, k] positions into the pool that recommend returned, got %s'
                         % (U, '%s %s' % (positions.dtype, tuple(positions.shape)) if isinstance(positions, torch.Tensor) else repr(positions)))
    for t, name in ((cand_freshness, 'cand_freshness'), (cand_lifetime, 'cand_lifetime')):
        if tuple(t.shape) not in ((C,), (U, C)):
            raise ValueError('%s must be [C] = [%d] or [U, C] = [%d, %d], got %s' % (name, C, U, C, tuple(t.shape)))
    pos = positions.to(dev).long()
    k = pos.shape[1]
    filled = (pos >= 0) & (pos < C)
    u_of, j_of = filled.nonzero(as_tuple=True)                # user-major, slot order: the lists one behind the other
    at = pos[u_of, j_of]
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), filled.sum(dim=1).cumsum(0)])
    fresh, life = (t.to(dev).float().expand(U, C)[u_of, at] for t in (cand_freshness, cand_lifetime))
    if n_src is None and hasattr(ue, 'user_node_embedding'):
        n_src = min(U * C, H + ue.user_node_embedding.shape[0])
    ex = explain_lists(model, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, off, cand_index.to(dev)[at], fresh,
                       life, top, by, dense, n_src, pairs_per_pass)
    fills = (float('-inf'), float('-inf'), 1.0, -1, 0.0, 0.0, 0.0)
    whole = []
    for part, fill in zip(ex, fills):
        if part is None:
            whole.append(None)
            continue
        full = torch.full((U, k) + tuple(part.shape[1:]), fill, dtype=part.dtype, device=dev)
        full[u_of, j_of] = part
        whole.append(full)
    return Explanation(*whole)
