"""Drop-in for the scoring-path part of the reference's util.py: RemainingLifetimeWeighting (util.py:15-52) and the
eval harness around the model, compute_scores (util.py:77-129)."""
import numpy as np
import torch
import torch.nn as nn

from . import ops
from .evaluate import device_scoring, scoring


class RemainingLifetimeWeighting(nn.Module):
    """Dot-product interest match x sigmoid remaining-lifetime weight (util.py:23-49) as one HIP kernel."""

    def __init__(self, config):
        super().__init__()
        self.alpha = config.sigmoid_scaling_alpha
        self.beta = config.penalty_scaling_beta
        self.use_expired_penalty = config.use_expired_penalty
        self.use_remaining_lifetime_weighting = config.use_remaining_lifetime_weighting

    def forward(self, user_embedding, news_embedding, remaining_lifetime):
        if torch.is_grad_enabled() and (user_embedding.requires_grad or news_embedding.requires_grad):
            from . import training
            return training.lifetime_weighted_logits(self, user_embedding, news_embedding, remaining_lifetime)
        return ops.lifetime_score(user_embedding, news_embedding, remaining_lifetime, self.alpha, self.beta,
                                  self.use_remaining_lifetime_weighting, self.use_expired_penalty)

    def initialize(self):
        pass


def rank_impressions(scores, indices):
    """util.py:113-123: per impression, the 1-based rank of every candidate under a stable descending sort (ties keep
    the candidate order; +0.0 and -0.0 tie).  ``scores``: one per row; ``indices``: the impression of each row
    (non-decreasing, 0-based; impressions without rows get an empty list).  Returns a list of rank lists."""
    scores = np.asarray(scores, dtype=np.float64)
    indices = np.asarray(indices, dtype=np.int64)
    n_imp = int(indices[-1]) + 1 if indices.size else 0
    pos = np.arange(scores.size)
    order = np.lexsort((pos, -scores, indices))             # by impression, then score descending, then candidate order
    starts = np.searchsorted(indices, np.arange(n_imp), side='left')
    counts = np.bincount(indices, minlength=n_imp)
    rank = np.empty(scores.size, dtype=np.int64)
    rank[order] = pos - np.repeat(starts, counts) + 1       # position inside the impression's sorted block
    return [rank[starts[i]:starts[i] + counts[i]].tolist() for i in range(n_imp)]


def write_rank_file(result_file, ranks):
    """util.py:117-123: ``<impression> [r1,r2,...]`` lines, 1-based impression ids, no spaces, no trailing newline."""
    with open(result_file, 'w', encoding='utf-8') as f:
        for i, r in enumerate(ranks):
            f.write(('' if i == 0 else '\n') + str(i + 1) + ' ' + str(r).replace(' ', ''))


def compute_scores(model, batches, indices, result_file, truth_file=None):
    """The reference's dev / test pass (util.py:77-129) over an iterable of 25-tensor batches (what DevTest_Dataset
    yields, dataset.py:216-227): score every (impression, candidate) row with the model in eval mode, write the rank
    file, and -- given the truth file -- return (AUC, MRR, nDCG@5, nDCG@10), else four Nones.  The remaining lifetime is
    derived per ``config.lifetime_type`` exactly as util.py:98-106."""
    config = model.config
    dev = getattr(model, 'device', None) or next(model.parameters()).device
    scores = []
    was_training = model.training
    model.eval()
    with torch.no_grad():
        for batch in batches:
            batch = [x.to(dev, non_blocking=True) for x in batch]
            news_category, news_freshness, news_user_topic_lifetime = batch[15], batch[23], batch[24]
            if config.lifetime_type == 'fixed':
                remaining_lifetime = config.fixed_lifetime - news_freshness
            elif config.lifetime_type == 'topic_wise':
                remaining_lifetime = config.category_lifetime_map.to(news_category.device)[news_category.long()] - news_freshness
            elif config.lifetime_type == 'user_topic':
                remaining_lifetime = news_user_topic_lifetime - news_freshness
            else:
                raise ValueError('Invalid lifetime_type')
            scores.append(model(*batch, remaining_lifetime).squeeze(dim=1).float().cpu())
    model.train(was_training)
    scores = torch.cat(scores).tolist() if scores else []
    assert len(scores) == len(indices), 'one score per (impression, candidate) row'
    write_rank_file(result_file, rank_impressions(scores, indices))
    if truth_file is None:
        return None, None, None, None
    with open(truth_file, 'r', encoding='utf-8') as truth_f, open(result_file, 'r', encoding='utf-8') as result_f:
        return scoring(truth_f, result_f)


def compute_scores_cached(model, behaviors, indices, result_file, truth_file=None, rows_per_forward=None, recurrence_cache=False):
    """The same dev / test pass from a per-news content cache (Model.build_news_cache + Model.score_behaviors): every news goes
    through the token encoders ONCE instead of once per (row, slot) -- the reference re-encodes all 51 news of every row
    (util.py:86-111).  ``behaviors``: a dev / test ``DeviceBehaviors``.  Rows are scored in chunks of ``rows_per_forward`` (default:
    config.batch_size, as trainer.py:153 calls compute_scores; main.py:50,67 pass twice that, which only fits while
    2 x batch_size <= H + config.batch_size node slots) with the chunk's row count as the GraphSAGE source count, so the scores
    are those of ``compute_scores`` over the same batches; the remaining lifetime follows ``config.lifetime_type``
    ('fixed' / 'topic_wise' / 'user_topic', util.py:98-106).

    Under the CNE content encoder there is nothing to cache per news (its gates read the memory vector of another news of the same
    encoder call): the cache is empty, every chunk of rows is encoded as ``compute_scores`` would encode that batch, and the scores
    equal ``compute_scores``' only when the chunks are its batches (CNE's scores depend on the batch's composition).
    ``recurrence_cache`` = True (CNE alone): the recurrence of every news is cached once per call (Model.build_recurrence_cache) and
    every chunk is scored from it -- the same chunks, the same partners, no LSTM step per chunk."""
    config = model.config
    if config.lifetime_type not in ('fixed', 'topic_wise', 'user_topic'):
        raise ValueError('Invalid lifetime_type')
    per = rows_per_forward or config.batch_size
    nodes = getattr(model.user_encoder, 'user_node_embedding', None)       # CROWN's GraphSAGE node slots; ATT / MHSA have no such bound
    slots = behaviors.hist_index.shape[1] + nodes.shape[0] if nodes is not None else per
    if per > slots:
        raise ValueError('rows_per_forward = %d exceeds the H + config.batch_size = %d GraphSAGE node slots (SURVEY Q7): the '
                         'reference raises an index error there' % (per, slots))
    was_training = model.training
    model.eval()
    cache = model.build_news_cache(behaviors.corpus)
    rc = dict(recurrence_cache=model.build_recurrence_cache(behaviors.corpus), rows_per_forward=per) if recurrence_cache else {}
    scores = []
    for r0 in range(0, behaviors.num, per):
        rows = list(range(r0, min(behaviors.num, r0 + per)))
        scores.append(model.score_behaviors(behaviors, rows, cache, n_src=len(rows), **rc).float().cpu())
    model.train(was_training)
    scores = torch.cat(scores).tolist() if scores else []
    assert len(scores) == len(indices), 'one score per (impression, candidate) row'
    write_rank_file(result_file, rank_impressions(scores, indices))
    if truth_file is None:
        return None, None, None, None
    with open(truth_file, 'r', encoding='utf-8') as truth_f, open(result_file, 'r', encoding='utf-8') as result_f:
        return scoring(truth_f, result_f)


def ranks_to_lists(ranks, indices):
    """Device (or host) ranks, one per row -> the per-impression rank lists ``rank_impressions`` returns for the same rows: the
    impressions 0 .. indices[-1], an empty list for an impression without rows."""
    ranks = ranks.cpu().numpy() if isinstance(ranks, torch.Tensor) else np.asarray(ranks)
    indices = np.asarray(indices, dtype=np.int64)
    n_imp = int(indices[-1]) + 1 if indices.size else 0
    bounds = np.searchsorted(indices, np.arange(n_imp + 1), side='left')
    flat = ranks.tolist()
    return [flat[bounds[i]:bounds[i + 1]] for i in range(n_imp)]


# rows of one score_behaviors pass of evaluate_cached_on_device.  The user side of a pass materialises a few [rows, H, D] fp32
# tensors: 0.41 MB a row measured at the default configuration (H = 50), 3.4 GB for the 8192 rows of the default; the whole pass takes
# the same time from 4096 rows a pass up (DESIGN.md "Device-side evaluation", tools/bench_eval.py).
DEVICE_EVAL_ROWS_PER_PASS = 8192
# ... and with CNE's recurrence cache.  A CNE pass holds token-level tensors for every news of every row: per row H + 1 news of
# T + L token slots with the gated rows, the attention's hidden state and the cross terms (2h + attention_dim + 2h floats a slot),
# 51 . 160 . 7.2 KB = 59 MB a row at the defaults (computed from the shapes, not measured), 15 GB for 256 rows.
CNE_CACHED_ROWS_PER_PASS = 256


def impression_runs(indices, r0, r1):
    """The runs of equal values in indices[r0:r1] -> their first rows, int64 [n_runs + 1] ending with r1 (host)."""
    idx = np.asarray(indices, dtype=np.int64)[r0:r1]
    starts = np.flatnonzero(np.concatenate([[True], idx[1:] != idx[:-1]])) if idx.size else np.zeros(0, dtype=np.int64)
    return np.concatenate([starts + r0, [r1]]).astype(np.int64)


def check_one_history_per_impression(behaviors, indices):
    """ValueError unless all rows of every impression (run of equal values in ``indices``) carry identical hist_index / hist_mask /
    user_freshness / user_lifetime: compared on the device, one flag read back; remembered on ``behaviors`` once it holds."""
    b = behaviors
    if getattr(b, '_one_history_per_impression', False) or b.num < 2:
        return
    dev = b.hist_index.device
    idx = torch.as_tensor(np.asarray(indices, dtype=np.int64), device=dev)
    differs = torch.zeros(b.num - 1, dtype=torch.bool, device=dev)
    for t in (b.hist_index, b.hist_mask, b.user_freshness, b.user_lifetime):
        differs |= (t[1:] != t[:-1]).any(dim=1)
    bad = differs & (idx[1:] == idx[:-1])
    if bool(bad.any()):
        row = int(torch.nonzero(bad)[0]) + 1
        raise ValueError('impression %d: row %d carries another history than the row before it -- the grouped dev pass reads an '
                         'impression\'s history from its first row' % (int(idx[row]), row))
    b._one_history_per_impression = True


def _score_grouped(model, behaviors, indices, cache, scores, full, per, rows_per_pass):
    """evaluate_cached_on_device(grouped=True): rows [0, full) with n_src = per, rows [full, num) with n_src = their count, each as
    one ``score_lists`` call over the impressions' lists, into ``scores``."""
    b = behaviors
    check_one_history_per_impression(b, indices)
    dev, H = cache.device, b.hist_index.shape[1]
    for r0, r1, n_src in ((0, full, per), (full, b.num, b.num - full)):
        if r1 == r0:
            continue
        runs = impression_runs(indices, r0, r1)
        first = torch.from_numpy(runs[:-1]).to(dev)
        scores[r0:r1] = model.score_lists(cache, b.corpus, b.hist_index[first], b.hist_mask[first], b.user_freshness[first],
                                          b.user_lifetime[first], runs - r0, b.cand_index[r0:r1].reshape(-1),
                                          b.cand_freshness[r0:r1].reshape(-1), b.cand_lifetime[r0:r1].reshape(-1), n_src=n_src,
                                          pairs_per_pass=max(1, rows_per_pass * H))


def evaluate_cached_on_device(model, behaviors, indices, labels, result_file=None, rows_per_forward=None,
                              rows_per_pass=DEVICE_EVAL_ROWS_PER_PASS, return_scores=False, recurrence_cache=False, grouped=False,
                              news_cache=None):
    """The dev / test pass of ``compute_scores_cached`` without host round trips: one ``build_news_cache``, ``score_behaviors`` in
    passes of up to ``rows_per_pass`` rows that write into ONE device score buffer, one ``evaluate.device_scoring`` (ranks and
    metrics in one launch, csrc/rank_metrics.hip), one device -> host copy of the result.  ``labels``: the per-impression label
    lists (corpus.dev_labels / formats.truth_labels) in place of the truth file.  Returns (AUC, MRR, nDCG@5, nDCG@10); with
    ``result_file`` the rank file is written from the device ranks -- the bytes ``rank_impressions`` gives for the same scores; with
    ``return_scores`` the result is (metrics, the fp32 device score buffer).

    The scores are those of ``compute_scores_cached(..., rows_per_forward)``: a row's score depends on the row count of the
    reference's forward through the GraphSAGE source count and on nothing else of its pass, so the rows of the full
    ``rows_per_forward`` chunks are scored many chunks at a time with n_src = rows_per_forward, and the rows of the last, short chunk
    with n_src = its length.  (A pass of another row count may take GEMM kernels with another summation order: equal to fp32
    rounding, bitwise equal when rows_per_pass == rows_per_forward.)  ``rows_per_pass`` bounds memory: a pass allocates 0.41 MB a row at the
    default configuration (H = 50; measured, tools/bench_eval.py), 3.4 GB for the default of 8192 rows, and the whole pass is no
    faster with more.

    Under the CNE content encoder a score also depends on the other rows of its encoder call (the gates' partners).  Without
    ``recurrence_cache`` the CNE scores are those of ONE forward per pass of ``rows_per_pass`` rows, not of ``rows_per_forward``-row
    forwards.  ``recurrence_cache`` = True (CNE alone) builds the per-news recurrence cache once per call
    (Model.build_recurrence_cache) and passes it on with ``rows_per_forward``: a pass then scores many reference-sized chunks in one
    launch chain and still pairs the gates per chunk, which gives the scores of ``compute_scores_cached(..., rows_per_forward)``; a
    pass then holds at most CNE_CACHED_ROWS_PER_PASS rows (59 MB of token-level tensors a row at the defaults).

    ``grouped`` = True: the rows go through ``Model.score_lists`` instead -- an impression (a run of equal values in ``indices``) is
    one user with its rows as its candidate list and the history of its first row, so the user side runs once per (impression,
    candidate topic) and not once per row.  The chunk rule is kept: the rows of the full chunks with n_src = rows_per_forward, the
    rows of the short last chunk with n_src = its length, an impression that straddles that boundary cut into two lists -- two
    ``score_lists`` calls at the most, each within ``rows_per_pass`` x H refined rows a pass.  Same score buffer, same
    ``device_scoring``; the scores equal the ungrouped ones to fp32 rounding.  Once per ``DeviceBehaviors`` it is checked, on the device,
    that all rows of an impression carry one history (a split of ``from_devtest`` does): ValueError naming the first impression that
    does not.  CNE has no per-news cache: ``grouped`` is a ValueError there.  Off by default.

    ``news_cache``: the ``build_news_cache`` of this corpus under the model's present weights, where the caller holds one already
    (evaluate_slates_on_device reads its similarity table from it); None: it is built here."""
    config = model.config
    if grouped and model.reads_content_mask:
        raise ValueError('content_encoder \'CNE\' has no per-news content cache: the grouped dev pass (Model.score_lists) cannot serve '
                         'it -- use grouped=False')
    if config.lifetime_type not in ('fixed', 'topic_wise', 'user_topic'):
        raise ValueError('Invalid lifetime_type')
    per = rows_per_forward or config.batch_size
    nodes = getattr(model.user_encoder, 'user_node_embedding', None)       # CROWN's GraphSAGE node slots; ATT / MHSA have no such bound
    slots = behaviors.hist_index.shape[1] + nodes.shape[0] if nodes is not None else per
    if per > slots:
        raise ValueError('rows_per_forward = %d exceeds the H + config.batch_size = %d GraphSAGE node slots (SURVEY Q7): the '
                         'reference raises an index error there' % (per, slots))
    if rows_per_pass < 1:
        raise ValueError('rows_per_pass must be positive')
    num = behaviors.num
    assert num == len(indices), 'one score per (impression, candidate) row'
    was_training = model.training
    model.eval()
    try:
        cache = model.build_news_cache(behaviors.corpus) if news_cache is None else news_cache
        rc = dict(recurrence_cache=model.build_recurrence_cache(behaviors.corpus), rows_per_forward=per) if recurrence_cache else {}
        dev = cache.device
        scores = torch.empty(num, dtype=torch.float32, device=dev)
        full = (num // per) * per                                          # the rows of the full chunks: n_src = per
        step = max(1, (min(rows_per_pass, CNE_CACHED_ROWS_PER_PASS) if recurrence_cache else rows_per_pass) // per) * per
        if grouped:
            _score_grouped(model, behaviors, indices, cache, scores, full, per, rows_per_pass)
        else:
            for r0 in range(0, full, step):
                r1 = min(full, r0 + step)
                scores[r0:r1] = model.score_behaviors(behaviors, torch.arange(r0, r1, device=dev), cache, n_src=per, **rc).float()
            if full < num:                                                 # the last, short chunk: n_src = its length
                scores[full:] = model.score_behaviors(behaviors, torch.arange(full, num, device=dev), cache, n_src=num - full, **rc).float()
    finally:
        model.train(was_training)
    metrics, ranks = device_scoring(scores, indices, labels)
    if result_file is not None:
        write_rank_file(result_file, ranks_to_lists(ranks, indices))
    return (metrics, scores) if return_scores else metrics


# ---- the slates a selection setting makes of the dev split, and what they are worth (csrc/slate_metrics.hip) ----------------------------
SLATE_SETTING_KEYS = ('max_per_topic', 'quota_by', 'mmr_lambda', 'shortlist', 'similarity', 'topic_by', 'calibrate_lambda', 'calibrate_by',
                      'calibrate_alpha')
SLATE_RESULT_KEYS = ('ndcg', 'rr', 'hit', 'recall', 'ild', 'topics', 'filled', 'value')        # per_slate's columns, in order


def check_slate_settings(model, corpus, settings, k, value=None, num=None, calibration=None, H=None):
    """The refusals of ``evaluate_slates_on_device`` over ``settings`` / ``k`` / ``value`` / ``calibration`` (ValueError; nothing is
    launched): a list of dicts over SLATE_SETTING_KEYS, each refused as ``serving.topic_quota`` / ``serving.diversity`` /
    ``serving.calibration`` refuse its arguments (``H``: the history slots of the split, where known); ``topic_by`` 'category'
    (default) or 'topic'; MMR without a ``similarity`` needs a model with a per-news content cache; ``calibration`` None, 'category'
    or 'topic'.  -> per setting (TopicQuota or None, (lam, shortlist) or None, similarity or None, topic_by, Calibration or None)."""
    import numbers

    from . import serving
    from .recommend import CALIBRATE_ALPHA
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 1 <= k <= 128:
        raise ValueError('evaluate_slates_on_device keeps 1 <= k <= 128 news per slate (lime_slate_metrics_f32), got k = %r' % (k,))
    if not isinstance(settings, (list, tuple)) or not all(isinstance(s, dict) for s in settings):
        raise ValueError('settings must be a list of dicts over %s, got %r' % (SLATE_SETTING_KEYS, settings))
    if isinstance(value, str):
        if value not in ('freshness', 'remaining'):
            raise ValueError("value must be 'freshness', 'remaining', a [num] tensor or None, got %r" % (value,))
    elif value is not None and (not isinstance(value, torch.Tensor) or value.dim() != 1 or (num is not None and value.numel() != num)):
        raise ValueError("value must be 'freshness', 'remaining', a tensor with one entry per row%s or None, got %s"
                         % ('' if num is None else ' ([%d])' % num, tuple(value.shape) if isinstance(value, torch.Tensor) else repr(value)))
    if calibration not in (None, 'category', 'topic'):
        raise ValueError("calibration must be None, 'category' or 'topic' (the groups of the miscalibration), got %r" % (calibration,))
    n_news = corpus.news_category.shape[0]
    stub = torch.empty((n_news, 0), dtype=torch.float32, device=corpus.news_category.device)    # (no cache yet: the table comes later)
    histories = None if H is None else stub.new_empty((0, H))                # (the shape is all that is read of them)
    checked = []
    for i, s in enumerate(settings):
        unknown = sorted(set(s) - set(SLATE_SETTING_KEYS))
        if unknown:
            raise ValueError('settings[%d]: unknown key%s %s (the keys are %s)' % (i, 's' if len(unknown) > 1 else '', unknown,
                                                                                  SLATE_SETTING_KEYS))
        topic_by = s.get('topic_by', 'category')
        if topic_by not in ('category', 'topic'):
            raise ValueError("settings[%d]: topic_by must be 'category' or 'topic' (the (category, subCategory) pair), got %r" % (i, topic_by))
        quota = serving.topic_quota(corpus, s.get('max_per_topic'), s.get('quota_by', 'category'))
        cal = serving.calibration(k, s.get('calibrate_lambda'), s.get('calibrate_by', 'category'),
                                  s.get('calibrate_alpha', CALIBRATE_ALPHA), None, s.get('mmr_lambda'), s.get('shortlist'))
        div = serving.diversity(model, stub, k, s.get('mmr_lambda'), s.get('shortlist') if cal is None else None, s.get('similarity'))
        cal = serving.bind_calibration(cal, corpus, histories, stub.device)
        if div is not None and div.table is None and model.reads_content_mask:
            raise ValueError('settings[%d]: %s -- give a similarity table' % (i, model._NO_CONTENT_CACHE))
        checked.append((quota, None if div is None else (div.lam, div.shortlist), s.get('similarity'), topic_by, cal))
    if calibration is not None:                                              # the metric's own limits: the groups and the history slots
        serving.bind_calibration(serving.Calibration(1.0, k, calibration, CALIBRATE_ALPHA, None, None, 0), corpus, histories, stub.device)
    return checked


def sweep_slate_settings(model, behaviors, news_cache, scores, indices, labels, settings, k=10, value=None, per_impression=False,
                         calibration=None):
    """What ``evaluate_slates_on_device`` does behind its scoring pass: ``scores`` fp32 [num] (device), one per row of ``behaviors``;
    an impression (``evaluate.impression_layout`` of ``indices`` / ``labels``) is a list of candidates.  Per setting: the slates
    (``serving.select_segments``), then one ``ops.slate_metrics`` call; at the end ONE device -> host copy of every setting's sums
    and counts.  A calibrated setting selects against the impression's history -- the history of its first row, as the grouped dev
    pass takes it --, and with ``calibration`` one ``ops.slate_miscalibration`` call per setting measures every slate against it.
    -> one dict per setting (see ``evaluate_slates_on_device``)."""
    from . import serving
    from .device_data import topic_table_of
    from .evaluate import impression_layout
    from .recommend import CALIBRATE_ALPHA
    b, dev = behaviors, scores.device
    checked = check_slate_settings(model, b.corpus, settings, k, value, b.num, calibration, _history_slots(b))
    offsets, row_labels, skip = impression_layout(indices, labels)
    if scores.numel() != row_labels.size or b.num != row_labels.size:
        raise ValueError('one score per (impression, candidate) row: %d scores, %d rows, %d labelled rows' % (scores.numel(), b.num, row_labels.size))
    offsets = torch.from_numpy(offsets.astype(np.int64)).to(dev)
    row_labels, skip = torch.from_numpy(row_labels).to(dev), torch.from_numpy(skip).to(dev)
    cand_index = b.cand_index.reshape(-1)
    news = cand_index.to(torch.int32).contiguous()
    if isinstance(value, str):
        fresh = b.cand_freshness.reshape(-1).float()
        value = fresh if value == 'freshness' else model._lifetime_rule(fresh, lambda: b.cand_lifetime.reshape(-1).float(),
                                                                        lambda: b.corpus.news_category[cand_index.long()]).float()
    if value is not None:
        value = value.to(dev).float().contiguous()
    default_table = serving.content_columns(model, news_cache)
    if default_table is not None and default_table.shape[1] % 4:
        default_table = None                                                 # (lime_slate_metrics_f32 reads rows in quads)
    hist_keys = {}

    def history_of(by):
        """hist_keys int32 [n_imp, H] under ``by``: the history of every impression's first row (an impression without a row: no click)."""
        if by not in hist_keys:
            first = offsets[:-1].clamp(max=max(b.num - 1, 0))
            rowless = (offsets[1:] <= offsets[:-1]).unsqueeze(1)
            hist_keys[by] = serving.history_keys(topic_table_of(b.corpus, by)[0], b.hist_index[first], b.hist_mask[first].bool() & ~rowless)
        return hist_keys[by]
    found = []
    for quota, mmr, similarity, topic_by, cal in checked:
        table = similarity if similarity is not None else default_table
        div = None if mmr is None else serving.diversity(model, news_cache, k, mmr[0], mmr[1], similarity)
        positions, _ = serving.select_segments(scores, offsets, None, quota, div, cand_index, k, cal=cal,
                                               hist_keys=None if cal is None else history_of(cal.by))
        topic_of_news, cat_t, _ = topic_table_of(b.corpus, topic_by)
        miscal = None
        if calibration is not None:
            groups, cat_g, _ = topic_table_of(b.corpus, calibration)
            value_m, status_m = ops.slate_miscalibration(positions, k, offsets, news, groups, cat_g.numel(), history_of(calibration),
                                                         None, CALIBRATE_ALPHA)
            counted = (status_m == 0) & (skip == 0)
            miscal = (value_m, status_m, torch.stack([torch.where(counted, value_m, torch.zeros_like(value_m)).sum(), counted.sum().double()]))
        found.append((ops.slate_metrics(positions, k, offsets, news, row_labels, skip, value, table, topic_of_news, n_keys=cat_t.numel()),
                      table is not None, miscal))
    if not found:
        return []
    host = torch.stack([torch.cat([f.sums, f.counts.double()] + ([] if m is None else [m[2]])) for f, _, m in found]).cpu().numpy()
    results = []                                                             # (counts < 2^53: exact)
    for (f, has_table, miscal), row in zip(found, host):
        sums, counts = row[:8], row[8:11].astype(np.int64)
        mean = lambda c, n: float(sums[c] / n) if n else float('nan')
        res = {name: mean(c, counts[0 if c < 4 else 1 if c == 4 else 2]) for c, name in enumerate(SLATE_RESULT_KEYS)}
        if not has_table:
            res['ild'] = float('nan')
        if value is None:
            res['value'] = float('nan')
        res.update(n_relevance=int(counts[0]), n_diversity=int(counts[1]), n_slates=int(counts[2]))
        if miscal is not None:
            res.update(miscalibration=float(row[11] / row[12]) if row[12] else float('nan'), n_calibration=int(row[12]))
        if per_impression:
            res.update(per_impression=f.per_slate, status=f.status)
            if miscal is not None:
                res.update(miscalibration_per_impression=miscal[0], miscalibration_status=miscal[1])
        results.append(res)
    return results


def _history_slots(behaviors):
    """The history slots of a split's rows, or None where it carries no [num, H] history (the refusals' stand-ins)."""
    hist = getattr(behaviors, 'hist_index', None)
    return hist.shape[1] if isinstance(hist, torch.Tensor) and hist.dim() == 2 else None


def evaluate_slates_on_device(model, behaviors, indices, labels, settings, k=10, value=None, rows_per_forward=None,
                              rows_per_pass=DEVICE_EVAL_ROWS_PER_PASS, grouped=False, per_impression=False, result_file=None,
                              recurrence_cache=False, calibration=None):
    """The dev split scored ONCE, and a sweep of selection settings evaluated on those scores without a host round trip: how much
    nDCG@k does a quota or an MMR trade-off cost on the labelled impressions, and how much diversity does it buy?

    ``settings``: a list of dicts, one per setting, over ``max_per_topic`` / ``quota_by`` (Model.recommend's quota), ``mmr_lambda`` /
    ``shortlist`` / ``similarity`` (its MMR), ``calibrate_lambda`` / ``calibrate_by`` / ``calibrate_alpha`` (its calibration, against
    the impression's history: the history of its first row; ``shortlist`` is read with either lambda) and ``topic_by`` ('category',
    the default, or 'topic': the keys behind 'topics'); ``{}`` is the plain top k.  They are refused as ``serving.topic_quota`` /
    ``serving.diversity`` / ``serving.calibration`` refuse them, before any scoring.
    ``calibration``: None, or 'category' / 'topic' -- every setting's dict also holds 'miscalibration', the mean of
    ``ops.slate_miscalibration`` (KL of the impression's history mix against the slate's, at recommend.CALIBRATE_ALPHA) over the
    'n_calibration' slates where it is defined (status 0) and ``skip`` is unset, nan if there are none; with ``per_impression`` also
    'miscalibration_per_impression' fp64 [n_imp] and 'miscalibration_status' int32 [n_imp].
    ``value``: 'freshness', 'remaining' (the remaining lifetime under config.lifetime_type) or a [num] tensor, one number per row;
    None: none.  The other arguments are ``evaluate_cached_on_device``'s, and so are the refusals (``grouped``, the chunk rule, CNE).

    One ``build_news_cache``, one ``evaluate_cached_on_device(..., return_scores=True)``; every impression is then a user's list:
    per setting ``serving.select_segments`` picks its slate of k from the score buffer (the kernels of ``recommend_lists``) and
    lime_slate_metrics_f32 turns the slates into metrics; one device -> host copy of all settings' sums and counts at the end.

    Returns ((AUC, MRR, nDCG@5, nDCG@10) -- exactly ``evaluate_cached_on_device``'s --, a list with one dict per setting): 'ndcg',
    'rr', 'hit', 'recall' -- means over the 'n_relevance' impressions ``scoring`` counts (labelled, both classes) --, 'ild' (1 - mean
    pairwise cosine of the slate's similarity rows: the setting's ``similarity``, else the content columns of the news cache) over
    the 'n_diversity' labelled impressions with >= 2 filled slots, 'topics' (distinct keys), 'filled' and 'value' over the
    'n_slates' with >= 1; nan where nothing was counted or the input is missing.  With ``per_impression`` a dict also holds
    'per_impression' fp64 [n_imp, 8] (the columns in SLATE_RESULT_KEYS' order) and 'status' int32 [n_imp], device tensors."""
    check_slate_settings(model, behaviors.corpus, settings, k, value, behaviors.num, calibration, _history_slots(behaviors))
    was_training = model.training
    model.eval()
    try:
        cache = model.build_news_cache(behaviors.corpus)
    finally:
        model.train(was_training)
    metrics, scores = evaluate_cached_on_device(model, behaviors, indices, labels, result_file=result_file, rows_per_forward=rows_per_forward,
                                                rows_per_pass=rows_per_pass, return_scores=True, recurrence_cache=recurrence_cache,
                                                grouped=grouped, news_cache=cache)
    return metrics, sweep_slate_settings(model, behaviors, cache, scores, indices, labels, settings, k, value, per_impression, calibration)
