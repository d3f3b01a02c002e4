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
                              rows_per_pass=DEVICE_EVAL_ROWS_PER_PASS, return_scores=False, recurrence_cache=False, grouped=False):
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
    does not.  CNE has no per-news cache: ``grouped`` is a ValueError there.  Off by default."""
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
        cache = model.build_news_cache(behaviors.corpus)
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
