"""MIND-style ranking metrics from rank files: a restatement of the reference's evaluate.py:7-89 (SURVEY.md section 8f
row 1).  Host-side logic (numpy); the scores it consumes come from the HIP path.  ``metrics_from_ranks`` states the same metrics as
closed forms of the ranks, and ``device_scoring`` evaluates those on the device from device-resident scores (csrc/rank_metrics.hip).

Pinned by tests/golden/eval_*.json, produced by running the reference's own ``util.compute_scores`` and
``evaluate.scoring`` (tools/make_eval_goldens.py).  AUC is computed the way sklearn's ``roc_auc_score`` does for a
binary target (ROC curve at the distinct score thresholds, trapezoidal area), without importing sklearn.
"""
import json

import numpy as np


def _by_score(y_true, y_score, k=None):
    """Labels reordered by descending score (numpy's default sort reversed, as the reference does: evaluate.py:8, :22)."""
    ranked = np.take(y_true, np.argsort(y_score)[::-1][:k])
    return ranked, np.arange(ranked.shape[0])


def dcg_score(y_true, y_score, k=10):
    """sum_i (2^rel_i - 1) / log2(i + 2) over the k best-scored items (evaluate.py:7-12)."""
    rel, pos = _by_score(y_true, y_score, k)
    return np.sum((2 ** rel - 1) / np.log2(pos + 2))


def ndcg_score(y_true, y_score, k=10):
    """DCG normalised by the DCG of the ideal order (evaluate.py:15-18)."""
    ideal = dcg_score(y_true, y_true, k)
    return dcg_score(y_true, y_score, k) / ideal


def mrr_score(y_true, y_score):
    """Sum of label / rank over the label mass (evaluate.py:21-25)."""
    rel, pos = _by_score(y_true, y_score)
    return np.sum(rel / (pos + 1)) / np.sum(y_true)


def roc_auc_score(y_true, y_score):
    """Binary ROC AUC as sklearn computes it (evaluate.py:77): thresholds at the distinct scores, trapezoidal rule."""
    y_true = np.asarray(y_true, dtype=np.float64)
    y_score = np.asarray(y_score, dtype=np.float64)
    if np.unique(y_true).size != 2:
        raise ValueError('Only one class present in y_true. ROC AUC score is not defined in that case.')
    pos = y_true == y_true.max()
    order = np.argsort(y_score, kind='mergesort')[::-1]
    y_score, pos = y_score[order], pos[order]
    distinct = np.where(np.diff(y_score))[0]
    idx = np.r_[distinct, pos.size - 1]
    tps = np.cumsum(pos)[idx].astype(np.float64)
    fps = (1 + idx - tps).astype(np.float64)
    tps, fps = np.r_[0.0, tps], np.r_[0.0, fps]
    tpr, fpr = tps / tps[-1], fps / fps[-1]
    return float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) * 0.5))          # trapezoidal rule


def parse_line(line):
    """'<impression id> [v1,v2,...]' -> (id, list)  (evaluate.py:27-30)."""
    impid, payload = line.strip('\n').split()
    return impid, json.loads(payload)


def _rank_scores(ranks, n_labels, line_no):
    """A rank file stores 1-based ranks; the metrics consume 1 / rank (evaluate.py:60-66)."""
    out = []
    for r in ranks:
        v = 1. / r
        if not 0 <= v <= 1:
            raise ValueError('Line-{}: score_rslt should be int from 0 to {}'.format(line_no, float(n_labels)))
        out.append(v)
    return out


def scoring(truth_f, sub_f):
    """(AUC, MRR, nDCG@5, nDCG@10) averaged over the impressions of a truth file and a rank file read in lock step
    (evaluate.py:32-89): impressions with an empty label list are skipped, a missing submission line counts as all-ones."""
    per_impression = []
    line_no = 1
    for truth_line in truth_f:
        sub_line = sub_f.readline()
        impid, labels = parse_line(truth_line)
        if not labels:                          # masked impression (the submission line is consumed all the same)
            continue
        if sub_line == '':
            sub_id, ranks = impid, [1] * len(labels)
        else:
            try:
                sub_id, ranks = parse_line(sub_line)
            except Exception:
                raise ValueError('line-{}: Invalid Input Format!'.format(line_no))
        if sub_id != impid:
            raise ValueError('line-{}: Inconsistent Impression Id {} and {}'.format(line_no, sub_id, impid))
        y_true = np.array(labels, dtype='float32')
        y_score = _rank_scores(ranks, len(labels), line_no)
        per_impression.append((roc_auc_score(y_true, y_score), mrr_score(y_true, y_score), ndcg_score(y_true, y_score, 5),
                               ndcg_score(y_true, y_score, 10)))
        line_no += 1
    cols = list(zip(*per_impression)) if per_impression else [[], [], [], []]
    return tuple(np.mean(c) for c in cols)


# ---- the same metrics as closed forms of the ranks (the host twin of csrc/rank_metrics.hip) ----------------------------------------
ONE_CLASS = 'Only one class present in y_true. ROC AUC score is not defined in that case.'


def metrics_from_ranks(ranks, labels, per_impression=False):
    """What ``scoring`` computes, as closed forms of the ranks, vectorised over a whole split.  ``scoring`` feeds 1 / rank into every
    metric, so with P positives among the n rows of an impression (N = n - P), q the rank of a positive and ahead_pos the number of
    positives ranked ahead of it:

        AUC    = sum_pos (N - (q - 1 - ahead_pos)) / (P N)      the (positive, negative) pairs in the right order: ranks are distinct
        MRR    = (sum_pos 1 / q) / P
        nDCG@k = (sum_pos, q <= k  1 / log2(q + 1)) / (sum_{p < min(k, P)} 1 / log2(p + 2))         k = 5, 10

    ``ranks``: per impression the 1-based ranks in candidate order (util.rank_impressions); ``labels``: per impression the 0 / 1 labels
    (formats.truth_labels).  An impression with an empty label list is left out, as ``scoring`` leaves it out (its rank line is consumed).
    Returns (AUC, MRR, nDCG@5, nDCG@10) averaged over the counted impressions and raises the ValueError of ``roc_auc_score`` for an
    impression with one class only; with ``per_impression`` it returns (per_imp fp64 [n_imp, 4], status int32 [n_imp]) instead and
    raises nothing for the data: status 0 counted, 1 left out, 2 one class only, 3 a label outside {0, 1}."""
    n_imp = len(labels)
    if len(ranks) < n_imp:
        raise ValueError('%d rank lists for %d label lists' % (len(ranks), n_imp))
    lens = np.fromiter((len(l) for l in labels), dtype=np.int64, count=n_imp)
    for i in np.flatnonzero(lens):
        if len(ranks[i]) != lens[i]:
            raise ValueError('impression %d: %d ranks for %d labels' % (i + 1, len(ranks[i]), lens[i]))
    q = np.fromiter((r for i in range(n_imp) if lens[i] for r in ranks[i]), dtype=np.int64, count=int(lens.sum()))
    y = np.fromiter((v for l in labels for v in l), dtype=np.int64, count=int(lens.sum()))
    seg = np.repeat(np.arange(n_imp), lens)
    bad = np.bincount(seg[(y != 0) & (y != 1)], minlength=n_imp) > 0
    pos = y != 0
    P = np.bincount(seg[pos], minlength=n_imp)
    N = lens - P
    status = np.where(lens == 0, 1, np.where(bad, 3, np.where((P == 0) | (N == 0), 2, 0))).astype(np.int32)
    # the positives in (impression, rank) order: a positive's place inside its impression's block is ahead_pos
    sp, qp = seg[pos], q[pos]
    order = np.lexsort((qp, sp))
    sp, qp = sp[order], qp[order]
    first = np.cumsum(P) - P
    ahead_pos = np.arange(sp.size) - first[sp]
    disc = 1.0 / np.log2(np.arange(10) + 2.0)
    gain = np.where(qp <= 10, disc[np.minimum(qp, 10) - 1], 0.0)
    neg_ahead = np.bincount(sp, weights=(qp - 1 - ahead_pos).astype(np.float64), minlength=n_imp)
    ideal = np.concatenate(([0.0], np.cumsum(disc)))
    per = np.zeros((n_imp, 4), dtype=np.float64)
    ok = status == 0
    Pf, Nf = P[ok].astype(np.float64), N[ok].astype(np.float64)
    per[ok, 0] = (Pf * Nf - neg_ahead[ok]) / (Pf * Nf)
    per[ok, 1] = np.bincount(sp, weights=1.0 / qp, minlength=n_imp)[ok] / Pf
    per[ok, 2] = np.bincount(sp, weights=np.where(qp <= 5, gain, 0.0), minlength=n_imp)[ok] / ideal[np.minimum(P[ok], 5)]
    per[ok, 3] = np.bincount(sp, weights=gain, minlength=n_imp)[ok] / ideal[np.minimum(P[ok], 10)]
    if per_impression:
        return per, status
    if (status >= 2).any():
        i = int(np.flatnonzero(status >= 2)[0])
        raise ValueError(ONE_CLASS if status[i] == 2 else 'impression %d: labels must be 0 or 1' % (i + 1))
    return tuple(np.mean(per[ok, m]) for m in range(4)) if ok.any() else (np.mean([]),) * 4


def impression_layout(indices, labels):
    """(offsets int32 [n_imp + 1], row labels uint8 [R], skip uint8 [n_imp]) of ``ops.rank_metrics`` from the impression of every row
    (``indices``: 0-based, non-decreasing -- corpus.dev_indices) and the per-impression label lists (formats.truth_labels /
    corpus.dev_labels; an empty list marks an impression that ``scoring`` leaves out).  n_imp = len(labels).  Raises ValueError for a
    decreasing ``indices``, an impression id outside the labels, and a labelled impression whose row count is not its label count."""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    n_imp = len(labels)
    if idx.size and (np.diff(idx) < 0).any():
        raise ValueError('indices must be non-decreasing (the rows of an impression are contiguous): first decrease at row %d'
                         % (int(np.argmax(np.diff(idx) < 0)) + 1))
    if idx.size and (idx[0] < 0 or idx[-1] >= n_imp):
        raise ValueError('indices name impressions %d .. %d, the labels hold %d impressions' % (idx[0], idx[-1], n_imp))
    offsets = np.searchsorted(idx, np.arange(n_imp + 1), side='left').astype(np.int32)
    counts = np.diff(offsets)
    lens = np.fromiter((len(l) for l in labels), dtype=np.int64, count=n_imp)
    wrong = np.flatnonzero((lens > 0) & (lens != counts))
    if wrong.size:
        raise ValueError('impression %d has %d rows and %d labels' % (wrong[0] + 1, counts[wrong[0]], lens[wrong[0]]))
    flat = np.fromiter((v for l in labels for v in l), dtype=np.int64, count=int(lens.sum()))
    if flat.size and (flat.min() < 0 or flat.max() > 255):
        raise ValueError('labels must be 0 or 1')
    row_labels = np.zeros(idx.size, dtype=np.uint8)
    row_labels[np.repeat(lens > 0, counts)] = flat.astype(np.uint8)
    return offsets, row_labels, (lens == 0).astype(np.uint8)


def device_scoring(scores, indices, labels):
    """``scoring`` without the files and without the host: ranks and metrics of a whole split from the device-resident scores
    (fp32 CUDA tensor, one per row) in one ``ops.rank_metrics`` call.  ``indices`` / ``labels`` as in ``impression_layout``.
    Returns ((AUC, MRR, nDCG@5, nDCG@10) as Python floats, ranks int32 CUDA tensor [R]).  Raises ValueError where ``scoring`` does -- an
    impression with one class only (``roc_auc_score``'s error, naming the first such impression) -- and for a NaN score or a label
    outside {0, 1}.  One device -> host copy (status, sums, count) at the end."""
    import torch

    from . import ops
    if not isinstance(scores, torch.Tensor) or not scores.is_cuda:
        raise TypeError('scores must be a CUDA tensor (the HIP path has no CPU fallback)')
    offsets, row_labels, skip = impression_layout(indices, labels)
    if scores.numel() != row_labels.size:
        raise ValueError('one score per (impression, candidate) row: %d scores, %d rows' % (scores.numel(), row_labels.size))
    dev = scores.device
    res = ops.rank_metrics(scores.reshape(-1), torch.from_numpy(row_labels).to(dev), offsets, torch.from_numpy(skip).to(dev))
    status = res.status.cpu().numpy()
    if (status == 3).any():
        raise ValueError('impression %d: a NaN score or a label outside {0, 1}' % (int(np.flatnonzero(status == 3)[0]) + 1))
    if (status == 2).any():
        raise ValueError('impression %d: %s' % (int(np.flatnonzero(status == 2)[0]) + 1, ONE_CLASS))
    return res.means(), res.ranks
