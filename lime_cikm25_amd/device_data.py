"""Device-side batch assembly: the reference's Train_Dataset / DevTest_Dataset
(dataset.py:105-141, :192-227) are pure gathers from the corpus tables (corpus.py:360-367) by news index, so the tables
stay resident in HBM and a batch is two launches of ``lime_gather_rows_multi`` (behaviour rows by behaviour index, then the
eight per-news arrays of every candidate and history slot by news index) instead of B x (H + K) host-side numpy gathers,
a collate and a host->device copy per step.  Negative sampling (dataset.py:42-77) is on the host by default, as in the reference:
its result (the sampled candidate tables) is an input of ``DeviceBehaviors.from_train``.  ``DeviceBehaviors.train_resident`` is the
opt-in other way: the train split is uploaded once, with every record's non-clicked news as CSR, and ``resample(seed, epoch)`` refills
the candidate tables in place with one launch of ``lime_negative_sample`` (``counter_negative_sampling`` is its host twin).

The output is the reference's 25-tuple (+ remaining_lifetime, which the caller derives: trainer.py:126-127), with each
candidate tensor laid out directly in front of its history counterpart so that the news encoder's cat is a view.
"""
from itertools import chain

import numpy as np
import torch

from . import ops
from ._lib import NEG_MAX_K

_NEWS_FIELDS = ('news_category', 'news_subCategory', 'news_title_text', 'news_title_mask', 'news_title_entity',
                'news_abstract_text', 'news_abstract_mask', 'news_abstract_entity')


def _pad_history_list(values, H):
    """dataset.py:125-128: the LAST H entries, then zeros up to H."""
    values = list(values)
    return values[-H:] + [0] * max(0, H - len(values))


def negative_sampling(train_behaviors, negative_sample_num, randint=None):
    """Train_Dataset.negative_sampling (dataset.py:42-77) on the host: per train record [positive, negatives ...] news indices,
    the candidate freshness repeated, and [positive lifetime, negative lifetimes ...].  A record with at most
    ``negative_sample_num`` non-clicked news cycles through them; otherwise distinct ones are drawn with ``randint(0, n - 1)``.
    The reference imports ``randint`` from numpy.random (dataset.py:6), whose upper bound is EXCLUSIVE: the last non-clicked
    news of such an impression is never drawn.  That is the default here too (same ``np.random.seed`` -> same samples, pinned
    by tests/golden/dataset_train.npz); pass ``randint=lambda lo, hi: random.randint(lo, hi)`` for the inclusive draw."""
    if randint is None:
        from numpy.random import randint
    samples, freshness, lifetime = [], [], []
    for rec in train_behaviors:
        neg_indices, fresh, neg_lifetimes = rec[4], rec[6], rec[8]
        s, f, l = [rec[3]], [fresh], [rec[7]]
        n = len(neg_indices)
        used = set()
        for j in range(negative_sample_num):
            if n <= negative_sample_num:
                k = j % n
            else:
                while True:
                    k = randint(0, n - 1)
                    if k not in used:
                        used.add(k)
                        break
            s.append(neg_indices[k])
            f.append(fresh)
            l.append(neg_lifetimes[k])
        samples.append(s)
        freshness.append(f)
        lifetime.append(l)
    return samples, freshness, lifetime


_U64 = np.uint64


def _splitmix64(z):
    """The finaliser of csrc/dropout.h (lime_hash4) on a uint64 array."""
    with np.errstate(over='ignore'):
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
        return z ^ (z >> _U64(31))


def counter_negative_draws(counts, negative_sample_num, seed, epoch, inclusive=False):
    """The sampling rule of ``lime_negative_sample`` (csrc/negative_sample.hip) as a pure function, in NumPy integer arithmetic, bit
    for bit: for records ``i`` with ``counts[i]`` non-clicked news the int64 table [len(counts), K] of the indices INTO
    each record's non-clicked list that the K = ``negative_sample_num`` slots take.

      * n <= K: slot j takes j % n (dataset.py:59-63).
      * n >  K: K distinct indices, uniform over [0, m) with m = n - 1 -- the reference's ``randint`` excludes its upper bound, so the
        last non-clicked news is never drawn (dataset.py:64-74) -- or m = n with ``inclusive``.  A partial Fisher-Yates instead of the
        reference's draw-and-reject loop (the same distribution, in exactly K steps): slot j takes the value at position
        r = (u * (m - j)) >> 32 among the m - j values still free and the last free value moves to position r; at most K such moves
        are remembered, a position never moved holds its own number.  The multiply-shift picks each free value with a probability
        within (m - j) / 2^32, relative, of 1 / (m - j): below 2e-8 for a 71-news impression.
      * u of draw j of record i is the upper half of splitmix64(key + 16 i + j), key = seed * 0x9E3779B97F4A7C15 +
        (epoch + 1) * 0xD1B54A32D192ED03 (mod 2^64): the generator and key mixing of csrc/dropout.h with the epoch as the site.  A
        row depends on (seed, epoch, i) and its own n alone -- not on the other records, nor on how many there are.

    Every count must be >= 1 (ValueError otherwise: the reference divides by zero there)."""
    K, seed, epoch = int(negative_sample_num), int(seed), int(epoch)
    if not 1 <= K <= NEG_MAX_K:
        raise ValueError('negative_sample_num must be in [1, %d], got %d' % (NEG_MAX_K, K))
    if not 0 <= epoch < 2 ** 32 - 1 or not 0 <= seed < 2 ** 64:
        raise ValueError('seed must be in [0, 2^64) and epoch in [0, 2^32 - 1), got %d, %d' % (seed, epoch))
    n = np.asarray(counts, dtype=np.int64).reshape(-1)
    if n.size and n.min() < 1:
        raise ValueError('train record %d has no non-clicked news: nothing to sample from' % int(np.argmin(n >= 1)))
    if n.size and n.max() >= 2 ** 31:
        raise ValueError('a record with 2^31 or more non-clicked news')
    out = np.arange(K, dtype=np.int64)[None, :] % n[:, None]
    rec = np.nonzero(n > K)[0]
    if rec.size == 0:
        return out
    key = _U64((seed * 0x9E3779B97F4A7C15 + (epoch + 1) * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF)
    m = (n[rec] - (0 if inclusive else 1)).astype(np.uint64)
    with np.errstate(over='ignore'):
        base = rec.astype(np.uint64) * _U64(NEG_MAX_K) + key
    pos, val = [], []
    for j in range(K):
        c = m - _U64(j)
        with np.errstate(over='ignore'):
            u = _splitmix64(base + _U64(j)) >> _U64(32)
        r = (u * c) >> _U64(32)                                   # u < 2^32, c < 2^31: no overflow
        k, last = r.copy(), c - _U64(1)
        for p, v in zip(pos, val):                                # in order: the latest move of a position wins
            k = np.where(p == r, v, k)
            last = np.where(p == c - _U64(1), v, last)
        pos.append(r)
        val.append(last)
        out[rec, j] = k.astype(np.int64)
    return out


def counter_negative_sampling(train_behaviors, negative_sample_num, seed, epoch, inclusive=False):
    """The host twin of the device sampler (``DeviceBehaviors.resample`` / ``ops.negative_sample``), to that kernel what
    ``evaluate.metrics_from_ranks`` is to ``ops.rank_metrics``: the three lists ``negative_sampling`` returns -- so ``from_train``
    takes them -- with the draws of ``counter_negative_draws(..., seed, epoch, inclusive)`` instead of ``numpy.random``'s stream.
    Where every record has at most ``negative_sample_num`` non-clicked news the two functions return the same lists.  A record
    without non-clicked news is refused with a ValueError that names it."""
    draws = counter_negative_draws([len(rec[4]) for rec in train_behaviors], negative_sample_num, seed, epoch, inclusive).tolist()
    samples, freshness, lifetime = [], [], []
    for rec, ks in zip(train_behaviors, draws):
        neg_indices, fresh, neg_lifetimes = rec[4], rec[6], rec[8]
        samples.append([rec[3]] + [neg_indices[k] for k in ks])
        freshness.append([fresh] * (1 + len(ks)))
        lifetime.append([rec[7]] + [neg_lifetimes[k] for k in ks])
    return samples, freshness, lifetime


def _padded_tail(lists, H, dtype):
    """``_pad_history_list`` of every list into one [len(lists), H] array, in one pass over the flattened values."""
    lens = np.fromiter((len(v) for v in lists), dtype=np.int64, count=len(lists))
    flat = np.fromiter(chain.from_iterable(lists), dtype=dtype, count=int(lens.sum()))
    keep = np.minimum(lens, H)
    out = np.zeros((len(lists), H), dtype=dtype)
    row = np.repeat(np.arange(len(lists)), keep)
    col = np.arange(int(keep.sum())) - np.repeat(np.cumsum(keep) - keep, keep)
    out[row, col] = flat[np.repeat(np.cumsum(lens) - keep, keep) + col]           # the LAST H entries of each list
    return out


def topic_table_of(corpus, by):
    """``recommend.topic_table`` over ``corpus.news_category`` / ``corpus.news_subCategory`` (tensors), as tensors on their device;
    kept on the corpus per ``by`` (the ids are read back to the host once per corpus and ``by``, never per call)."""
    from .recommend import topic_table
    tables = corpus.__dict__.setdefault('_topic_tables', {})
    if by not in tables:
        cat, sub = corpus.news_category, corpus.news_subCategory
        topic, tcat, tsub = topic_table(cat.cpu().numpy(), sub.cpu().numpy(), by)
        tables[by] = (torch.from_numpy(topic).to(cat.device), torch.from_numpy(tcat).to(cat.device).to(cat.dtype),
                      torch.from_numpy(tsub).to(sub.device).to(sub.dtype))
    return tables[by]


class DeviceCorpus:
    """The eight per-news arrays of the reference's Corpus (corpus.py:360-367) on the device."""

    def __init__(self, corpus, device='cuda'):
        self.device = torch.device(device)
        for name in _NEWS_FIELDS:
            arr = np.ascontiguousarray(getattr(corpus, name))
            setattr(self, name, torch.from_numpy(arr).to(self.device))
        self.max_history_num = corpus.max_history_num
        self.category_num = corpus.config.category_num
        self._topic_tables = {}

    def topic_table(self, by):
        """``recommend.topic_table`` of this corpus, on the device: (topic_of_news int32 [n_news], category [T_all], subCategory
        [T_all], the topics' ids in the dtype of ``news_category``).  Computed once per ``by`` and kept."""
        return topic_table_of(self, by)

    def fields(self):
        return [getattr(self, n) for n in _NEWS_FIELDS]


class DeviceBehaviors:
    """One split's behaviour table on the device: per behaviour row the user id, the history (news indices, mask, padded
    freshness / lifetime lists) and the candidates (news indices, freshness, lifetime)."""

    def __init__(self, corpus, user_id, hist_index, hist_mask, user_fr, user_lt, cand_index, cand_fr, cand_lt, eval_shape):
        dev = corpus.device
        self.corpus = corpus
        self.eval_shape = eval_shape
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(dev)
        self.user_id = t(user_id, np.int64).view(-1, 1)
        self.hist_index = t(hist_index, np.int32)
        self.hist_mask = t(hist_mask, bool)
        self.user_freshness = t(user_fr, np.float32)
        self.user_lifetime = t(user_lt, np.float32)
        self.cand_index = t(cand_index, np.int32)
        self.cand_freshness = t(cand_fr, np.float32)
        self.cand_lifetime = t(cand_lt, np.float32)
        self.num = self.user_id.shape[0]
        self._plans, self._turn = {}, {}
        self._neg = None                                                     # train_resident: the CSR of the non-clicked news

    @classmethod
    def from_train(cls, dev_corpus, corpus, train_samples, train_freshness, train_user_topic_lifetime):
        """corpus.train_behaviors (corpus.py:539-552) + the tables negative_sampling filled (dataset.py:42-77)."""
        H = corpus.max_history_num
        beh = corpus.train_behaviors
        return cls(dev_corpus, [b[0] for b in beh], np.stack([np.asarray(b[1]) for b in beh]), np.stack([np.asarray(b[2]) for b in beh]),
                   [_pad_history_list(b[9], H) for b in beh], [_pad_history_list(b[10], H) for b in beh],
                   train_samples, train_freshness, train_user_topic_lifetime, eval_shape=False)

    @classmethod
    def train_resident(cls, dev_corpus, corpus, negative_sample_num):
        """The train split uploaded ONCE for a whole run: the history tables and user ids of ``from_train`` (the same values, built in
        one vectorised pass), the positives, and every record's non-clicked news and their lifetimes as CSR.  The three candidate
        tables [N, 1 + negative_sample_num] are allocated here and filled by ``resample(seed, epoch)``, in place: they, and every other
        table, keep their addresses, so the plans, descriptor tables and workspace rings ``assemble`` builds on its first batch stay
        valid for every later epoch.  A record without non-clicked news (the reference dies with ZeroDivisionError at dataset.py:61)
        is refused here with a ValueError that names it, before anything is uploaded or launched."""
        K = int(negative_sample_num)
        if not 1 <= K <= NEG_MAX_K:
            raise ValueError('negative_sample_num must be in [1, %d], got %d' % (NEG_MAX_K, K))
        H = corpus.max_history_num
        beh = corpus.train_behaviors
        N = len(beh)
        counts = np.fromiter((len(b[4]) for b in beh), dtype=np.int64, count=N)
        if N and counts.min() < 1:
            raise ValueError('train record %d has no non-clicked news: nothing to sample from' % int(np.argmin(counts >= 1)))
        if any(len(b[8]) != len(b[4]) for b in beh):
            raise ValueError('a train record whose non-clicked news and lifetimes differ in length')
        offsets = np.zeros(N + 1, dtype=np.int64)
        np.cumsum(counts, out=offsets[1:])
        nnz = int(offsets[-1])
        if nnz >= 2 ** 31:
            raise ValueError('the train split has 2^31 or more non-clicked news in all')
        empty = np.zeros((N, 1 + K))
        self = cls(dev_corpus, np.fromiter((b[0] for b in beh), dtype=np.int64, count=N),
                   np.stack([b[1] for b in beh]) if N else np.zeros((0, H)), np.stack([b[2] for b in beh]) if N else np.zeros((0, H)),
                   _padded_tail([b[9] for b in beh], H, np.float64), _padded_tail([b[10] for b in beh], H, np.float64),
                   empty, empty, empty, eval_shape=False)
        dev = dev_corpus.device
        up = lambda it, dt, n: torch.from_numpy(np.fromiter(it, dtype=np.float64 if dt == np.float32 else dt, count=n).astype(dt)).to(dev)
        self._neg = {'K': K, 'offsets': torch.from_numpy(offsets).to(dev),
                     'index': up(chain.from_iterable(b[4] for b in beh), np.int32, nnz),
                     'lifetime': up(chain.from_iterable(b[8] for b in beh), np.float32, nnz),
                     'pos_index': up((b[3] for b in beh), np.int32, N), 'pos_lifetime': up((b[7] for b in beh), np.float32, N),
                     'freshness': up((b[6] for b in beh), np.float32, N)}
        self.sampled = None                                                  # (seed, epoch, inclusive) of the tables' content
        return self

    def resample(self, seed, epoch, inclusive=False):
        """Refill the candidate tables of a ``train_resident`` split, in place, with the draws of (seed, epoch): one launch of
        ``lime_negative_sample`` on the current stream, no allocation, no synchronise, no host -> device copy.  The tables equal
        ``from_train(..., *counter_negative_sampling(train_behaviors, K, seed, epoch, inclusive))``'s bit for bit.  A batch assembled
        BEFORE the call keeps its values: ``assemble`` copies rows out of the tables."""
        if self._neg is None:
            raise ValueError('resample needs a split built by DeviceBehaviors.train_resident')
        g = self._neg
        ops.negative_sample(g['offsets'], g['index'], g['lifetime'], g['pos_index'], g['pos_lifetime'], g['freshness'], g['K'], seed, epoch,
                            inclusive, self.cand_index, self.cand_freshness, self.cand_lifetime)
        self.sampled = (int(seed), int(epoch), bool(inclusive))
        return self

    @classmethod
    def from_devtest(cls, dev_corpus, corpus, mode):
        """corpus.dev_behaviors / test_behaviors (corpus.py:590-600): one candidate per row."""
        assert mode in ('dev', 'test')
        H = corpus.max_history_num
        beh = corpus.dev_behaviors if mode == 'dev' else corpus.test_behaviors
        return cls(dev_corpus, [b[0] for b in beh], np.stack([np.asarray(b[1]) for b in beh]), np.stack([np.asarray(b[2]) for b in beh]),
                   [_pad_history_list(b[7], H) for b in beh], [_pad_history_list(b[8], H) for b in beh],
                   np.asarray([b[3] for b in beh]).reshape(-1, 1), np.asarray([b[5] for b in beh]).reshape(-1, 1),
                   np.asarray([b[6] for b in beh]).reshape(-1, 1), eval_shape=True)

    def assemble(self, rows):
        """The collated batch of behaviour rows `rows` (int32 / int64 tensor or sequence): the reference's 25 tensors in
        ``__getitem__`` order, on the device.  Train split: candidates [B, 1 + neg, ...]; dev / test: without the N axis.

        The output tensors come from a ring of two pre-built workspaces per batch size (allocations, views and the two
        descriptor tables are made once): a returned batch stays valid until the call after the next one.
        """
        dev = self.corpus.device
        if self._neg is not None and self.sampled is None:
            raise ValueError('a train_resident split has no candidates before the first resample(seed, epoch)')
        rows = torch.as_tensor(rows, device=dev)
        B = rows.numel()
        if B not in self._plans:
            self._plans[B] = [self._plan(B), self._plan(B)]
        ring = self._plans[B]
        plan = ring[self._turn.get(B, 0)]
        self._turn[B] = 1 - self._turn.get(B, 0)
        plan['rows'].copy_(rows.reshape(-1))                                 # int64 -> int32 on the way if need be
        ops.gather_rows_multi_run(plan['rows'], plan['level1'])
        ops.gather_rows_multi_run(plan['idx_all'], plan['level2'])
        return list(plan['out'])

    def _plan(self, B):
        c = self.corpus
        dev = c.device
        H, N = self.hist_index.shape[1], self.cand_index.shape[1]
        rows = torch.empty(B, dtype=torch.int32, device=dev)
        # level 1: behaviour rows.  The news indices go into ONE vector, candidates first: the order of the level-2 outputs.
        idx_all = torch.empty(B * N + B * H, dtype=torch.int32, device=dev)
        user_id = torch.empty((B, 1), dtype=torch.int64, device=dev)
        hist_mask = torch.empty((B, H), dtype=torch.bool, device=dev)
        ufr, ult = torch.empty((B, H), dtype=torch.float32, device=dev), torch.empty((B, H), dtype=torch.float32, device=dev)
        cfr, clt = torch.empty((B, N), dtype=torch.float32, device=dev), torch.empty((B, N), dtype=torch.float32, device=dev)
        level1 = [(self.cand_index, idx_all[:B * N].view(B, N)), (self.hist_index, idx_all[B * N:].view(B, H)),
                  (self.user_id, user_id), (self.hist_mask, hist_mask), (self.user_freshness, ufr), (self.user_lifetime, ult),
                  (self.cand_freshness, cfr), (self.cand_lifetime, clt)]
        # level 2: the eight per-news arrays for candidates and history in one launch; every output is one buffer whose
        # first B * N rows are the candidates and the rest the history (adjacent -> the encoder's cat is a view)
        outs = [torch.empty((B * N + B * H,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for t in c.fields()]
        news = [o[:B * N].view((B, N) + tuple(o.shape[1:])) for o in outs]
        user = [o[B * N:].view((B, H) + tuple(o.shape[1:])) for o in outs]
        if self.eval_shape:                                                  # DevTest_Dataset: candidate tensors without the N axis
            news = [t.squeeze(1) for t in news]
            cfr, clt = cfr.squeeze(1), clt.squeeze(1)
        out = [user_id.view(B)] + user + [ufr, ult, hist_mask] + self._zeros(B, H) + news + [cfr, clt]
        return {'rows': rows, 'idx_all': idx_all, 'level1': ops.gather_rows_multi_prepare(B, level1),
                'level2': ops.gather_rows_multi_prepare(B * N + B * H, list(zip(c.fields(), outs))), 'out': out}

    def _zeros(self, B, H):
        """dataset.py:119-121: the SUE-only tensors are zeros for every other user encoder."""
        dev = self.corpus.device
        return [torch.zeros((B, H, H), dtype=torch.float32, device=dev),
                torch.zeros((B, self.corpus.category_num + 1), dtype=torch.bool, device=dev),
                torch.zeros((B, H), dtype=torch.int64, device=dev)]
