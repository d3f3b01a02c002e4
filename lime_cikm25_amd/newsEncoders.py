"""Drop-in news encoders of the scoring path: FreshnessEncoder, LIME, CROWN, CNN, NAML, MHSA, CNE and KCNN
(reference newsEncoders.py:38-161, 167-373, 439-532, 535-563, 566-595, 598-638, 641-695, 806-828).

The modules keep the reference's attribute and parameter names, so ``state_dict()`` has the same
183 keys and reference checkpoints load.  Standard torch containers
(nn.Linear, nn.Embedding, nn.TransformerEncoder ...) are used as *parameter holders* with their
constructor-default initialisation, exactly as the reference leaves them; their ``forward`` is never
called.  All arithmetic runs in hand-written HIP kernels (lime_cikm25_amd.ops -> liblime_hip.so):

  word gather + positional table      fused into the A-operand fetch of the in_proj GEMM
  in_proj / out_proj / FFN            exact-fp32 MFMA GEMM; bias, ReLU, residual and LayerNorm in the epilogue
  token attention                     one wave per 32 query rows, scores held in MFMA accumulators
  mean pool / intent tail / buckets   small fixed-order kernels
"""
import collections
import math
import os
import types

import torch
import torch.nn as nn
from torch.nn import TransformerEncoder, TransformerEncoderLayer

from . import kept, ops
from .layers import Attention, Conv1D, Conv2D_Pool, LinearHolder, LSTMHolder, MultiHeadAttention, ScaledDotProduct_CandidateAttention

# tokens encoded per pass of the token encoder: bounds the activation workspace (9.2 KB / token)
MAX_TOKENS_PER_PASS = 4 * 1024 * 1024

# Encode only what differs (encode_tokens_compact): all-padding sequences share one representative, in_proj runs over the live
# tokens only.  Exact (same arithmetic per row, nothing cached between forwards); LIME_DENSE_TOKENS=1 (or DEDUP = False) runs
# every token of every slot through the layer as the reference does -- the A/B switch behind bench.py's "dense" figures.
DEDUP = os.environ.get('LIME_DENSE_TOKENS', '0') != '1'
# Behind the token encoders, run the row-wise tail (intent layers, intent attention, fuse, LIME.project) once per DISTINCT news: the
# repetitions of the padding news collapse onto one representative (csrc/compact.hip, lime_compact_batch) and the result is expanded
# through news_inv.  Exact (same kernels, same arithmetic per row); needs DEDUP, covers the one-pass fp32 compacted path of CROWN
# under LIME's concat + project.  LIME_NEWS_DEDUP=0 (or NEWS_DEDUP = False): every slot through the tail, as before (A/B runs).
NEWS_DEDUP = os.environ.get('LIME_NEWS_DEDUP', '1') != '0'


def _no_train_dropout(module, p):
    if module.training and p > 0:
        raise NotImplementedError('encode_flat() is the fused scoring kernel chain (eval-mode children, or dropout_rate = 0): with '
                                  'training-mode dropout active call the module (forward) or Model.forward, which take the '
                                  'differentiable path of lime_cikm25_amd.training')


def _flat_inputs(title_text, title_mask, content_text, category, subCategory):
    B, n = title_text.shape[0], title_text.shape[1]
    return (_i32(title_text).reshape(B * n, -1).contiguous(), title_mask.reshape(B * n, -1).contiguous(),
            _i32(content_text).reshape(B * n, -1).contiguous(), _i32(category).reshape(-1).contiguous(),
            _i32(subCategory).reshape(-1).contiguous())


_SIDE = {}


# Independent branches of the forward CAN be forked onto side streams (fork / join with wait_stream, which is also how
# the fork is recorded into the HIP graph): branch 0 = freshness encoder, 2 = candidate-aware attention weights (small,
# latency-bound kernels that otherwise sit on the critical path in front of the token encoders), 1 = title chain beside the
# body chain, 3 = the body encoder's preparation under the title encoder, 4 = category representation + stacked intent weights, 5 = the
# body half of the intent attention's hidden GEMM, 6 = the candidate side of the interest match (same-box A/B at config 2b, ms per
# step: {0,2} 2.414, {0,2,3} 2.372, {0,2,4} 2.446 -- short kernels in front of a persistent GEMM delay some of its statically
# scheduled workgroups --, {0,2,5,6} 2.415, all 2.466), 7 = on the compacted path, the title encoder's chain beside the body
# encoder's: the compacted launches have few tiles (423 / 251 / 502 on 512 workgroup slots for the title, a half-empty last round
# for the body), so the two chains fill each other's gaps ({0,2,3} 2.288, {0,2,3,7} 2.210; on the dense path, whose launches fill
# every slot for ten rounds, the same fork -- branch 1 -- measured slower; beside the forked title chain branch 4 now pays:
# {0,2,3,7} 2.242, {0,2,3,4,7} 2.206; three interleaved 300-step runs each: {0,2,3,4,7} 2.195, + 5 2.175, + 6 2.170, + {5,6} 2.155).  OVERLAP_BRANCHES is the set that is forked (LIME_OVERLAP_STREAMS = 0: none, 2: the two small branches --
# the default, 4.557 vs 4.593 ms --, 1: all three).  The title / body fork is off by default: the big GEMMs hold two
# workgroups of 256 VGPRs x 4 waves and 61 KB LDS on every CU, so nothing else becomes resident beside them and that fork
# measured slower (4.651 ms).
def _branches(spec):
    named = {'0': frozenset(), '1': frozenset((0, 1, 2, 3, 4, 5, 6, 7)), '2': frozenset((0, 2, 3, 4, 5, 6, 7))}
    return named[spec] if spec in named else frozenset(int(x) for x in spec.split('+'))       # e.g. LIME_OVERLAP_STREAMS=0+2+4


OVERLAP_BRANCHES = _branches(os.environ.get('LIME_OVERLAP_STREAMS', '2'))
SERIAL_STREAMS = False          # bench.py's instrumented pass forces everything onto one stream


def _side_stream(device, which=0):
    if SERIAL_STREAMS or which not in OVERLAP_BRANCHES:
        return torch.cuda.current_stream(device)
    key = (device.type, device.index, which)
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=device)
    return _SIDE[key]


_ZERO_IDS = {}


def _grown(cache, n, device, floor, make):
    """The first n entries of a per-device constant (``make(size)``: all zeros, or an arange -- a prefix of either is right for every
    n) that is allocated once and never written.  A captured HIP graph holds the ADDRESS of the tensor it was recorded with, so a
    tensor once handed out is never released: when a caller needs more entries a new generation of at least twice the size is added
    and the older ones stay alive in ``cache`` (at most as much memory again as the newest one), where a replay still finds them."""
    gens = cache.setdefault((device.type, device.index), [])
    if not gens or gens[-1].numel() < n:
        gens.append(make(max(n, floor, 2 * gens[-1].numel() if gens else 0)))
    return gens[-1][:n]


def _zero_ids(n, device):
    """n zero word ids (the padding word), allocated once per device and never written: a forward does not pay a fill launch for them."""
    return _grown(_ZERO_IDS, n, device, 512, lambda size: torch.zeros(size, dtype=torch.int32, device=device))


def _cat_rows(ts):
    """torch.cat(ts, dim=0) -- as a VIEW when the pieces already sit back to back in one storage (the Model's packed
    graph inputs are laid out that way), so the per-forward concatenation of candidates and history costs no kernel."""
    t0 = ts[0]
    ok = all(t.is_contiguous() and t.dtype == t0.dtype and t.shape[1:] == t0.shape[1:] and
             t.untyped_storage().data_ptr() == t0.untyped_storage().data_ptr() for t in ts)
    if ok:
        end = t0.storage_offset()
        for t in ts:
            ok = ok and t.storage_offset() == end
            end += t.numel()
    if not ok:
        return torch.cat(ts, dim=0)
    rows = sum(t.shape[0] for t in ts)
    size = (rows,) + tuple(t0.shape[1:])
    stride = t0.stride() if t0.dim() > 1 else (1,)
    return t0.as_strided(size, stride, t0.storage_offset())


def _i32(t):
    return t if t.dtype == torch.int32 else t.to(torch.int32)


def reference_bucket(x, num_buckets):
    """The reference's bucket rule (newsEncoders.py:53-58) as torch evaluates it in fp32 on the CPU."""
    x = torch.clamp(x.float(), min=1)
    scaled = torch.log(x) / torch.log(torch.tensor(60 * 60 * 24.0))
    return torch.clamp((scaled * (num_buckets / 7)).long(), max=num_buckets - 1)


def bucket_cut_points(num_buckets):
    """The num_buckets - 1 fp32 cut points of the bucket rule: the smallest float whose bucket is >= k, for k = 1 .. num_buckets - 1,
    found by bisection over the bit patterns of the positive floats with the rule's own fp32 evaluation on the CPU (the rule is
    monotone; a +-64-ulp window around every cut is re-checked).  Comparing against them reproduces the rule bit-exactly on the
    device without depending on any logf (for num_buckets = 10 this is the table built into lime_bucketize_f32)."""
    import numpy as np
    top = int(np.array([np.finfo(np.float32).max], dtype=np.float32).view(np.uint32)[0])
    one = int(np.array([1.0], dtype=np.float32).view(np.uint32)[0])
    f = lambda bits: reference_bucket(torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy()), num_buckets)
    cuts = []
    for k in range(1, num_buckets):
        lo, hi = one, top                                   # bucket(lo) = 0 < k <= bucket(hi)
        if int(f([hi])[0]) < k:
            raise ValueError('bucket %d is never reached with num_buckets = %d' % (k, num_buckets))
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if int(f([mid])[0]) >= k:
                hi = mid
            else:
                lo = mid
        win = list(range(max(one, hi - 64), min(top, hi + 64) + 1))
        b = f(win)
        if not bool(((b >= k) == (torch.tensor(win) >= hi)).all()):
            raise ValueError('the bucket rule is not monotone around its cut point %d (num_buckets = %d)' % (k, num_buckets))
        cuts.append(hi)
    return torch.from_numpy(np.array(cuts, dtype=np.uint32).view(np.float32).copy())


class FreshnessEncoder(nn.Module):
    """newsEncoders.py:38-83.  hidden = content dim always: ``fusion_method == 'add' or 'gated'`` is truthy (:42-45)."""

    def __init__(self, config, base_news_encoder):
        super().__init__()
        embedding_dim = config.freshness_embedding_dim
        hidden_dim = base_news_encoder.news_embedding_dim
        self.num_buckets = config.num_buckets
        # num_buckets = 10 (config.py:59): the cut points are built into lime_bucketize_f32; any other count: derived here from the
        # rule's own fp32 evaluation (a plain attribute, not a buffer: the state_dict keeps the reference's keys)
        self._cuts = None if self.num_buckets == 10 else bucket_cut_points(self.num_buckets)
        self.freshness_embedding = nn.Embedding(self.num_buckets, embedding_dim)
        self.lifetime_embedding = nn.Embedding(self.num_buckets, embedding_dim)
        self.dense = nn.Linear(embedding_dim * 2, hidden_dim)
        self.activation = nn.Tanh()

    def bucketize(self, x):
        """int64 like the reference (newsEncoders.py:53-58); computed by threshold comparison on the device."""
        return self.buckets(x.float()).long()

    def cuts_on(self, device):
        """The cut-point table on ``device`` (None for num_buckets = 10: the table built into the kernels)."""
        if self._cuts is not None and self._cuts.device != device:
            self._cuts = self._cuts.to(device)
        return self._cuts

    def buckets(self, x):
        """int32 buckets of a flat fp32 tensor."""
        return ops.bucketize(x, self.cuts_on(x.device))

    def encode_flat(self, freshness, lifetime, out):
        """freshness / lifetime: [M] fp32; out: [M, hidden] (may be a view of a wider buffer)."""
        M = freshness.numel()
        E = self.freshness_embedding.embedding_dim
        fb = self.buckets(freshness)
        lb = self.buckets(lifetime)
        cat = torch.empty((M, 2 * E), dtype=torch.float32, device=out.device)
        ops.gather_rows(fb, self.freshness_embedding.weight, cat[:, :E])
        ops.gather_rows(lb, self.lifetime_embedding.weight, cat[:, E:])
        return ops.linear(cat, self.dense.weight, self.dense.bias, act='tanh', out=out)

    def forward(self, news_freshness, news_user_topic_lifetime):
        if news_freshness.dim() == 1:
            news_freshness = news_freshness.unsqueeze(1)
        if news_user_topic_lifetime.dim() == 1:
            news_user_topic_lifetime = news_user_topic_lifetime.unsqueeze(1)
        if news_freshness.shape != news_user_topic_lifetime.shape:
            news_user_topic_lifetime = news_user_topic_lifetime.expand_as(news_freshness)
        B, n = news_freshness.shape
        out = torch.empty((B * n, self.dense.out_features), dtype=torch.float32, device=news_freshness.device)
        self.encode_flat(news_freshness.float().contiguous().view(-1), news_user_topic_lifetime.float().contiguous().view(-1), out)
        return out.view(B, n, -1)


class LIME(nn.Module):
    """newsEncoders.py:87-161: content + freshness, fused by 'concat' + project (the default, 400 columns), 'add' or 'gated' (the
    content encoder's 900 columns)."""

    def __init__(self, config, base_news_encoder):
        super().__init__()
        self.final_dim = config.lime_output_dim
        self.category_embedding = nn.Embedding(config.category_num, config.category_embedding_dim)
        self.category_embedding.weight.requires_grad = False
        self.subCategory_embedding = nn.Embedding(config.subCategory_num, config.subCategory_embedding_dim)
        self.subCategory_embedding.weight.requires_grad = False
        self.category_affine = nn.Linear(config.category_embedding_dim + config.subCategory_embedding_dim,
                                         config.category_embedding_dim)
        self.base_news_encoder = base_news_encoder
        self.freshness_encoder = FreshnessEncoder(config, base_news_encoder)
        self.fusion_method = config.fusion_method       # 'concat' (default), 'add' or 'gated' (newsEncoders.py:99, :111-126)
        self.auxiliary_loss = getattr(base_news_encoder, 'auxiliary_loss', None)      # newsEncoders.py:100-103
        content_dim = self.base_news_encoder.news_embedding_dim
        freshness_dim = content_dim                                                   # newsEncoders.py:106-107
        if self.fusion_method == 'concat':
            self.output_dim = content_dim + freshness_dim
            if self.final_dim:
                self.project = nn.Linear(self.output_dim, self.final_dim)
                self.output_dim = self.final_dim
            else:
                self.project = nn.Identity()
        elif self.fusion_method == 'add':
            self.output_dim = content_dim
            self.project = nn.Identity()
        elif self.fusion_method == 'gated':
            self.gate = nn.Linear(content_dim + freshness_dim, content_dim)
            self.output_dim = content_dim
            self.project = nn.Identity()
        else:
            raise ValueError('Unknown fusion method: %s' % self.fusion_method)
        self.news_embedding_dim = self.output_dim

    def initialize(self):
        if hasattr(self.base_news_encoder, 'initialize'):
            self.base_news_encoder.initialize()
        nn.init.xavier_uniform_(self.freshness_encoder.dense.weight)
        nn.init.zeros_(self.freshness_encoder.dense.bias)
        nn.init.uniform_(self.category_embedding.weight, -0.1, 0.1)
        nn.init.uniform_(self.subCategory_embedding.weight, -0.1, 0.1)
        nn.init.xavier_uniform_(self.category_affine.weight)
        nn.init.zeros_(self.category_affine.bias)

    def _base_encode(self, title_text, title_mask, content_text, category, subCategory, out, content_mask, pair_groups=None,
                     title_entity=None, recurrence=None):
        """The content encoder's encode_flat; the body mask (and the reference calls' news counts) go to the encoder that reads them
        (CNE) and to no other, the title's entity ids to KCNN.  ``recurrence`` = (CNERecurrenceCache, news_index): CNE reads its
        recurrence from the cache instead of the texts (encode_cached_flat)."""
        enc = self.base_news_encoder
        if recurrence is not None:
            return enc.encode_cached_flat(recurrence[0], recurrence[1], title_mask, content_mask, category, subCategory, out, pair_groups)
        if getattr(enc, 'reads_title_entity', False):
            return enc.encode_flat(title_text, title_mask, content_text, category, subCategory, out, title_entity=title_entity)
        if getattr(enc, 'reads_content_mask', False):
            return enc.encode_flat(title_text, title_mask, content_text, category, subCategory, out, content_mask, pair_groups)
        return enc.encode_flat(title_text, title_mask, content_text, category, subCategory, out)

    def encode_flat(self, title_text, title_mask, content_text, category, subCategory, freshness, lifetime, content_mask=None,
                    pair_groups=None, title_entity=None, recurrence=None):
        """Flat batch of M news -> [M, output_dim].  title_text [M, T], content_text [M, L] int32; the rest [M].  content_mask [M, L]:
        the body mask, read by the CNE content encoder alone.  title_entity [M, T] int32: the title's entity ids, read by KCNN alone.
        ``recurrence`` = (CNERecurrenceCache, news_index int32 [M]), CNE alone: the M news are news of the cache, their recurrence is read
        from it and the texts are not (title_text / content_text may be None)."""
        M = category.shape[0]
        dev = category.device
        cdim = self.base_news_encoder.news_embedding_dim
        main = torch.cuda.current_stream()
        side = _side_stream(dev)
        if self.fusion_method in ('add', 'gated'):                                   # newsEncoders.py:154-159
            fused = torch.empty((M, 2 * cdim), dtype=torch.float32, device=dev)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                self.freshness_encoder.encode_flat(freshness, lifetime, fused[:, cdim:])
            self._base_encode(title_text, title_mask, content_text, category, subCategory, fused[:, :cdim], content_mask, pair_groups,
                              title_entity, recurrence)
            main.wait_stream(side)
            gate = ops.linear(fused, self.gate.weight, self.gate.bias, act='sigmoid') if self.fusion_method == 'gated' else None
            return ops.fuse_rows(fused[:, :cdim], fused[:, cdim:], gate)
        if isinstance(self.project, nn.Identity):
            fused = torch.empty((M, 2 * cdim), dtype=torch.float32, device=dev)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                self.freshness_encoder.encode_flat(freshness, lifetime, fused[:, cdim:])
            self._base_encode(title_text, title_mask, content_text, category, subCategory, fused[:, :cdim], content_mask, pair_groups,
                              title_entity, recurrence)
            main.wait_stream(side)
            return fused
        # project(cat(content, fresh)) = content W_c^T + (fresh W_f^T + b), and fresh = tanh(dense(cat(E_f[b1], E_l[b2]))) takes one of
        # num_buckets^2 values: the freshness half of `project` is a [100, 400] table G per forward (three GEMMs on 10 / 100-row
        # operands instead of one on M rows), gathered into the content GEMM as a residual by the bucket pair (newsEncoders.py:60-83,
        # :151-153; same sums, associated per half).  The branch depends on the inputs' buckets and the weights only: side stream.
        fe = self.freshness_encoder
        nb = fe.num_buckets
        enc = self.base_news_encoder
        if (NEWS_DEDUP and recurrence is None and title_text is not None and hasattr(enc, 'news_dedup_applicable') and
                enc.news_dedup_applicable(title_text, content_text)):
            # the tail once per distinct news: the compaction (three launches on branch 3, in front of the encoders' preparation) also
            # lists the news; the bucket pair and the topic rows are taken from the compact keys (one launch on the content encoder's
            # branch 4, which leaves the pair in nw.pair: int32 [M + 1], unused slots valid), `project` runs over n_news rows and the
            # result is expanded to the M slots -- the one launch this adds to the critical path.  The table is the kept one, or
            # computed here on the side stream (occurrence_tables)
            side3 = _side_stream(dev, 3)
            side3.wait_stream(main)
            with torch.cuda.stream(side3):
                news = ops.compact_batch(title_text, content_text, category, subCategory, freshness.contiguous(), lifetime.contiguous(),
                                         count_mult=enc.intent_num)
            nw = news[2]
            table = self._kept_tables()
            forked = table is None
            if forked:
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    table = self._compute_occurrence_tables()
            content = torch.empty((M + 1, cdim), dtype=torch.float32, device=dev)
            enc.encode_flat(title_text, title_mask, content_text, category, subCategory, content, news=news,
                            buckets=(nb, fe.cuts_on(dev)))
            if forked:
                main.wait_stream(side)
            rep_c = ops.linear(content, self.project.weight[:, :cdim], None, res=table[0], res_ids=nw.pair, m_dev=nw.n_news)
            return ops.gather_rows(nw.news_inv, rep_c, torch.empty((M, rep_c.shape[1]), dtype=torch.float32, device=dev))
        side.wait_stream(main)
        with torch.cuda.stream(side):
            pair = torch.add(fe.buckets(lifetime), fe.buckets(freshness), alpha=nb)                        # b_f * nb + b_l, int32 [M]
            table, _ = self.occurrence_tables()                                                           # [nb^2, final_dim]
        content = torch.empty((M, cdim), dtype=torch.float32, device=dev)
        self._base_encode(title_text, title_mask, content_text, category, subCategory, content, content_mask, pair_groups, title_entity,
                          recurrence)
        main.wait_stream(side)
        return ops.linear(content, self.project.weight[:, :cdim], None, res=table, res_ids=pair)         # newsEncoders.py:152-153

    def occurrence_tables(self):
        """(T, Q): what an occurrence adds to its news, for each of the num_buckets^2 (freshness bucket, lifetime bucket) pairs (row
        b_f * nb + b_l), from the current parameters -- a handful of launches on 10- and 100-row operands, per call, on the device.
        F = tanh(dense(cat(E_f[b_f], E_l[b_l]))) = tanh(E_f W[:, :E]^T [b_f] + (E_l W[:, E:]^T + b)[b_l])  (newsEncoders.py:60-83), then

            concat + project   T = F . W_p[:, c:]^T + b_p   [nb^2, final_dim]     (the freshness half of `project`, :152-153)
            concat, identity   T = F                        [nb^2, c]
            add                T = F                        [nb^2, c]             (:154-155)
            gated              T = F,  Q = F . W_g[:, c:]^T + b_g                 (the freshness half of `gate`, :156-159)

        Q is None except for 'gated'.

        The tables depend on weights alone, so a scoring call takes them from ``OccurrenceTables`` (kept across calls, refreshed in
        place: ``kept.Kept``) where ``_kept_tables`` allows it, and computes them otherwise."""
        tables = self._kept_tables()
        return tables if tables is not None else self._compute_occurrence_tables()

    def _table_sources(self):
        """Every tensor ``occurrence_tables()`` is computed from, in a fixed order."""
        fe = self.freshness_encoder
        src = [fe.freshness_embedding.weight, fe.lifetime_embedding.weight, fe.dense.weight, fe.dense.bias]
        if self.fusion_method == 'gated':
            src += [self.gate.weight, self.gate.bias]
        elif self.fusion_method == 'concat' and not isinstance(self.project, nn.Identity):
            src += [self.project.weight, self.project.bias]
        return src

    def _kept_tables(self, create=True):
        """(T, Q) from the module's ``OccurrenceTables`` (``kept.current``), or None where the caller has to compute them: the switch
        ``WEIGHT_PREP_CACHE`` off, a CPU module, autograd recording with a source that requires grad (a caller inside a training
        step: its weights move every step, and whatever it builds on the tables must not alias a buffer that a later refresh
        overwrites), and a stream capture in progress with stale tables."""
        src = kept.kept_sources(self, '_table_paths', self._table_sources, self.fusion_method)
        if not WEIGHT_PREP_CACHE or not src[0].is_cuda or (torch.is_grad_enabled() and any(t.requires_grad for t in src)):
            return None
        tables = kept.current(self, '_tables', OccurrenceTables, src, create=create)
        return None if tables is None else (tables.T, tables.Q)

    def kept_key(self):
        """``kept.key`` of the tables, or None for the fusions whose ``encode_flat`` never reads them ('add', 'gated', concat without
        a projection: their serving entries do, outside any captured graph)."""
        if self.fusion_method != 'concat' or isinstance(self.project, nn.Identity):
            return None
        return kept.key(self, '_tables', self._kept_tables)

    def _apply(self, fn, *args, **kwargs):
        kept.forget(self, '_tables', '_table_paths')
        return super()._apply(fn, *args, **kwargs)

    def _compute_occurrence_tables(self):
        """``occurrence_tables()`` from the current parameters, on the device and the current stream."""
        fe = self.freshness_encoder
        E, nb = fe.freshness_embedding.embedding_dim, fe.num_buckets
        cdim = self.base_news_encoder.news_embedding_dim
        t_f, t_l = ops.linear_group([dict(a=fe.freshness_embedding.weight, w=fe.dense.weight[:, :E], bias=None),       # [nb, cdim]
                                     dict(a=fe.lifetime_embedding.weight, w=fe.dense.weight[:, E:], bias=fe.dense.bias)])   # [nb, cdim]
        fresh = torch.tanh(t_f.unsqueeze(1) + t_l.unsqueeze(0)).view(nb * nb, -1)                         # row b_f * nb + b_l
        if self.fusion_method == 'gated':
            return fresh, ops.linear(fresh, self.gate.weight[:, cdim:], self.gate.bias)
        if self.fusion_method == 'concat' and not isinstance(self.project, nn.Identity):
            return ops.linear(fresh, self.project.weight[:, cdim:], self.project.bias), None
        return fresh, None

    def occurrence_ids(self, freshness, lifetime):
        """int32 [R]: the row b_f * nb + b_l of ``occurrence_tables()`` for each occurrence (freshness[r], lifetime[r]) -- the two bucket
        launches and their sum, nothing per column."""
        fe = self.freshness_encoder
        fr, lt = freshness.float().reshape(-1).contiguous(), lifetime.float().reshape(-1).contiguous()
        return torch.add(fe.buckets(lt), fe.buckets(fr), alpha=fe.num_buckets)

    def occurrence_ids_schedule(self, freshness, lifetime):
        """int32 [S, R]: ``occurrence_ids`` for S time slots of R occurrences whose lifetime does not move with the slot -- freshness
        [S, R], lifetime [R]: the lifetime's bucket launch runs once, over R."""
        fe = self.freshness_encoder
        S = freshness.shape[0]
        fr, lt = freshness.float().reshape(-1).contiguous(), lifetime.float().reshape(-1).contiguous()
        return torch.add(fe.buckets(lt).unsqueeze(0), fe.buckets(fr).view(S, -1), alpha=fe.num_buckets)

    # ---- per-news content cache (eval: a news occurs in many impressions, its token encoders need to run once) ----------
    def build_content_cache(self, title_text, title_mask, content_text, category, subCategory, rows_per_pass=8192, title_entity=None):
        """One row per news: everything of LIME's representation that depends on the news alone (all the token-encoder work).

        'concat' [n, output_dim]: the representation is project(cat(content(news), freshness(freshness, lifetime)))
        (newsEncoders.py:146-153) and project is linear, so  rep = content . W[:, :c]^T  +  freshness . W[:, c:]^T + b : the cache
        holds the first term per news id (the content itself when `project` is the identity).
        'add' [n, c]: the content (rep = content + freshness, :154-155).
        'gated' [n, 2 c]: columns :c the content, columns c: its half of the gate's pre-activation, content . W_g[:, :c]^T
        (rep = g content + (1 - g) freshness, g = sigmoid(gate(cat(content, freshness))), :156-159) -- one tensor, two column views.
        ``encode_cached`` adds the occurrence's side.  Rebuild it when weights change.
        ``title_entity`` [n, T]: the titles' entity ids, for the content encoder that reads them (KCNN)."""
        n = title_text.shape[0]
        reads_entity = getattr(self.base_news_encoder, 'reads_title_entity', False)
        if reads_entity and title_entity is None:
            raise TypeError('the KCNN content encoder reads the title entity ids: pass title_entity -- the ids are never guessed')
        cdim = self.base_news_encoder.news_embedding_dim
        dev = title_text.device
        ident = isinstance(self.project, nn.Identity)
        gated = self.fusion_method == 'gated'
        cache = torch.empty((n, 2 * cdim if gated else cdim if ident else self.project.out_features), dtype=torch.float32, device=dev)
        direct = gated or ident                                               # the content is (part of) the cache row itself
        for r0 in range(0, n, rows_per_pass):
            r1 = min(n, r0 + rows_per_pass)
            content = cache[r0:r1, :cdim] if direct else torch.empty((r1 - r0, cdim), dtype=torch.float32, device=dev)
            kw = dict(title_entity=_i32(title_entity[r0:r1]).contiguous()) if reads_entity else {}
            self.base_news_encoder.encode_flat(_i32(title_text[r0:r1]).contiguous(), title_mask[r0:r1].contiguous(),
                                               _i32(content_text[r0:r1]).contiguous(), _i32(category[r0:r1]).contiguous(),
                                               _i32(subCategory[r0:r1]).contiguous(), content, **kw)
            if gated:
                ops.linear(content, self.gate.weight[:, :cdim], None, out=cache[r0:r1, cdim:])
            elif not ident:
                ops.linear(content, self.project.weight[:, :cdim], None, out=cache[r0:r1])
        return cache

    def encode_cached(self, cache, news_index, freshness, lifetime, fused=None):
        """Representations of the occurrences (news_index[r], freshness[r], lifetime[r]) -> [R, output_dim].

        'add' and 'gated' take lime_cached_occurrence_f32: bucket pair, row gathers from the cache and from ``occurrence_tables()``,
        combine -- one launch behind the tables.  'concat' + project takes it with ``fused=True`` (default: ops.FUSED_OCCURRENCE,
        off) and otherwise runs FreshnessEncoder per occurrence with its half of `project` behind it, the cache gathered as a
        residual: the same sums associated differently, so the default results stay what they were."""
        cdim = self.base_news_encoder.news_embedding_dim
        R = news_index.numel()
        idx = _i32(news_index.reshape(-1)).contiguous()
        fr, lt = freshness.float().reshape(-1).contiguous(), lifetime.float().reshape(-1).contiguous()
        ident = isinstance(self.project, nn.Identity)
        if self.fusion_method != 'concat' or (not ident and (ops.FUSED_OCCURRENCE if fused is None else fused)):
            T, Q = self.occurrence_tables()
            A, P = (cache[:, :cdim], cache[:, cdim:]) if self.fusion_method == 'gated' else (cache, None)
            return ops.cached_occurrence(self.fusion_method, idx, fr, lt, A, T, P, Q, cuts=self.freshness_encoder.cuts_on(cache.device))
        fresh = torch.empty((R, cdim), dtype=torch.float32, device=cache.device)
        self.freshness_encoder.encode_flat(fr, lt, fresh)
        if ident:
            return torch.cat([cache[idx.long()], fresh], dim=1)
        return ops.linear(fresh, self.project.weight[:, cdim:], self.project.bias, res=cache, res_ids=idx)

    def encode_many(self, groups):
        """Encode several [B, n, ...] groups (candidates, history) in ONE pass over the kernels.

        Each group: (title_text, title_mask, content_text, category, subCategory, freshness, lifetime[, content_mask[, title_entity]])
        -- the optional eighth member is the body mask, which the CNE content encoder reads, the optional ninth the title's entity ids,
        which KCNN reads (every group carries them then, or none does).
        Returns one [B, n, output_dim] tensor per group.
        """
        shapes, flat, cmasks, ents = [], [[] for _ in range(7)], [], []
        for group in groups:
            tt, tm, ct, cat, sub, fr, lt = group[:7]
            if len(group) > 7 and group[7] is not None:
                cmasks.append(group[7].reshape(tt.shape[0] * tt.shape[1], -1))
            if len(group) > 8 and group[8] is not None:
                ents.append(_i32(group[8]).reshape(tt.shape[0] * tt.shape[1], -1))
            B, n = tt.shape[0], tt.shape[1]
            shapes.append((B, n))
            if fr.dim() == 1:
                fr = fr.unsqueeze(1)
            if lt.dim() == 1:
                lt = lt.unsqueeze(1)
            if lt.shape != fr.shape:
                lt = lt.expand_as(fr)
            for dst, t in zip(flat, (_i32(tt).reshape(B * n, -1), tm.reshape(B * n, -1), _i32(ct).reshape(B * n, -1),
                                     _i32(cat).reshape(-1), _i32(sub).reshape(-1), fr.float().reshape(-1), lt.float().reshape(-1))):
                dst.append(t)
        cat_all = [t[0].contiguous() if len(t) == 1 else _cat_rows(t) for t in flat]
        if cmasks and len(cmasks) != len(groups):
            raise ValueError('encode_many: the body mask must be given for every group or for none')
        cmask = None if not cmasks else (cmasks[0].contiguous() if len(cmasks) == 1 else _cat_rows(cmasks))
        # each group is one call of the reference's news encoder (model.py:171, userEncoders.py:110): CNE pairs its gates per call
        if ents and len(ents) != len(groups):
            raise ValueError('encode_many: the title entity ids must be given for every group or for none')
        if getattr(self.base_news_encoder, 'reads_title_entity', False) and not ents:
            raise TypeError('the KCNN content encoder reads the title entity ids: every group needs them -- the ids are never guessed')
        ent = None if not ents else (ents[0].contiguous() if len(ents) == 1 else _cat_rows(ents))
        out = self.encode_flat(*cat_all, content_mask=cmask, pair_groups=[B * n for B, n in shapes] if cmask is not None else None,
                               title_entity=ent)
        res, r0 = [], 0
        for (B, n) in shapes:
            res.append(out[r0:r0 + B * n].view(B, n, -1))
            r0 += B * n
        return res

    def forward(self, title_text, title_mask, title_entity, content_text, content_mask, content_entity, category, subCategory,
                user_embedding, news_freshness=None, news_user_topic_lifetime=None):
        """newsEncoders.py:140-161 -> [B, n, output_dim].  In training mode (autograd recording or dropout active) the call takes
        the differentiable path (``training.news_flat``): gradients reach every parameter the reference's do."""
        from . import training
        if training.wants_train_path(self, getattr(self.base_news_encoder, 'dropout_rate', 0.0)):
            B, n = title_text.shape[0], title_text.shape[1]
            fr, lt = news_freshness, news_user_topic_lifetime
            fr = fr.unsqueeze(1) if fr.dim() == 1 else fr
            lt = lt.unsqueeze(1) if lt.dim() == 1 else lt
            lt = lt.expand_as(fr) if lt.shape != fr.shape else lt
            rep = training.news_flat(self, *_flat_inputs(title_text, title_mask, content_text, category, subCategory),
                                     fr.float().reshape(-1).contiguous(), lt.float().reshape(-1).contiguous(),
                                     content_mask=None if content_mask is None else content_mask.reshape(B * n, -1).contiguous(),
                                     pair_groups=[B * n], title_entity=self._entity_rows(title_entity, B * n))
            return rep.view(B, n, -1)
        reads_entity = getattr(self.base_news_encoder, 'reads_title_entity', False)
        return self.encode_many([(title_text, title_mask, content_text, category, subCategory, news_freshness,
                                  news_user_topic_lifetime, content_mask, title_entity if reads_entity else None)])[0]

    def _entity_rows(self, title_entity, rows):
        if not getattr(self.base_news_encoder, 'reads_title_entity', False) or title_entity is None:
            return None
        return _i32(title_entity).reshape(rows, -1).contiguous()


class NewsEncoder(nn.Module):
    """newsEncoders.py:167-225: shared tables.  The word table is filled by the caller (``load_state_dict`` or
    ``word_embedding.weight.data.copy_``); the reference unpickles it from the cwd at :173-174.  An edit through ``.data`` moves
    neither the tensor's version counter nor its address: after one, call ``Model.weights_changed()`` (or
    ``ops.note_param_write()``) so that what CROWN keeps across forwards (``WeightProducts``) is recomputed."""

    def __init__(self, config):
        super().__init__()
        self.word_embedding_dim = config.word_embedding_dim
        self.category_num = config.category_num
        self.word_embedding = nn.Embedding(num_embeddings=config.vocabulary_size, embedding_dim=self.word_embedding_dim)
        self.category_embedding = nn.Embedding(num_embeddings=config.category_num, embedding_dim=config.category_embedding_dim)
        self.category_embedding.weight.requires_grad = False
        self.subCategory_embedding = nn.Embedding(num_embeddings=config.subCategory_num,
                                                  embedding_dim=config.subCategory_embedding_dim)
        self.subCategory_embedding.weight.requires_grad = False
        self.dropout_rate = config.dropout_rate
        self.dropout = nn.Dropout(p=config.dropout_rate, inplace=True)
        self.dropout_ = nn.Dropout(p=config.dropout_rate, inplace=False)
        self.auxiliary_loss = None
        self.affine = nn.Linear(config.word_embedding_dim, config.word_embedding_dim, bias=True)   # unused upstream too

    reads_content_mask = False      # True: encode_flat needs the body mask (CNE alone)
    reads_title_entity = False      # True: encode_flat needs the title's entity ids (KCNN alone)

    def kept_key(self):
        """``kept.key`` of what the encoder keeps across forwards and a captured ``encode_flat`` reads; None: nothing."""
        return None

    def initialize(self):
        nn.init.uniform_(self.category_embedding.weight, -0.1, 0.1)
        nn.init.uniform_(self.subCategory_embedding.weight, -0.1, 0.1)
        nn.init.zeros_(self.subCategory_embedding.weight[0])
        nn.init.xavier_uniform_(self.affine.weight)
        nn.init.zeros_(self.affine.bias)

    def forward(self, title_text, title_mask, title_entity, content_text, content_mask, content_entity, category, subCategory,
                user_embedding, news_freshness=None, news_user_topic_lifetime=None):
        B, n = title_text.shape[0], title_text.shape[1]
        flat = _flat_inputs(title_text, title_mask, content_text, category, subCategory)
        cmask = content_mask.reshape(B * n, -1).contiguous() if (self.reads_content_mask and content_mask is not None) else None
        ent = None
        if self.reads_title_entity:
            if title_entity is None:
                raise TypeError('the KCNN content encoder reads the title entity ids: pass title_entity')
            ent = _i32(title_entity).reshape(B * n, -1).contiguous()
        from . import training
        if training.wants_train_path(self, self.dropout_rate):
            return training.content_flat(self, *flat, content_mask=cmask, pair_groups=[B * n], title_entity=ent).view(B, n, -1)
        out = torch.empty((B * n, self.news_embedding_dim), dtype=torch.float32, device=title_text.device)
        if self.reads_title_entity:
            self.encode_flat(*flat, out, title_entity=ent)
        elif self.reads_content_mask:
            self.encode_flat(*flat, out, content_mask=cmask, pair_groups=[B * n])      # one call of the reference's encoder
        else:
            self.encode_flat(*flat, out)
        return out.view(B, n, -1)

    # ---- the content encoder as the model's news encoder itself (config.news_encoder = 'CROWN', 'CNN', ...: reference model.py:41-62,
    # the baselines LIME is compared with).  The surface Model calls on LIME, with the occurrence side -- freshness, the user's topic
    # lifetime -- being the identity: a representation depends on the news alone.
    occurrence_free = True          # serving.pass_logits: candidates are read in place through an index (LIME: one row per occurrence)

    def encode_rows(self, title_text, title_mask, content_text, category, subCategory, title_entity=None):
        """M flat news -> [M, news_embedding_dim] on the scoring kernels (``encode_flat`` into a fresh buffer)."""
        if self.reads_content_mask:
            raise NotImplementedError('%s pairs the news of an encoder call: it has no per-news form' % type(self).__name__)
        out = torch.empty((category.shape[0], self.news_embedding_dim), dtype=torch.float32, device=category.device)
        if self.reads_title_entity:
            if title_entity is None:
                raise TypeError('the KCNN content encoder reads the title entity ids: pass title_entity -- the ids are never guessed')
            self.encode_flat(title_text, title_mask, content_text, category, subCategory, out, title_entity=title_entity)
        else:
            self.encode_flat(title_text, title_mask, content_text, category, subCategory, out)
        return out

    def encode_many(self, groups):
        """``LIME.encode_many`` without the occurrence side: several [B, n, ...] groups (candidates, history) in ONE pass over the kernels
        -> one [B, n, news_embedding_dim] tensor per group.  A group's freshness, lifetime and body mask (members six to eight) are
        accepted and not read; the ninth, the title's entity ids, is read by KCNN alone."""
        shapes, flat, ents = [], [[] for _ in range(5)], []
        for group in groups:
            tt, tm, ct, cat, sub = group[:5]
            B, n = tt.shape[0], tt.shape[1]
            shapes.append((B, n))
            if len(group) > 8 and group[8] is not None:
                ents.append(_i32(group[8]).reshape(B * n, -1))
            for dst, t in zip(flat, (_i32(tt).reshape(B * n, -1), tm.reshape(B * n, -1), _i32(ct).reshape(B * n, -1),
                                     _i32(cat).reshape(-1), _i32(sub).reshape(-1))):
                dst.append(t)
        if ents and len(ents) != len(groups):
            raise ValueError('encode_many: the title entity ids must be given for every group or for none')
        cat_all = [t[0].contiguous() if len(t) == 1 else _cat_rows(t) for t in flat]
        ent = None if not ents else (ents[0].contiguous() if len(ents) == 1 else _cat_rows(ents))
        out = self.encode_rows(*cat_all, title_entity=ent)
        res, r0 = [], 0
        for (B, n) in shapes:
            res.append(out[r0:r0 + B * n].view(B, n, -1))
            r0 += B * n
        return res

    def build_content_cache(self, title_text, title_mask, content_text, category, subCategory, rows_per_pass=8192, title_entity=None):
        """One row per news [n, news_embedding_dim]: the news' representation itself (nothing of it depends on the occurrence).
        Rebuild it when weights change.  ``title_entity`` [n, T]: the titles' entity ids, for KCNN."""
        n = title_text.shape[0]
        if self.reads_title_entity and title_entity is None:
            raise TypeError('the KCNN content encoder reads the title entity ids: pass title_entity -- the ids are never guessed')
        cache = torch.empty((n, self.news_embedding_dim), dtype=torch.float32, device=title_text.device)
        for r0 in range(0, n, rows_per_pass):
            r1 = min(n, r0 + rows_per_pass)
            kw = dict(title_entity=_i32(title_entity[r0:r1]).contiguous()) if self.reads_title_entity else {}
            self.encode_flat(_i32(title_text[r0:r1]).contiguous(), title_mask[r0:r1].contiguous(), _i32(content_text[r0:r1]).contiguous(),
                             _i32(category[r0:r1]).contiguous(), _i32(subCategory[r0:r1]).contiguous(), cache[r0:r1], **kw)
        return cache

    def encode_cached(self, cache, news_index, freshness=None, lifetime=None, fused=None):
        """Representations of the occurrences -> [R, news_embedding_dim]: a row gather from the cache (``freshness`` / ``lifetime`` are
        accepted and not read)."""
        idx = _i32(news_index.reshape(-1)).contiguous()
        return ops.gather_rows(idx, cache, torch.empty((idx.numel(), cache.shape[1]), dtype=torch.float32, device=cache.device))


class PositionalEncoding(nn.Module):
    """newsEncoders.py:806-828: the sinusoid table, a registered buffer (part of the state_dict)."""

    def __init__(self, d_model, dropout=0.1, max_len=5000):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2) * (-math.log(10000.0) / d_model))
        pe = torch.zeros(max_len, d_model)
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer('pe', pe.unsqueeze(0))

    def table(self):
        return self.pe[0]


class _MAB(nn.Module):
    """Parameter holder for newsEncoders.py:395-422 (never called on the scoring path)."""

    def __init__(self, dim_Q, dim_K, dim_V, num_heads, ln=False):
        super().__init__()
        self.fc_q = nn.Linear(dim_Q, dim_V)
        self.fc_k = nn.Linear(dim_K, dim_V)
        self.fc_v = nn.Linear(dim_K, dim_V)
        if ln:
            self.ln0 = nn.LayerNorm(dim_V)
            self.ln1 = nn.LayerNorm(dim_V)
        self.fc_o = nn.Linear(dim_V, dim_V)


class ISAB(nn.Module):
    """Parameter holder: the reference constructs ISAB (newsEncoders.py:250-254) and never calls it (:325-333 are
    commented out), but its 25 tensors are part of the checkpoint."""

    def __init__(self, dim_in, dim_out, num_heads, num_inds, ln=False):
        super().__init__()
        self.I = nn.Parameter(torch.Tensor(1, num_inds, dim_out))
        nn.init.xavier_uniform_(self.I)
        self.mab0 = _MAB(dim_out, dim_in, dim_out, num_heads, ln=ln)
        self.mab1 = _MAB(dim_in, dim_out, dim_out, num_heads, ln=ln)


class CategoryPredictor(nn.Module):
    """Parameter holder for newsEncoders.py:375-393: under LIME the auxiliary loss is dead."""

    def __init__(self, title_embedding, category_num):
        super().__init__()
        self.fc = nn.Linear(title_embedding, category_num)


# How one pass over a token encoder addresses its rows: all that differs between the dense batch and the compacted one (csrc/compact.hip).
#   n_seq, S            sequences the layer runs over (M, or M + 1 compacted: the live ones + the all-padding representative)
#   a_ids, res_ids      word ids of the first in_proj's A gather / of the residual out_proj rebuilds
#   w_in, pew           the first layer's in_proj weight (heads padded) and the positional table through it (+ bias), [S, 3W]
# compacted only (None on the dense batch):
#   qkv                 the first layer's q / k / v buffer, the S padding rows filled in behind its n_seq * S compact rows
#   c_ids, m_tok        the first in_proj's scatter list and the device count of live tokens
#   m_rows, n_seq_dev   device counts of compact rows / sequences
#   row_map             the first layer's attention looks every token's q / k / v row up through it
#   seq_inv             pooled_out[s] = pooled rows[seq_inv[s]]
# kept across forwards (``WeightProducts``; None: computed in this forward):
#   ew                  the word table through the first in_proj, [V, 3W]: with it the first layer runs no in_proj, attention reads
#                       token r's q / k / v as ew[res_ids[r]] + pew[r % S] (a padding token is id 0), and w_in / qkv / c_ids /
#                       row_map are not needed
#   ffn                 per layer, the (w1p, w2p) of ops.ffn_pack_sp
#   oproj               per layer, the packed out_proj weight of ops.oproj_pack_sp
_Rows = collections.namedtuple('_Rows', 'n_seq S a_ids res_ids w_in pew qkv c_ids m_tok m_rows n_seq_dev row_map seq_inv ew ffn oproj',
                               defaults=(None,) * 10)


def _encode_layers(r, table, pe, transformer, nhead, pooled_out, blocks_only=False):
    """Word gather + positional table + the post-LN encoder layer(s) of newsEncoders.py:311-320 over the rows ``r`` describes: in_proj,
    attention, out_proj + residual + norm1, linear1 + ReLU, linear2 + residual + norm2 -- five launches per layer (four with the fused
    feed-forward), activations stay fp32.  With ``pooled_out`` the token mean pooling of :317 / :321 is taken in the last GEMM's
    epilogue (pool32: means over 32-token blocks; a longer sequence is finished by a mean over its S / 32 block rows) and the layer
    output never reaches HBM; returns None then, the layer output [n_seq * S, E] otherwise.  ``blocks_only`` (compacted rows, no
    ``pooled_out``): returns the last GEMM's block means [n_seq * S / 32, E] in compact order and leaves the rest of the pooling and
    the expansion through ``seq_inv`` to the caller (ops.news_xin)."""
    n_seq, S = r.n_seq, r.S
    E = table.shape[1]
    hd = E // nhead
    hs = 32 if hd <= 32 else hd                    # heads padded to 32 columns in the in_proj output: the 128 x 320 GEMM
    W = nhead * hs                                 # tiles compute those columns anyway, and attention gets 16-byte loads
    scale = 1.0 / math.sqrt(hd)
    rows = dict(m_dev=r.m_rows)
    pooled = pooled_out if r.seq_inv is None else None            # compacted: the pooled rows in compact order first
    x = None
    for li, layer in enumerate(transformer.layers):
        sa = layer.self_attn
        ln1 = (layer.norm1.weight, layer.norm1.bias)
        qkv = None
        if li == 0 and r.ew is not None:
            # (E W^T)[ids] + (PE W^T + b)[t] with both products kept across forwards: no in_proj, attention adds the two rows
            res = dict(res=table, res_ids=r.res_ids, res_pe=pe, res_period=S)
        elif li == 0:
            # (E[ids] + PE) W^T + b = E[ids] W^T + (PE W^T + b)[t]: the positional term is an [S, 3W] table added as a
            # periodic residual, so the A operand is a pure row gather (which the LDS-DMA GEMM can stage directly)
            qkv = ops.linear(table, r.w_in, None, a_ids=r.a_ids, res=r.pew, res_mod=S, n_alg=3 * E, c_ids=r.c_ids, m_dev=r.m_tok,
                             out=None if r.qkv is None else r.qkv[:n_seq * S])
            qkv = qkv if r.qkv is None else r.qkv
            res = dict(res=table, res_ids=r.res_ids, res_pe=pe, res_period=S)
        else:
            # a layer behind the first (config.py:70 allows num_layers = 2): its input rows are all distinct, so of the compaction only
            # the sequence-level sharing is left -- device-side row counts, attention through the identity map
            w_in = ops.pad_heads(sa.in_proj_weight, 3 * nhead, hd, hs) if hs != hd else sa.in_proj_weight
            b_in = ops.pad_heads(sa.in_proj_bias, 3 * nhead, hd, hs) if hs != hd else sa.in_proj_bias
            qkv = ops.linear(x, w_in, b_in, n_alg=3 * E, **rows)
            res = dict(res=x)
        if qkv is None:
            attn = ops.token_attention_vocab(r.ew, r.pew, r.res_ids, r.n_seq_dev, n_seq, S, nhead, hd, scale)
            if attn is None:
                raise RuntimeError('the vocab form of lime_token_attention_f32 does not cover S = %d, head_dim = %d (vocab_qkv_applicable said it would)' % (S, hd))
        elif r.row_map is None:
            attn = ops.token_attention(qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:], n_seq, S, nhead, hd, scale, head_stride=hs)
        else:
            attn = ops.token_attention_rows(qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:],
                                            r.row_map if li == 0 else _identity_rows(n_seq * S, table.device), r.n_seq_dev,
                                            n_seq, S, nhead, hd, scale)
        if _oproj_sp_applicable(sa, attn, res):
            # out_proj + residual + norm1 as split products in one token-stationary launch
            wop = r.oproj[li] if r.oproj is not None and r.oproj[li] is not None else ops.oproj_pack_sp(sa.out_proj.weight)
            x1 = ops.encoder_oproj_sp(attn, wop, sa.out_proj.bias, ln1, layer.norm1.eps, **res, **rows)
        else:
            x1 = ops.linear(attn, sa.out_proj.weight, sa.out_proj.bias, ln=ln1, ln_eps=layer.norm1.eps, **res, **rows)
        last = li == len(transformer.layers) - 1
        pool = last and (pooled_out is not None or blocks_only) and transformer.norm is None and S % 32 == 0 and n_seq * S >= 4096
        ln2 = (layer.norm2.weight, layer.norm2.bias)
        if _ffn_sp_applicable(layer, x1):
            # linear1 + ReLU + linear2 + residual + norm2 (+ the 32-token block means of the last layer) in one launch
            w1p, w2p = r.ffn[li] if r.ffn is not None else ops.ffn_pack_sp(layer.linear1.weight, layer.linear2.weight)
            direct = S == 32 and (pooled is None or (pooled.data_ptr() % 16 == 0 and pooled.stride(0) % 4 == 0))
            ffn = lambda **kw: ops.encoder_ffn_sp(x1, w1p, w2p, layer.linear1.bias, layer.linear2.bias, ln2, layer.norm2.eps, **kw, **rows)
        else:
            h = ops.linear(x1, layer.linear1.weight, layer.linear1.bias, act='relu', **rows)
            direct = S == 32
            ffn = lambda **kw: ops.linear(h, layer.linear2.weight, layer.linear2.bias, res=x1, ln=ln2, ln_eps=layer.norm2.eps, **kw, **rows)
        if not pool:
            x = ffn()
            continue
        if blocks_only:
            return ffn(pool32=True)
        blocks = ffn(pool32=True, out=pooled if direct else None)                                      # [n_seq * S / 32, E] block means
        pooled = blocks if direct else ops.mean_pool(blocks, n_seq, S // 32, out=pooled, n_seq_dev=r.n_seq_dev)
        break
    else:
        if transformer.norm is not None:
            raise NotImplementedError('a final encoder norm is not used by the reference (newsEncoders.py:245,247)')
        if blocks_only:
            raise NotImplementedError('blocks_only needs the pooled epilogue (S a multiple of 32, >= 4096 rows: compact_applicable)')
        if pooled_out is None:
            return x
        pooled = ops.mean_pool(x, n_seq, S, out=pooled, n_seq_dev=r.n_seq_dev)
    if r.seq_inv is not None:
        ops.gather_rows(r.seq_inv, pooled, pooled_out)
    return None


def encode_tokens(ids, table, pe, transformer, nhead, pooled_out=None):
    """``_encode_layers`` over every token of the dense batch.  ids: [M, S] int32 (every id must be in [0, V): unchecked, as on
    nn.Embedding's device path); returns the layer output [M * S, E], or None with ``pooled_out`` ([M, E])."""
    M, S = ids.shape
    hd = table.shape[1] // nhead
    sa = transformer.layers[0].self_attn
    w_in = ops.pad_heads(sa.in_proj_weight, 3 * nhead, hd, 32) if hd < 32 else sa.in_proj_weight
    b_in = ops.pad_heads(sa.in_proj_bias, 3 * nhead, hd, 32) if hd < 32 else sa.in_proj_bias
    flat = ids.reshape(-1)
    return _encode_layers(_Rows(M, S, flat, flat, w_in, ops.linear(pe[:S], w_in, b_in)), table, pe, transformer, nhead, pooled_out)


def encode_tokens_compact(ids, table, pe, transformer, nhead, pooled_out, products=None):
    """``encode_tokens(..., pooled_out)`` without the repetitions of a padded batch (csrc/compact.hip): the history slots of an
    impression are padded with the all-zero <PAD> news (corpus.py:476-477, dataset.py:105-141) and every text with the padding
    word behind it; the reference encodes them all (newsEncoders.py:311-321).

      * sequence level: an all-padding sequence pools to the same vector wherever it stands (no mask, no cross-sequence term in
        the layer), so the live sequences + ONE all-padding representative go through the layer (n_c = live + 1 sequences) and
        ``pooled_out[s] = pooled_c[seq_inv[s]]``;
      * token level: the in_proj row of a padding token is (E[0] + PE[t]) W^T + b, a function of its position alone: S table
        rows computed once; in_proj runs over the live tokens (rows scattered to their compact positions) and attention looks
        every token's q / k / v row up through ``row_map``.  From the attention output on every position is distinct.

    Counts live in device memory (lime_linear_args.m_dev / n_seq_dev), buffers have their full-batch size: the forward stays one
    HIP graph.  Same kernels, same per-row arithmetic as the dense path; results differ from it only through the S padding rows
    coming from the small-M GEMM kernel (different k order, ~1e-7).  Returns None (the result is ``pooled_out``).

    ``products``: this encoder's entry of ``WeightProducts.encoder`` (weight-only results kept across forwards: the word and
    positional tables through the first in_proj, the packed feed-forward weights); the first layer then runs no in_proj at all.
    """
    return compact_run(compact_prepare(ids, table, pe, transformer, nhead, products), table, pe, transformer, nhead, pooled_out)


def compact_prepare(ids, table, pe, transformer, nhead, products=None):
    """Everything of ``encode_tokens_compact`` in front of the big GEMMs -- index lists, padded in_proj weights, the positional
    table through in_proj, the S rows shared by the padding tokens: a dozen short launches that depend on the ids and the
    weights only, so the caller can run them on a side stream under another encoder's GEMMs."""
    return compact_prepare_many([(ids, pe, transformer)], table, nhead, products=None if products is None else [products])[0]


def compact_prepare_many(encoders, table, nhead, cmps=None, products=None):
    """``compact_prepare`` for several token encoders over one word table ((ids, pe, transformer) each): their positional tables go
    through in_proj in ONE grouped launch, their padding rows in another (independent, latency-bound GEMMs).  ``cmps``: the encoders'
    index lists when the caller has them already (``ops.compact_batch``).  ``products``: per encoder, its entry of
    ``WeightProducts.encoder`` or None; an encoder whose entry holds ``ew`` needs the index lists only -- no padded weights, no
    positional GEMM, no padding rows, no q / k / v buffer."""
    E = table.shape[1]
    hd = E // nhead
    W = nhead * 32
    products = products or [None] * len(encoders)
    preps, parts = [None] * len(encoders), []
    for i, (ids, pe, transformer) in enumerate(encoders):
        M, S = ids.shape
        sa = transformer.layers[0].self_attn
        cap = (M + 1) * S
        cmp = ops.compact_sequences(ids) if cmps is None else cmps[i]           # pad rows live at qkv[cap : cap + S]
        prod = products[i] or {}
        if prod.get('ew') is not None:
            preps[i] = (cmp, None, prod['pew'], None, prod)
            continue
        w_in = ops.pad_heads(sa.in_proj_weight, 3 * nhead, hd, 32)
        b_in = ops.pad_heads(sa.in_proj_bias, 3 * nhead, hd, 32)
        qkv = torch.empty((cap + S, 3 * W), dtype=torch.float32, device=ids.device)
        parts.append((cmp, w_in, b_in, qkv, pe, S, cap, i, prod))
    if parts:
        pews = ops.linear_group([dict(a=pe[:S], w=w_in, bias=b_in) for (_, w_in, b_in, _, pe, S, _, _, _) in parts])   # [S, 3W]: positional term + bias
        ops.linear_group([dict(a=table, w=w_in, bias=None, a_ids=_zero_ids(S, table.device), res=pew, res_mod=S, out=qkv[cap:])
                          for (_, w_in, _, qkv, _, S, cap, _, _), pew in zip(parts, pews)])                       # the S padding rows
        for (cmp, w_in, _, qkv, _, _, _, i, prod), pew in zip(parts, pews):
            preps[i] = (cmp, w_in, pew, qkv, prod)
    return preps


SP_FUSED_FFN = os.environ.get('LIME_SP_FUSED_FFN', '1') != '0'      # 0: the fp32 linear1 / linear2 as two lime_linear_f32 launches (A/B runs)


def _ffn_sp_shape(layer, E):
    """The shapes lime_encoder_ffn_sp / lime_ffn_pack_sp are built for: E <= 304 (E % 4 == 0), F a multiple of 128 up to 4096, biases."""
    F = layer.linear1.out_features
    return (E <= 304 and E % 4 == 0 and F % 128 == 0 and F <= 4096 and layer.linear1.bias is not None and
            layer.linear2.bias is not None)


def _ffn_sp_applicable(layer, x1):
    """lime_encoder_ffn_sp takes the fp32 feed-forward half where lime_linear_f32 would run both GEMMs as split products: the split
    GEMM on, a shape of ``_ffn_sp_shape``, 16-byte rows, and enough 128-row blocks that linear1 is not left to the mid-M kernel
    (lime_linear_f32's fill rule)."""
    M, E = x1.shape
    F = layer.linear1.out_features
    return (SP_FUSED_FFN and ops.split_gemm_on() and _ffn_sp_shape(layer, E) and x1.stride(1) == 1 and x1.stride(0) % 4 == 0 and
            x1.data_ptr() % 16 == 0 and M >= 4096 and ((M + 127) // 128) * ((F + 255) // 256) >= 160)


SP_OPROJ = os.environ.get('LIME_SP_OPROJ', '1') != '0'      # 0: the fp32 out_proj + norm1 stays with lime_linear_f32 (A/B runs)


def oproj_sp_rule(on, split_on, M, E, has_bias, aligned):
    """The rule of ``_oproj_sp_applicable`` as a pure function: the switch and the split GEMM on, E within the build (E <= 304,
    E % 4 == 0), a bias, 16-byte rows, at least 4096 rows and 160 tiles of 128 rows -- below that a persistent grid of one workgroup
    per CU leaves too much of the chip idle and lime_linear_f32's own fill rules choose better."""
    return bool(on and split_on and 0 < E <= 304 and E % 4 == 0 and has_bias and aligned and M >= 4096 and (M + 127) // 128 >= 160)


def _oproj_sp_applicable(sa, attn, res):
    """lime_encoder_oproj_sp takes out_proj + residual + norm1 of the fp32 scoring layers (compacted or dense rows, every layer)
    under ``oproj_sp_rule``; ``res``: the residual arguments ``_encode_layers`` would hand ``ops.linear``."""
    M, E = attn.shape
    ok16 = lambda t: t is None or (t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0)
    return oproj_sp_rule(SP_OPROJ, ops.split_gemm_on(), M, E, sa.out_proj.bias is not None,
                         ok16(attn) and ok16(res['res']) and ok16(res.get('res_pe')))


_IDENT = {}


def _identity_rows(n, device):
    """arange(n) int32, allocated once per device: the row map of an encoder layer behind the first (every compact row is its own)."""
    return _grown(_IDENT, n, device, 4096, lambda size: torch.arange(size, dtype=torch.int32, device=device))


def compact_run(prep, table, pe, transformer, nhead, pooled_out, blocks_only=False):
    """``encode_tokens_compact`` behind its preparation: the layer(s) over the compacted rows, ``pooled_out`` through ``seq_inv`` (or,
    ``blocks_only``, the compact block means returned: see ``_encode_layers``)."""
    cmp, w_in, pew, qkv, prod = prep
    rows = _Rows(cmp.n_seq + 1, cmp.S, cmp.tok_ids, cmp.ids_c, w_in, pew, qkv, c_ids=cmp.tok_rows, m_tok=cmp.n_live_tokens,
                 m_rows=cmp.n_rows, n_seq_dev=cmp.n_compact, row_map=cmp.row_map, seq_inv=cmp.seq_inv, ew=prod.get('ew'),
                 ffn=prod.get('ffn'), oproj=prod.get('oproj'))
    return _encode_layers(rows, table, pe, transformer, nhead, pooled_out, blocks_only)


def compact_applicable(ids, table, transformer, nhead):
    """The compacted path covers the shapes of the big-M kernels: post-LN layers without a final norm, head_dim <= 32,
    S a multiple of 32 that the row-map attention is built for, at least 4096 token rows, 16-byte aligned table rows."""
    M, S = ids.shape
    E = table.shape[1]
    return (DEDUP and len(transformer.layers) >= 1 and transformer.norm is None and E % nhead == 0 and E // nhead <= 32 and
            E % 4 == 0 and S % 32 == 0 and (S // 32 <= 4 or S // 32 in (8, 16)) and (M + 1) * S >= 4096 and
            ids.dtype == torch.int32 and ids.is_contiguous())


FUSED_FFN = os.environ.get('LIME_BF16_FUSED_FFN', '1') != '0'        # 0: linear1 / linear2 as two lime_linear_bf16 launches (A/B runs)
FUSED_BLOCK = FUSED_FFN and os.environ.get('LIME_BF16_FUSED_BLOCK', '1') != '0'     # 0: out_proj + norm1 as its own launch


def _inproj_applicable(N, K):
    """lime_inproj_bf16: q / k / v columns in passes of 320 (ten heads padded to 32), K <= 320."""
    return FUSED_FFN and N % 320 == 0 and K <= 320 and K % 8 == 0


def _ffn_fused_applicable(layer, E, EP):
    """lime_encoder_ffn_bf16 is built for the reference's encoder shape: E = 300 carried as 304, hidden width a multiple of 128."""
    return (FUSED_FFN and EP == ops.ffn_model_columns() and EP - 15 <= E < EP and layer.linear1.out_features % 128 == 0 and
            layer.linear1.bias is not None and layer.linear2.bias is not None)


def _pack_layer_bf16(layer, first, pe, S, EP, nhead):
    """The weights of one encoder layer in the packings its bf16 launches take -- which launches those are is decided here, from the
    switches and the layer's shape.  E = 300 is carried as EP = 304 columns (zero weights / bias / gamma / beta in the pad, so the
    pad stays exactly zero through the layer).  ``first``: the layer whose input is the word gather + positional table."""
    sa = layer.self_attn
    E = pe.shape[1]
    hd = E // nhead
    padv = lambda v: torch.cat([v, v.new_zeros(EP - E)])
    p = types.SimpleNamespace(inproj=_inproj_applicable(3 * nhead * 32, EP), ffn=_ffn_fused_applicable(layer, E, EP))
    p.block = FUSED_BLOCK and p.ffn and E % 4 == 0
    w_in = ops.pad_heads(sa.in_proj_weight, 3 * nhead, hd, 32)                      # fp32 [3W, E]
    b_in = ops.pad_heads(sa.in_proj_bias, 3 * nhead, hd, 32)
    p.w_in = ops.inproj_pack_bf16(w_in, EP) if p.inproj else ops.to_bf16(w_in, cols_out=EP)
    # what in_proj adds to its rows: the first layer's positional term + bias (fp32 [S, 3W]), the bias alone behind it
    p.in_rows = ops.linear(pe[:S], w_in, b_in) if first else b_in.view(1, -1) if p.inproj else b_in
    if p.ffn:
        p.w1p, p.w2p = ops.ffn_pack_bf16(layer.linear1.weight, layer.linear1.bias, layer.linear2.weight)
    else:
        p.w1, p.w2 = ops.to_bf16(layer.linear1.weight, cols_out=EP), ops.to_bf16(layer.linear2.weight, rows_out=EP)
        p.b2, p.ln2 = padv(layer.linear2.bias), (padv(layer.norm2.weight), padv(layer.norm2.bias))
    if p.block:
        p.w0p = ops.oproj_pack_bf16(sa.out_proj.weight)
        p.add_rows = pe[:S] + sa.out_proj.bias if first else sa.out_proj.bias.view(1, E)
    else:
        p.w_o, p.b_o = ops.to_bf16(sa.out_proj.weight, rows_out=EP, cols_out=EP), padv(sa.out_proj.bias)
        p.ln1 = (padv(layer.norm1.weight), padv(layer.norm1.bias))
        p.pe_p = torch.cat([pe[:S], pe.new_zeros(S, EP - E)], dim=1) if first else None
    return p


def _encode_layers_bf16(ids, cmp, table_bf16, pe, transformer, nhead, pooled_out, shared=None):
    """The encoder layer(s) + mean pool on the bf16 matrix cores, over every token of ``ids`` (``cmp`` None) or over its compacted batch
    (``cmp = ops.compact_sequences(ids)``, one layer): in_proj (activation-stationary, or lime_linear_bf16) -> attention -> everything
    behind it in one launch / out_proj + fused feed-forward / three GEMMs -> 32-token block means -> ``pooled_out``.  Activations
    between the launches are bf16; accumulation, bias, residual adds, softmax and LayerNorm are fp32.  ``shared``: a dict that lives
    for one forward, through which the passes over one encoder share its packed weights."""
    M, S = ids.shape
    EP = table_bf16.shape[1]
    E = pe.shape[1]
    hd = E // nhead
    if hd > 32 or S % 32 != 0:
        raise NotImplementedError('the bf16 encoder path needs head_dim <= 32 and S a multiple of 32 (got %d, %d)' % (hd, S))
    if transformer.norm is not None:
        raise NotImplementedError('a final encoder norm is not used by the reference (newsEncoders.py:245,247)')
    W = nhead * 32
    scale = 1.0 / math.sqrt(hd)
    shared = {} if shared is None else shared
    if cmp is None:
        n_seq, a_ids, res_ids, c_ids, n_seq_dev, rows = M, ids.reshape(-1), ids.reshape(-1), None, None, {}
    else:                            # live sequences + one all-padding representative, in_proj over the live tokens, the row-map attention
        n_seq, a_ids, res_ids, c_ids, n_seq_dev, rows = M + 1, cmp.tok_ids, cmp.ids_c, cmp.tok_rows, cmp.n_compact, dict(m_dev=cmp.n_rows)
    cap = n_seq * S
    x = None
    for li, layer in enumerate(transformer.layers):
        if li not in shared:
            shared[li] = _pack_layer_bf16(layer, li == 0, pe, S, EP, nhead)
        p = shared[li]
        # compacted: the S rows shared by the padding tokens, which the row map points at, stand behind the cap compact rows
        qkv = torch.empty((cap if cmp is None else cap + S, 3 * W), dtype=torch.bfloat16, device=ids.device)
        if li > 0 and p.inproj:
            ops.inproj_bf16(x, p.w_in, p.in_rows, 3 * W, qkv)
        elif li > 0:
            ops.linear_bf16(x, p.w_in, p.in_rows, n_alg=3 * E, k_alg=E, out=qkv)
        elif p.inproj:
            # activation-stationary q / k / v projection (csrc/inproj_bf16.hip): the tile is read once for all 3 W columns; compacted:
            # the S padding rows are entries of the token list behind the live tokens
            ops.inproj_bf16(table_bf16, p.w_in, p.in_rows, 3 * W, qkv, a_ids=a_ids, c_ids=c_ids,
                            m_dev=None if cmp is None else cmp.n_tokens_and_pad_rows)
        else:
            if cmp is not None:
                ops.linear_bf16(table_bf16, p.w_in, None, a_ids=_zero_ids(S, ids.device), res=p.in_rows, res_kind=1, res_mod=S, out=qkv[cap:])
            ops.linear_bf16(table_bf16, p.w_in, None, a_ids=a_ids, res=p.in_rows, res_kind=1, res_mod=S, out=qkv[:cap], c_ids=c_ids,
                            m_dev=None if cmp is None else cmp.n_live_tokens, n_alg=3 * E, k_alg=E)
        q, k, v = qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:]
        if cmp is None:
            attn = ops.token_attention_bf16(q, k, v, n_seq, S, nhead, hd, scale, out_cols=EP)
        else:
            attn = ops.token_attention_rows_bf16(q, k, v, cmp.row_map, n_seq_dev, n_seq, S, nhead, hd, scale, out_cols=EP)
        sa = layer.self_attn
        pool = li == len(transformer.layers) - 1                  # token mean pooling in the epilogue: fp32 means over 32-token blocks
        res = dict(res=table_bf16, res_kind=2, res_ids=res_ids) if li == 0 else dict(res=x, res_kind=3)
        ln2 = (layer.norm2.weight, layer.norm2.bias)
        if p.block:
            # everything behind the attention core in ONE launch (csrc/ffn_bf16.hip): out_proj + residual + norm1 written into the
            # stationary LDS tile the feed-forward half then reads
            x = ops.encoder_block_bf16(attn, p.w0p, p.add_rows, (layer.norm1.weight, layer.norm1.bias), layer.norm1.eps, w1p=p.w1p, w2p=p.w2p,
                                       b2=layer.linear2.bias, ln2=ln2, ln2_eps=layer.norm2.eps, E=E, pool32=pool, **res, **rows)
            continue
        x1 = ops.linear_bf16(attn, p.w_o, p.b_o, res_pe=p.pe_p, res_period=S if li == 0 else 0, ln=p.ln1, ln_eps=layer.norm1.eps, ln_count=E,
                             n_alg=E, k_alg=E, **res, **rows)
        if p.ffn:
            # linear1 + ReLU + linear2 + residual + norm2 in ONE launch: the hidden state stays in registers (csrc/ffn_bf16.hip)
            x = ops.encoder_ffn_bf16(x1, p.w1p, p.w2p, layer.linear2.bias, ln2, layer.norm2.eps, E, pool32=pool, **rows)
            continue
        h = ops.linear_bf16(x1, p.w1, layer.linear1.bias, act='relu', k_alg=E, **rows)
        x = ops.linear_bf16(h, p.w2, p.b2, res=x1, res_kind=3, ln=p.ln2, ln_eps=layer.norm2.eps, ln_count=E, pool32=pool, n_alg=E, **rows)
    # x: the last layer's block means, fp32 [cap / 32, EP]
    pooled = ops.mean_pool(x[:, :E], n_seq, S // 32, out=pooled_out if cmp is None else None, n_seq_dev=n_seq_dev)
    if cmp is not None:
        ops.gather_rows(cmp.seq_inv, pooled, pooled_out)
    return None


def encode_tokens_bf16(ids, table_bf16, pe, transformer, nhead, pooled_out):
    """encode_tokens + mean pool on the bf16 matrix cores (BASELINE config 3).  table_bf16: the word table converted with
    ``ops.to_bf16`` ([V, E rounded up to 8], zero padded)."""
    return _encode_layers_bf16(ids, None, table_bf16, pe, transformer, nhead, pooled_out)


def encode_tokens_bf16_compact(ids, table_bf16, pe, transformer, nhead, pooled_out, shared=None):
    """``encode_tokens_bf16`` on the compacted batch (see ``encode_tokens_compact``).  The S padding rows come from the same bf16
    GEMM kernel as the live rows (lime_linear_bf16 takes any M)."""
    if len(transformer.layers) != 1:
        raise NotImplementedError('the compacted bf16 path covers one encoder layer (compact_applicable_bf16)')
    return _encode_layers_bf16(ids, ops.compact_sequences(ids), table_bf16, pe, transformer, nhead, pooled_out, shared)


def compact_applicable_bf16(ids, transformer, nhead, E):
    M, S = ids.shape
    return (DEDUP and len(transformer.layers) == 1 and transformer.norm is None and E % nhead == 0 and E // nhead <= 32 and
            (E // nhead) % 2 == 0 and S in (32, 64, 128) and (M + 1) * S >= 4096 and ids.dtype == torch.int32 and ids.is_contiguous())


# ---- weight-only results kept across forwards ------------------------------------------------------------------------------------
# 0 (LIME_VOCAB_QKV=0): every forward derives what it needs from the weights itself -- in_proj over the batch's tokens, the
# feed-forward weights packed per call -- as before ``WeightProducts`` (A/B runs)
VOCAB_QKV = os.environ.get('LIME_VOCAB_QKV', '1') != '0'
# 0 (LIME_WEIGHT_PREP_CACHE=0): the small weight-only preparation of a scoring forward -- CROWN's stacked intent weights, LIME's
# occurrence tables -- is computed in every forward (and by every serving call) as before it was kept (A/B runs)
WEIGHT_PREP_CACHE = os.environ.get('LIME_WEIGHT_PREP_CACHE', '1') != '0'


def vocab_qkv_applicable(S, E, nhead):
    """The vocab form of ``lime_token_attention_f32`` covers the first layer of a token encoder over S-token sequences."""
    return S in (32, 64, 128) and E % nhead == 0 and E // nhead <= 32 and E % 4 == 0


class WeightProducts(kept.Kept):
    """What the fp32 token encoders of a CROWN module compute from weights alone, kept from one scoring forward to the next:

      * per encoder, ``ew`` = E W_in^T over the WHOLE word table ([V, 3W], heads padded to 32 columns) and ``pew`` = PE W_in^T + b
        ([S, 3W]): the first layer then runs no in_proj -- attention reads a token's q / k / v row as ew[id] + pew[t]
        (ops.token_attention_vocab).  One forward of the flagship batch pushes 79k token rows through that GEMM against a
        50k-row table, and a dev pass scores thousands of batches between two weight updates;
      * per encoder and layer, the packed feed-forward weights of ``ops.ffn_pack_sp`` and the packed out_proj weight of
        ``ops.oproj_pack_sp``;
      * ``intent``: the k intent layers' weights stacked row-wise with zero pad columns (``w`` [k D, ldx]) and their biases (``b``
        [k D]), what the tail's one GEMM over the k layers reads (``WEIGHT_PREP_CACHE``; they were two cats, a pad and a copy per
        forward).

    ``config`` = (``budget``: the bytes of [V, 3W] products the module may keep, whether ``intent`` is kept).  Staleness, the in-place
    refresh and ``generation``: ``kept.Kept``."""

    def __init__(self):
        super().__init__()
        self.encoder = [{}, {}]            # title, body: dict(ew=, pew=, ffn=[(w1p, w2p) per layer], oproj=[wp per layer]); 'ew' / 'pew' absent over the budget
        self.intent = {}                   # dict(w=, b=), or empty with WEIGHT_PREP_CACHE off

    def refresh(self, crown, config):
        """Recompute everything from ``crown``'s weights, on the current stream."""
        self.budget, keep_intent = config                          # (budget: the one this set was built under)
        table, nhead = crown.word_embedding.weight, crown.head_num
        encoders = ((crown.title_pos_encoder.table(), crown.title_transformer, crown.max_title_length),
                    (crown.body_pos_encoder.table(), crown.body_transformer, crown.max_body_length))
        V, E = table.shape
        want = [vocab_qkv_applicable(S, E, nhead) for _, _, S in encoders]
        if sum(V * 3 * nhead * 32 * 4 for w in want if w) > self.budget:
            want = [False, False]
        if keep_intent:
            self._stack_intent(list(crown.intent_layers), table.device)
        elif self.intent:
            self.intent = {}
            self.let_go()
        for ent, (pe, transformer, S), w in zip(self.encoder, encoders, want):
            self._vocab_products(ent, table, pe[:S], transformer.layers[0].self_attn, nhead, w)
            self._packs(ent, transformer.layers, E, table.device)

    def _stack_intent(self, layers, dev):
        """``intent``: the k intent layers' weights and biases stacked, the rows padded with zeros to a multiple of 4 columns."""
        (D, kin), k = layers[0].weight.shape, len(layers)
        ldx, old = (kin + 3) // 4 * 4, self.intent.get('w')
        w = self.intent['w'] = self.buffer(old, (k * D, ldx), torch.float32, dev)
        b = self.intent['b'] = self.buffer(self.intent.get('b'), (k * D,), torch.float32, dev)
        if w is not old and ldx > kin:
            w[:, kin:].zero_()                                     # the pad columns: written once, the copies below stay left of them
        for i, lin in enumerate(layers):
            w[i * D:(i + 1) * D, :kin].copy_(lin.weight)
            b[i * D:(i + 1) * D].copy_(lin.bias)

    def _vocab_products(self, ent, table, pe, sa, nhead, want):
        """``ent['ew']`` / ``ent['pew']`` of one token encoder: the word table and the positions ``pe`` through the in_proj of ``sa``."""
        if want:
            (V, E), S, W = table.shape, pe.shape[0], nhead * 32
            w_in = ops.pad_heads(sa.in_proj_weight, 3 * nhead, E // nhead, 32)
            b_in = ops.pad_heads(sa.in_proj_bias, 3 * nhead, E // nhead, 32)
            ent['ew'] = ops.linear(table, w_in, None, out=self.buffer(ent.get('ew'), (V, 3 * W), torch.float32, table.device))
            ent['pew'] = ops.linear(pe, w_in, b_in, out=self.buffer(ent.get('pew'), (S, 3 * W), torch.float32, table.device))
        elif 'ew' in ent:
            del ent['ew'], ent['pew']
            self.let_go()

    def _packs(self, ent, layers, E, dev):
        """``ent['ffn']`` / ``ent['oproj']`` of one token encoder, per layer (None: a shape the split kernels do not cover)."""
        ffn, oproj = (ent.get(name) or [None] * len(layers) for name in ('ffn', 'oproj'))
        for li, layer in enumerate(layers):
            if _ffn_sp_shape(layer, E):
                sizes = ops.ffn_pack_sp_sizes(layer.linear1.weight.shape[0])
                out = tuple(self.buffer(old, (n,), torch.bfloat16, dev) for old, n in zip(ffn[li] or (None, None), sizes))
                ffn[li] = ops.ffn_pack_sp(layer.linear1.weight, layer.linear2.weight, out=out)
            else:
                ffn[li] = None
        for li, layer in enumerate(layers):
            if E <= 304 and E % 4 == 0:
                out = self.buffer(oproj[li], (ops.oproj_pack_sp_size(),), torch.bfloat16, dev)
                oproj[li] = ops.oproj_pack_sp(layer.self_attn.out_proj.weight, out=out)
            else:
                oproj[li] = None
        ent['ffn'], ent['oproj'] = ffn, oproj


class OccurrenceTables(kept.Kept):
    """``LIME.occurrence_tables()`` kept from one scoring call to the next: the tables are a handful of launches on 10- and 100-row
    operands that read weights only, and a scoring forward, every ``recommend*`` / ``score_*`` call and every candidate-table build
    asked for them anew.  Staleness, the in-place refresh and ``generation``: ``kept.Kept``."""

    T = Q = None

    def refresh(self, lime, config):
        """Compute the tables from ``lime``'s weights and copy them into the kept buffers, on the current stream."""
        T, Q = lime._compute_occurrence_tables()
        self.T = self.buffer(self.T, T.shape, T.dtype, T.device).copy_(T)
        self.Q = None if Q is None else self.buffer(self.Q, Q.shape, Q.dtype, Q.device).copy_(Q)


class CROWN(NewsEncoder):
    """newsEncoders.py:228-373: title/body transformer encoders, mean pooling, category-aware k-intent
    disentanglement, intent attention, title-body similarity, feature fusion.  -> [B, n, 900]."""

    def __init__(self, config):
        super().__init__(config)
        self.max_title_length = config.max_title_length
        self.max_body_length = config.max_abstract_length
        self.compute_dtype = getattr(config, 'compute_dtype', 'fp32')            # 'fp32' | 'bf16' (not a reference option)
        if self.compute_dtype not in ('fp32', 'bf16'):
            raise ValueError('compute_dtype must be fp32 or bf16')
        self.max_history_num = config.max_history_num
        self.category_embedding_dim = config.category_embedding_dim
        self.intent_embedding_dim = config.intent_embedding_dim
        self.category_embedding = nn.Embedding(config.category_num, config.category_embedding_dim)     # trainable again (:237)
        self.news_embedding_dim = config.intent_embedding_dim * 2 + config.category_embedding_dim + config.subCategory_embedding_dim
        self.head_num = config.head_num
        self.title_pos_encoder = PositionalEncoding(config.word_embedding_dim, config.dropout_rate, config.max_title_length)
        self.body_pos_encoder = PositionalEncoding(config.word_embedding_dim, config.dropout_rate, config.max_abstract_length)
        title_encoder_layers = TransformerEncoderLayer(config.word_embedding_dim, config.head_num, config.feedforward_dim,
                                                       config.dropout_rate, batch_first=True)
        self.title_transformer = TransformerEncoder(title_encoder_layers, config.num_layers)
        body_encoder_layers = TransformerEncoderLayer(config.word_embedding_dim, config.head_num, config.feedforward_dim,
                                                      config.dropout_rate, batch_first=True)
        self.body_transformer = TransformerEncoder(body_encoder_layers, config.num_layers)
        self.ISAB = ISAB(dim_in=config.word_embedding_dim, dim_out=config.word_embedding_dim, num_heads=config.isab_num_heads,
                         num_inds=config.isab_num_inds, ln=True)
        self.category_affine = nn.Linear(config.category_embedding_dim + config.subCategory_embedding_dim,
                                         config.category_embedding_dim)
        self.intent_num = config.intent_num
        self.alpha = config.alpha
        self.title_intent_attention = Attention(config.intent_embedding_dim, config.attention_dim)
        self.body_intent_attention = Attention(config.intent_embedding_dim, config.attention_dim)
        self.intent_layers = nn.ModuleList([nn.Linear(config.word_embedding_dim + config.category_embedding_dim,
                                                      config.intent_embedding_dim, bias=True) for _ in range(self.intent_num)])
        self.category_predictor = CategoryPredictor(config.intent_embedding_dim, config.category_num)

    def initialize(self):
        super().initialize()
        self.title_intent_attention.initialize()
        self.body_intent_attention.initialize()
        nn.init.xavier_uniform_(self.category_affine.weight)
        nn.init.zeros_(self.category_affine.bias)
        for intent_layer in self.intent_layers:
            nn.init.xavier_uniform_(intent_layer.weight)
            nn.init.zeros_(intent_layer.bias)
        nn.init.uniform_(self.category_embedding.weight, -0.1, 0.1)

    vocab_qkv_budget = 1 << 30     # bytes of [V, 3W] products a module may keep (both encoders: V <= 139k at 960 columns)

    def _product_sources(self):
        """Every tensor ``WeightProducts`` is computed from, in a fixed order."""
        src = [self.word_embedding.weight]
        for pos, tr in ((self.title_pos_encoder, self.title_transformer), (self.body_pos_encoder, self.body_transformer)):
            sa = tr.layers[0].self_attn
            src += [sa.in_proj_weight, sa.in_proj_bias, pos.pe]
            for layer in tr.layers:
                src += [layer.linear1.weight, layer.linear2.weight, layer.self_attn.out_proj.weight]
        for lin in self.intent_layers:
            src += [lin.weight, lin.bias]
        return src

    def weight_products(self, create=True):
        """The module's ``WeightProducts`` (``kept.current``), or None where the forward derives everything itself, in_proj included:
        the switch ``VOCAB_QKV`` off, bf16, the split product off, a CPU module, a capture over stale products.  ``create``: build
        them when the module has none yet -- what ``encode_flat`` asks for once it knows that a compacted call site takes them (they
        cost 2 V 960 floats and one GEMM over the vocabulary per encoder); ``kept_key`` passes False."""
        src = kept.kept_sources(self, '_product_paths', self._product_sources)           # (src[0]: the word table, without an attribute walk)
        if not VOCAB_QKV or self.compute_dtype == 'bf16' or not src[0].is_cuda or not ops.split_gemm_on():
            return None
        return kept.current(self, '_products', WeightProducts, src, (self.vocab_qkv_budget, WEIGHT_PREP_CACHE), create)

    def kept_key(self):
        return kept.key(self, '_products', self.weight_products)

    def _apply(self, fn, *args, **kwargs):
        kept.forget(self, '_products', '_product_paths')
        return super()._apply(fn, *args, **kwargs)

    def _step_of(self, S, M, bf16):
        """News per pass of a token encoder over sequences of S tokens."""
        E = self.word_embedding_dim
        return min(max(1, MAX_TOKENS_PER_PASS // S),
                   # the compacted in_proj scatters rows with 32-bit byte offsets from the base of qkv ([rows, 3 * 320])
                   max(1, (0x7FFFFFF0 // (3 * self.head_num * 32 * (2 if bf16 else 4))) // S - 2) if DEDUP else M,
                   # the fused bf16 entry points address a pass's rows with 32-bit byte offsets ([rows, 304] bf16)
                   max(1, (0x7FFFFFF0 // (((E + 7) // 8 * 8) * 2)) // S - 2) if bf16 else M)

    def _one_pass(self, title_text, content_text):
        """Both token encoders on the compacted fp32 path, one pass each."""
        M = title_text.shape[0]
        table = self.word_embedding.weight
        return (self.compute_dtype != 'bf16' and
                all(M <= self._step_of(ids.shape[1], M, False) and compact_applicable(ids, table, tr, self.head_num)
                    for ids, tr in ((title_text, self.title_transformer), (content_text, self.body_transformer))))

    def news_dedup_applicable(self, title_text, content_text):
        """The tail over the distinct news (``encode_flat(..., news=...)``) covers the one-pass compacted path, and the batches whose
        tail GEMMs the mid-M kernel takes with and without the compaction (2 (M + 1) < 4096 rows of intent input, k (M + 1) < 12288
        rows of intents): every computed row then keeps its kernel and its arithmetic."""
        M = title_text.shape[0]
        return (DEDUP and title_text.is_cuda and self._one_pass(title_text, content_text) and 2 * (M + 1) < 4096 and
                self.intent_num * (M + 1) < 12288)

    def encode_flat(self, title_text, title_mask, content_text, category, subCategory, out, content_mask=None, news=None,
                    buckets=None):
        """M news -> out [M, 900] (out may be a column slice of a wider buffer).  The token masks are computed and never
        used by the reference (:307-308); title_mask is accepted and ignored.
        ``news`` = ``ops.compact_batch(title_text, content_text, category, subCategory, ...)`` (``news_dedup_applicable`` batches only):
        the layers behind the token encoders run over the distinct news, and ``out`` is [M + 1, 900] in compact order -- row
        ``news[2].news_inv[i]`` is news i, rows at or beyond the device count ``news[2].n_news`` are not written.
        ``buckets`` = (num_buckets, cut points or None) with ``news``: the caller (LIME) wants the bucket pair of the compact keys; the
        launch that writes the topic rows leaves it in ``news[2].pair`` (``ops.news_keys``), valid on the caller's stream on return."""
        _no_train_dropout(self, self.dropout_rate)
        M, T = title_text.shape
        L = content_text.shape[1]
        if T != self.max_title_length or L != self.max_body_length:
            raise ValueError('token tensors must be [*, %d] / [*, %d]' % (self.max_title_length, self.max_body_length))
        E, Dc, D = self.word_embedding_dim, self.category_embedding_dim, self.intent_embedding_dim
        k = self.intent_num
        dev = title_text.device
        table = self.word_embedding.weight
        kin = E + Dc
        ldx = (kin + 3) // 4 * 4                                   # 352: keeps the rows 16-byte aligned
        dedup = news is not None
        if dedup:
            cmp_t, cmp_b, nw = news
            if not self.news_dedup_applicable(title_text, content_text) or nw.n != M or nw.count_mult != k:
                raise ValueError('news: the batch is outside news_dedup_applicable, or the lists are not this batch\'s (count_mult = intent_num)')
            category, subCategory = nw.cat_c, nw.sub_c             # the topic rows of the distinct news
        R = M + 1 if dedup else M                                  # rows per half of the tail: distinct news (capacity) or every slot
        if out.shape[0] != R:
            raise ValueError('out must have %d rows' % R)
        # rows [0, R): [title_pooled | category_rep], rows [R, 2R): [body_pooled | category_rep]   (:343-344)
        xin = torch.empty((2 * R, ldx), dtype=torch.float32, device=dev)
        # The title and body encoders are independent chains of five GEMM / attention launches each (optionally on two
        # streams, see SERIAL_STREAMS).
        bf16 = self.compute_dtype == 'bf16'
        if bf16:                                                   # the word table in bf16, rows padded to 8 columns
            table_b = ops.to_bf16(table, cols_out=(E + 7) // 8 * 8)
        main = torch.cuda.current_stream()
        encoders = ((title_text, self.title_pos_encoder, self.title_transformer, T),
                    (content_text, self.body_pos_encoder, self.body_transformer, L))
        step_of = lambda S: self._step_of(S, M, bf16)
        one_pass = self._one_pass(title_text, content_text)
        # what is kept across forwards (WeightProducts): built or refreshed here, in front of every branch, and only when a
        # compacted call site below takes it
        compacted = not bf16 and (one_pass or any(compact_applicable(ids[m0:min(M, m0 + step_of(S))], table, tr, self.head_num)
                                                   for ids, _, tr, S in encoders for m0 in range(0, M, step_of(S))))
        wp = self.weight_products() if compacted else None
        prods = [None, None] if wp is None else wp.encoder
        # branch 4: the category representation (:340-342) and the raw category / subCategory rows of feature_fusion (:221-225) -- they
        # depend on ids and weights only, and run beside the token encoders.  Over the distinct news for LIME (``buckets``) it is ONE
        # launch, ops.news_keys: the topic row into both halves of xin, the zeros of xin's pad columns and the bucket pair of the
        # compact keys.  Otherwise: topic_rep once per half and a fill.  The stacked intent weights come from the weight products; a
        # forward without them (bf16, a dense pass, a capture over stale products, the switches off) stacks them here.
        side4 = _side_stream(dev, 4)
        side4.wait_stream(main)
        with torch.cuda.stream(side4):
            if dedup:
                side4.wait_event(nw.ready)                         # the compact keys (unused slots hold id 0: valid over the capacity)
            sub_table = self.subCategory_embedding.weight
            emb_out = out[:, 2 * D:2 * D + Dc + sub_table.shape[1]]
            if dedup and buckets is not None:
                nw.pair = ops.news_keys(nw, buckets[0], buckets[1], self.category_embedding.weight, sub_table, self.category_affine.weight,
                                        self.category_affine.bias, xin, E, emb_out)
            else:
                ops.topic_rep(category, subCategory, self.category_embedding.weight, sub_table, self.category_affine.weight,
                              self.category_affine.bias, out=xin[:R, E:kin], emb_out=emb_out)
                ops.topic_rep(category, subCategory, self.category_embedding.weight, sub_table, self.category_affine.weight,
                              self.category_affine.bias, out=xin[R:, E:kin])
                if ldx > kin:
                    xin[:, kin:] = 0.0
            # the k intent weight matrices stacked row-wise, K = 350 carried as ldx = 352 zero-padded columns (16-byte rows: the
            # LDS-DMA GEMM kernels take it; the two pad columns of xin are zeroed to match)
            if wp is not None and wp.intent:
                w_int, b_int = wp.intent['w'], wp.intent['b']
            else:
                w_int = torch.nn.functional.pad(torch.cat([lin.weight for lin in self.intent_layers], dim=0), (0, ldx - kin))
                b_int = torch.cat([lin.bias for lin in self.intent_layers], dim=0)
        if one_pass:
            # both encoders on the compacted path in one pass each: the body's preparation (index lists, padded weights, padding
            # rows: a dozen short launches) runs on branch 3 under the title encoder's GEMMs
            (t_ids, t_pos, t_tr, _), (b_ids, b_pos, b_tr, _) = encoders
            side3 = _side_stream(dev, 3)
            side3.wait_stream(main)
            with torch.cuda.stream(side3):              # both encoders' preparation together: their small GEMMs share launches
                prep_t, prep_b = compact_prepare_many([(t_ids, t_pos.table(), t_tr), (b_ids, b_pos.table(), b_tr)], table, self.head_num,
                                                      cmps=(cmp_t, cmp_b) if dedup else None, products=prods)
            side1 = _side_stream(dev, 7)                   # branch 7: the (short) title chain beside the body chain
            side1.wait_stream(side3)
            with torch.cuda.stream(side1):
                tb = compact_run(prep_t, table, t_pos.table(), t_tr, self.head_num, None if dedup else xin[:M, :E], dedup)    # :311-317
            main.wait_stream(side3)
            bb = compact_run(prep_b, table, b_pos.table(), b_tr, self.head_num, None if dedup else xin[M:, :E], dedup)        # :312-321
            main.wait_stream(side1)
            if dedup:
                # the pooled rows of the distinct news straight from the compact block means: the rest of the body's mean and both
                # expansions through seq_inv in one launch (they were mean_pool + two gather_rows over all M slots)
                ops.news_xin(tb, T // 32, bb, L // 32, nw, xin, E)
        else:
            side = _side_stream(dev, 7 if DEDUP else 1)   # compacted chunks: title beside body (branch 7); dense: branch 1 (off)
            side.wait_stream(main)
            for half, (ids, pos, tr, S) in enumerate(encoders):
                step = step_of(S)
                with torch.cuda.stream(side if half == 0 else main):
                    shared = {}                                # packed weights of this encoder, for the passes of this forward
                    for m0 in range(0, M, step):
                        m1 = min(M, m0 + step)
                        if bf16:
                            if compact_applicable_bf16(ids[m0:m1], tr, self.head_num, E):
                                encode_tokens_bf16_compact(ids[m0:m1], table_b, pos.table(), tr, self.head_num,
                                                           xin[half * M + m0:half * M + m1, :E], shared=shared)
                            else:
                                encode_tokens_bf16(ids[m0:m1], table_b, pos.table(), tr, self.head_num, xin[half * M + m0:half * M + m1, :E])
                            continue
                        if compact_applicable(ids[m0:m1], table, tr, self.head_num):
                            encode_tokens_compact(ids[m0:m1], table, pos.table(), tr, self.head_num,
                                                  pooled_out=xin[half * M + m0:half * M + m1, :E], products=prods[half])
                            continue
                        encode_tokens(ids[m0:m1], table, pos.table(), tr, self.head_num,
                                      pooled_out=xin[half * M + m0:half * M + m1, :E])                                   # :311-321
            main.wait_stream(side)
        main.wait_stream(side4)
        # k intent layers (:284-295): [2M, 350] x [400, 350]^T each, ReLU fused, written side by side
        # (one GEMM against the k weight matrices stacked row-wise: the k layers share their input)
        if dedup:
            # one problem per half, each over its first n_news rows (device count): the tiles behind it exit at once
            intents = torch.empty((2 * R, w_int.shape[0]), dtype=torch.float32, device=dev)
            ops.linear_group([dict(a=xin[half * R:(half + 1) * R], w=w_int, bias=b_int, act='relu', out=intents[half * R:(half + 1) * R],
                                   m_dev=nw.n_news) for half in range(2)])
        else:
            intents = ops.linear(xin, w_int, b_int, act='relu')
        # intent attention (:355-356): tanh(affine1) on the GEMM (title on the main stream, body on branch 5), the rest in the fuse kernel
        A = self.title_intent_attention.affine1.out_features
        hidden = torch.empty((2 * R * k, A), dtype=torch.float32, device=dev)
        iv = intents.view(2 * R * k, D)
        rows_k = dict(m_dev=nw.n_news_mult) if dedup else {}                       # k rows of intents per news
        # the two halves do not depend on each other: one grouped launch (they were two launches on two streams)
        ops.linear_group([dict(a=iv[half * R * k:(half + 1) * R * k], w=att.affine1.weight, bias=att.affine1.bias, act='tanh',
                               out=hidden[half * R * k:(half + 1) * R * k], **rows_k)
                          for half, att in enumerate((self.title_intent_attention, self.body_intent_attention))])
        ops.intent_fuse(iv, hidden, self.title_intent_attention.affine2.weight.view(-1),
                        self.body_intent_attention.affine2.weight.view(-1), out, R, k, D, A,
                        m_dev=nw.n_news if dedup else None)                                           # :355-371
        return out


class MHSA(NewsEncoder):
    """newsEncoders.py:566-595: title-only multi-head self-attention + additive attention.  -> [B, n, 300]."""

    def _encode(self, ids, mask, out, compact):
        """Project -> attend -> tanh GEMM -> additive pool over the titles ``ids`` [n, T].  ``compact``: over the live sequences + ONE
        representative of the padding news' title (see ``encode_tokens_compact``; sequence level only: this encoder masks its padding
        tokens, so their rows are needed).  A sequence repeats the representative when its ids are all zero AND its mask is the padding
        news' mask (first position set, corpus.py:476-477); an all-zero sequence with any other mask counts as live."""
        n, T = ids.shape
        mha = self.multiheadAttention
        n_seq, rows, seqs, ids_r = n, {}, {}, ids.reshape(-1)
        if compact:
            if mask.dtype not in (torch.bool, torch.uint8):
                mask = mask.bool()
            mask = mask.contiguous()
            # all-zero ids under a mask that is not the padding news' mask: live (a sentinel in the first id); behind the compaction the
            # sentinel goes back to the padding word and the key mask is gathered into compact order -- two launches (they were ~18 torch ops)
            cmp = ops.compact_sequences(ops.mhsa_live_ids(ids, mask))
            mask = ops.mhsa_compact_mask(cmp, mask)
            n_seq, rows, seqs, ids_r = n + 1, dict(m_dev=cmp.n_rows), dict(n_seq_dev=cmp.n_compact), cmp.ids_c
        qkv = mha.project(table=self.word_embedding.weight, ids=ids_r, **rows)                          # :588 + layers.py:224-226
        c = mha.attend(qkv, n_seq, T, mask, **seqs)                                                     # layers.py:227-237
        hidden = ops.linear(c, self.attention.affine1.weight, self.attention.affine1.bias, act='tanh', **rows)
        pooled = ops.additive_pool(hidden, self.attention.affine2.weight.view(-1), c, n_seq, T, mask=mask, out=None if compact else out,
                                   **seqs)                                                              # :592
        if compact:
            ops.gather_rows(cmp.seq_inv, pooled, out)

    def _compact_applicable(self, ids, n, T):
        """The compacted title path rests on the device-count forms of the kernels, which are stricter than the dense ones:
        lime_linear_f32 with m_dev needs 16-byte friendly operands (K and N multiples of 4), lime_token_attention with a device count
        head_dim <= 32 and T <= 512.  Anything else takes the dense branch."""
        mha = self.multiheadAttention
        return (DEDUP and (n + 1) * T >= 4096 and ids.dtype == torch.int32 and ids.is_contiguous() and mha.d_model % 4 == 0 and
                (3 * mha.h * mha.d_k) % 4 == 0 and mha.d_k <= 32 and mha.d_v <= 32 and T <= 512)

    def __init__(self, config):
        super().__init__(config)
        self.max_sentence_length = config.max_title_length
        self.feature_dim = config.head_num * config.head_dim
        self.multiheadAttention = MultiHeadAttention(config.head_num, config.word_embedding_dim, config.max_title_length,
                                                     config.max_title_length, config.head_dim, config.head_dim)
        self.attention = Attention(config.head_num * config.head_dim, config.attention_dim)
        self.news_embedding_dim = config.head_num * config.head_dim + config.category_embedding_dim + config.subCategory_embedding_dim
        self.category_embedding = nn.Embedding(config.category_num, config.category_embedding_dim)

    def initialize(self):
        super().initialize()
        self.multiheadAttention.initialize()
        self.attention.initialize()
        nn.init.uniform_(self.category_embedding.weight, -0.1, 0.1)

    def encode_flat(self, title_text, title_mask, content_text, category, subCategory, out, content_mask=None):
        _no_train_dropout(self, self.dropout_rate)
        M, T = title_text.shape
        F = self.feature_dim
        mask = title_mask.contiguous()
        step = max(1, MAX_TOKENS_PER_PASS // T)
        for m0 in range(0, M, step):
            m1 = min(M, m0 + step)
            ids = title_text[m0:m1]
            self._encode(ids, mask[m0:m1], out[m0:m1, :F], self._compact_applicable(ids, m1 - m0, T))
        ops.topic_rep(category, subCategory, self.category_embedding.weight, self.subCategory_embedding.weight,
                      emb_out=out[:, F:])                                                               # :594
        return out


_ROW_COUNTS = {}


def _row_count(n, device):
    """A device int32 holding n (the m_dev of a dense pass), one per (device, n), never written after its creation."""
    key = (device.type, device.index, n)
    t = _ROW_COUNTS.get(key)
    if t is None:
        t = _ROW_COUNTS[key] = torch.full((1,), n, dtype=torch.int32, device=device)
    return t


class CNN(NewsEncoder):
    """newsEncoders.py:535-563: title-only 1-D convolution (layers.py:98-135, ReLU) + additive attention.  -> [B, n, cnn_kernel_num + 100].

    The convolution is the windowed conv GEMM (csrc/conv_sp_f32.hip): word rows gathered straight into its A operand, zeros beyond the
    title's ends, bias + ReLU in the epilogue, the group3 convolutions writing their column slices of one output."""

    def __init__(self, config):
        super().__init__(config)
        if getattr(config, 'compute_dtype', 'fp32') != 'fp32':
            raise NotImplementedError("compute_dtype %r: the CNN content encoder is built for fp32 (compute_dtype='fp32')" % config.compute_dtype)
        self.max_sentence_length = config.max_title_length
        self.cnn_kernel_num = config.cnn_kernel_num
        self.conv = Conv1D(config.cnn_method, config.word_embedding_dim, config.cnn_kernel_num, config.cnn_window_size)
        self.attention = Attention(config.cnn_kernel_num, config.attention_dim)
        self.news_embedding_dim = config.cnn_kernel_num + config.category_embedding_dim + config.subCategory_embedding_dim
        self.category_embedding = nn.Embedding(config.category_num, config.category_embedding_dim)     # trainable (re-created)
        nn.init.uniform_(self.category_embedding.weight, -0.1, 0.1)

    def initialize(self):
        super().initialize()
        self.attention.initialize()

    def _compact_applicable(self, ids):
        return (DEDUP and ids.dtype == torch.int32 and ids.is_contiguous() and self.cnn_kernel_num % 4 == 0 and
                self.attention.affine1.out_features % 4 == 0)

    def _encode(self, ids, mask, out, compact):
        """One pass over n titles.  Both forms run every GEMM with the SAME capacity ((n + 1) T rows) and a device row count, so the
        dispatcher picks the same kernels and a title's representation has the same bits whether it went through the compacted or the
        dense form (the conv kernel computes a row the same way whatever the row count)."""
        n, T = ids.shape
        dev = ids.device
        K, A = self.cnn_kernel_num, self.attention.affine1.out_features
        cap = (n + 1) * T
        c = torch.empty((cap, K), dtype=torch.float32, device=dev)
        hidden = torch.empty((cap, A), dtype=torch.float32, device=dev)
        table = self.word_embedding.weight
        a2 = self.attention.affine2.weight.view(-1)
        if compact:
            # the live titles + ONE representative of the padding news' title (ids all zero AND the padding news' mask); an all-zero title
            # under another mask is live (MHSA._encode_compact)
            cmp = ops.compact_sequences(ops.mhsa_live_ids(ids, mask))
            mask_c = ops.mhsa_compact_mask(cmp, mask)
            self.conv.relu_into(table, T, c, ids=cmp.ids_c, m_dev=cmp.n_rows)                                         # :556
            ops.linear(c, self.attention.affine1.weight, self.attention.affine1.bias, act='tanh', m_dev=cmp.n_rows, out=hidden)
            pooled_c = ops.additive_pool(hidden, a2, c, n + 1, T, mask=mask_c, n_seq_dev=cmp.n_compact)                  # :558
            ops.gather_rows(cmp.seq_inv, pooled_c, out)
            return
        self.conv.relu_into(table, T, c[:n * T], ids=ids.reshape(-1))                                                   # :556
        ops.linear(c, self.attention.affine1.weight, self.attention.affine1.bias, act='tanh', m_dev=_row_count(n * T, dev), out=hidden)
        ops.additive_pool(hidden[:n * T], a2, c[:n * T], n, T, mask=mask, out=out)                                      # :558

    def encode_flat(self, title_text, title_mask, content_text, category, subCategory, out, content_mask=None):
        _no_train_dropout(self, self.dropout_rate)
        M, T = title_text.shape
        K = self.cnn_kernel_num
        mask = title_mask if title_mask.dtype in (torch.bool, torch.uint8) else title_mask.bool()
        mask = mask.contiguous()
        ids = _i32(title_text).contiguous()
        step = max(1, MAX_TOKENS_PER_PASS // T)
        for m0 in range(0, M, step):
            m1 = min(M, m0 + step)
            self._encode(ids[m0:m1], mask[m0:m1], out[m0:m1, :K], self._compact_applicable(ids))
        ops.topic_rep(category, subCategory, self.category_embedding.weight, self.subCategory_embedding.weight,
                      emb_out=out[:, K:])                                                                               # :561
        return out


class KCNN(NewsEncoder):
    """newsEncoders.py:598-638: DKN's knowledge-aware CNN over the title -- per token the word row, tanh(M_entity(entity row)) and
    tanh(M_context(context row)) side by side, Conv2D_Pool (layers.py:138-190: convolution over the three, ReLU, maximum over the pooled
    positions), then feature_fusion with the encoder's own trainable category table.  -> [B, n, cnn_kernel_num + 100].  No mask, no
    dropout in front of the convolution: padding tokens take part (:630-633).

    ``entity_embedding`` / ``context_embedding`` are filled by the caller (``load_state_dict`` or ``.weight.data.copy_``) as the word
    table is; the reference unpickles them from the cwd (:607-610).

    The convolution, ReLU and pooling are ops.conv_pool (csrc/conv_pool_sp_f32.hip): the word rows are gathered straight into its A
    operand by word id.  The two transforms take whichever has fewer rows: a [entity_size, C] table tanh(E M^T + b) per forward, gathered
    inside the kernel by entity id, or one row per token through the GEMM's own gather (ops.linear(a_ids=...))."""

    reads_title_entity = True

    def __init__(self, config):
        super().__init__(config)
        if getattr(config, 'compute_dtype', 'fp32') != 'fp32':
            raise NotImplementedError("compute_dtype %r: the KCNN content encoder is built for fp32 (compute_dtype='fp32')" % config.compute_dtype)
        self.max_title_length = config.max_title_length
        self.cnn_kernel_num = config.cnn_kernel_num
        self.entity_embedding_dim = config.entity_embedding_dim
        self.context_embedding_dim = config.context_embedding_dim
        self.entity_embedding = nn.Embedding(num_embeddings=config.entity_size, embedding_dim=self.entity_embedding_dim)
        self.context_embedding = nn.Embedding(num_embeddings=config.entity_size, embedding_dim=self.context_embedding_dim)
        self.M_entity = LinearHolder(self.entity_embedding_dim, self.word_embedding_dim, bias=True)
        self.M_context = LinearHolder(self.context_embedding_dim, self.word_embedding_dim, bias=True)
        self.knowledge_cnn = Conv2D_Pool(config.cnn_method, config.word_embedding_dim, config.cnn_kernel_num, config.cnn_window_size, 3)
        if config.max_title_length < self.knowledge_cnn.max_window():
            raise ValueError('max_title_length %d is smaller than the largest convolution window %d: no position is left to pool '
                             '(layers.py:169-189)' % (config.max_title_length, self.knowledge_cnn.max_window()))
        if self.entity_embedding_dim % 4 or self.context_embedding_dim % 4:
            raise NotImplementedError('the entity / context tables must be a multiple of 4 wide')
        self.news_embedding_dim = config.cnn_kernel_num + config.category_embedding_dim + config.subCategory_embedding_dim
        self.category_embedding = nn.Embedding(config.category_num, config.category_embedding_dim)     # trainable (re-created, :615)

    def initialize(self):                                                                              # :617-623
        super().initialize()
        nn.init.xavier_uniform_(self.M_entity.weight, gain=nn.init.calculate_gain('tanh'))
        nn.init.zeros_(self.M_entity.bias)
        nn.init.xavier_uniform_(self.M_context.weight, gain=nn.init.calculate_gain('tanh'))
        nn.init.zeros_(self.M_context.bias)
        nn.init.uniform_(self.category_embedding.weight, -0.1, 0.1)

    def sources(self, word_ids, entity_ids):
        """The three (a, ids) sources of ops.conv_pool for the flat int32 word / entity ids of the tokens (:630-633)."""
        n_tok = word_ids.numel()
        src = [(self.word_embedding.weight, word_ids)]
        for table, lin in ((self.entity_embedding.weight, self.M_entity), (self.context_embedding.weight, self.M_context)):
            if table.shape[0] <= n_tok:
                src.append((ops.linear(table, lin.weight, lin.bias, act='tanh'), entity_ids))
            else:
                src.append((ops.linear(table, lin.weight, lin.bias, act='tanh', a_ids=entity_ids), None))
        return src

    def conv_pool_into(self, src, T, out, fused=None):
        """Conv2D_Pool over the sources' sequences of T tokens -> out [n, cnn_kernel_num] (the group convolutions write column slices)."""
        for conv, col, w, p, P in self.knowledge_cnn.convs(T):
            ops.conv_pool(src, ops.conv_pool_pack(conv.weight), w, p, P, T, bias=conv.bias, out=out[:, col:col + conv.out_channels],
                          fused=fused)
        return out

    def encode_flat(self, title_text, title_mask, content_text, category, subCategory, out, content_mask=None, title_entity=None):
        _no_train_dropout(self, self.dropout_rate)
        if title_entity is None:
            raise TypeError('the KCNN content encoder reads the title entity ids (title_entity): the ids are never guessed')
        M, T = title_text.shape
        if tuple(title_entity.shape) != (M, T):
            raise ValueError('title_entity must be [%d, %d] like title_text, got %s' % (M, T, tuple(title_entity.shape)))
        if T < self.knowledge_cnn.max_window():
            raise ValueError('titles of %d tokens are shorter than the largest convolution window %d' % (T, self.knowledge_cnn.max_window()))
        K = self.cnn_kernel_num
        ids = _i32(title_text).contiguous()
        ent = _i32(title_entity).contiguous()
        step = max(1, MAX_TOKENS_PER_PASS // T)
        for m0 in range(0, M, step):
            m1 = min(M, m0 + step)
            self.conv_pool_into(self.sources(ids[m0:m1].reshape(-1), ent[m0:m1].reshape(-1)), T, out[m0:m1, :K])   # :630-635
        ops.topic_rep(category, subCategory, self.category_embedding.weight, self.subCategory_embedding.weight,
                      emb_out=out[:, K:])                                                                           # :637
        return out


class NAML(NewsEncoder):
    """newsEncoders.py:641-695: title and body each through a 1-D convolution (layers.py:98-135, ReLU) and an additive attention, two
    category views (Linear 50 -> cnn_kernel_num + ReLU), and an additive attention over the four views -> [B, n, cnn_kernel_num].

    The convolutions are the windowed conv GEMM (csrc/conv_sp_f32.hip); the three attentions are the fused attention pool
    (csrc/attn_pool_sp_f32.hip: tanh(affine1), the score, the softmax and the weighted sum in one launch, the hidden state in registers)
    when ops.FUSED_ATTN_POOL asks for it, else linear(tanh) + additive_pool: on MI355X the fused launch is the slower one today.
    Reference behaviour kept: the word attentions take NO mask (:686-687: padding positions take part in the softmax; title_mask and
    content_mask are not read), no feature_fusion (the content dimension is cnn_kernel_num, :647), the view attention is a softmax
    over the stack [title, body, category, subcategory] (:692-694)."""

    def __init__(self, config):
        super().__init__(config)
        if getattr(config, 'compute_dtype', 'fp32') != 'fp32':
            raise NotImplementedError("compute_dtype %r: the NAML content encoder is built for fp32 (compute_dtype='fp32')" % config.compute_dtype)
        self.max_title_length = config.max_title_length
        self.max_content_length = config.max_abstract_length
        self.cnn_kernel_num = config.cnn_kernel_num
        self.news_embedding_dim = config.cnn_kernel_num                                                 # :647
        self.title_conv = Conv1D(config.cnn_method, config.word_embedding_dim, config.cnn_kernel_num, config.cnn_window_size)
        self.content_conv = Conv1D(config.cnn_method, config.word_embedding_dim, config.cnn_kernel_num, config.cnn_window_size)
        self.title_attention = Attention(config.cnn_kernel_num, config.attention_dim)
        self.content_attention = Attention(config.cnn_kernel_num, config.attention_dim)
        self.category_affine = nn.Linear(config.category_embedding_dim, config.cnn_kernel_num, bias=True)
        self.subCategory_affine = nn.Linear(config.subCategory_embedding_dim, config.cnn_kernel_num, bias=True)
        self.affine1 = nn.Linear(config.cnn_kernel_num, config.attention_dim, bias=True)
        self.affine2 = nn.Linear(config.attention_dim, 1, bias=False)
        self.category_embedding = nn.Embedding(config.category_num, config.category_embedding_dim)     # trainable (re-created, :656)

    def initialize(self):                                                                               # :658-669
        super().initialize()
        self.title_attention.initialize()
        self.content_attention.initialize()
        nn.init.xavier_uniform_(self.category_affine.weight)
        nn.init.zeros_(self.category_affine.bias)
        nn.init.xavier_uniform_(self.subCategory_affine.weight)
        nn.init.zeros_(self.subCategory_affine.bias)
        nn.init.xavier_uniform_(self.affine1.weight)
        nn.init.zeros_(self.affine1.bias)
        nn.init.xavier_uniform_(self.affine2.weight)
        nn.init.uniform_(self.category_embedding.weight, -0.1, 0.1)

    def _compact_applicable(self, ids):
        return DEDUP and ids.dtype == torch.int32 and ids.is_contiguous()

    def _encode_text(self, ids, conv, att, w1p, out, compact):
        """One pass over n texts (title or body): conv + the unmasked attention pool (:683-687) -> out [n, cnn_kernel_num] (a view slot).

        Both forms run every launch with the SAME capacity ((n + 1) sequences of T rows) and a device count, so the dispatcher picks the
        same kernels and a text's representation has the same bits whether it went through the compacted or the dense form (the conv
        kernel computes a row, the attention pool a sequence, the same way whatever the counts).  Compacted: the live texts (any non-zero
        id; NAML reads no mask) and ONE representative of the all-padding ones."""
        n, T = ids.shape
        dev = ids.device
        K = self.cnn_kernel_num
        cap = (n + 1) * T
        c = torch.empty((cap, K), dtype=torch.float32, device=dev)
        pooled = torch.empty((n + 1, K), dtype=torch.float32, device=dev)
        table = self.word_embedding.weight
        a1, a2 = att.affine1, att.affine2.weight.view(-1)
        if compact:
            cmp = ops.compact_sequences(ids)
            conv.relu_into(table, T, c, ids=cmp.ids_c, m_dev=cmp.n_rows)                                              # :681, :684
            ops.attn_pool(c, a1.weight, a1.bias, a2, n + 1, T, out=pooled, n_seq_dev=cmp.n_compact, w1p=w1p,
                          m_dev=cmp.n_rows)                                                                            # :686-687
            ops.gather_rows(cmp.seq_inv, pooled, out)
            return
        conv.relu_into(table, T, c[:n * T], ids=ids.reshape(-1))                                                       # :681, :684
        ops.attn_pool(c, a1.weight, a1.bias, a2, n + 1, T, out=pooled, n_seq_dev=_row_count(n, dev), w1p=w1p,
                      m_dev=_row_count(n * T, dev))                                                                    # :686-687
        ops.gather_rows(_identity_rows(n, dev), pooled, out)

    def encode_flat(self, title_text, title_mask, content_text, category, subCategory, out, content_mask=None):
        _no_train_dropout(self, self.dropout_rate)
        M, T = title_text.shape
        L = content_text.shape[1]
        K = self.cnn_kernel_num
        dev = title_text.device
        t_ids = _i32(title_text).contiguous()
        b_ids = _i32(content_text).contiguous()
        fused = ops.attn_pool_fused
        # the attention pools (ops.attn_pool: the fused launch where ops.FUSED_ATTN_POOL asks for it, else linear(tanh) + additive_pool);
        # W1 of a fused one split into its bf16 terms HERE (inside the forward: a captured graph repacks on every replay)
        w1p = [ops.attn_pool_pack(a.affine1.weight) if fused(K, a.affine1.out_features, t) else None
               for a, t in ((self.title_attention, T), (self.content_attention, L), (self, 4))]
        views = torch.empty((M, 4, K), dtype=torch.float32, device=dev)                                     # :692 stack
        step = max(1, MAX_TOKENS_PER_PASS // max(T, L))
        compact = self._compact_applicable(t_ids) and self._compact_applicable(b_ids)
        for m0 in range(0, M, step):
            m1 = min(M, m0 + step)
            self._encode_text(t_ids[m0:m1], self.title_conv, self.title_attention, w1p[0], views[m0:m1, 0], compact)
            self._encode_text(b_ids[m0:m1], self.content_conv, self.content_attention, w1p[1], views[m0:m1, 1], compact)
        ops.linear(self.category_embedding.weight, self.category_affine.weight, self.category_affine.bias, act='relu',
                   a_ids=_i32(category).reshape(-1).contiguous(), out=views[:, 2])                               # :689
        ops.linear(self.subCategory_embedding.weight, self.subCategory_affine.weight, self.subCategory_affine.bias, act='relu',
                   a_ids=_i32(subCategory).reshape(-1).contiguous(), out=views[:, 3])                            # :690
        ops.attn_pool(views.view(M * 4, K), self.affine1.weight, self.affine1.bias, self.affine2.weight.view(-1), M, 4, out=out,
                      w1p=w1p[2])                                                                                # :692-694
        return out


_ONES = {}


def _ones(n, device):
    """n ones (fp32), allocated once per device and never written."""
    return _grown(_ONES, n, device, 1024, lambda size: torch.ones(size, dtype=torch.float32, device=device))


class CNERecurrenceCache:
    """What CNE's recurrence leaves per news (CNE.build_recurrence_cache): a plain object, neither a buffer nor a parameter of the module
    (``state_dict()`` does not know it).  Per text (``title``, ``body``), with n news, S token slots and C = 2 hidden_dim:

        S        the token slots of the text (the width of its masks)
        lens     int32 [n]          the sum of the mask after the slot-0 rule (>= 1)
        offsets  int64 [n + 1]      the exclusive prefix sum of lens: news i owns the packed rows offsets[i] .. offsets[i + 1] - 1
        h        fp32 [sum(lens), C]  the LSTM output of the live tokens (slots 0 .. len - 1 of each news, in order)
        hh       fp32 [sum(lens), C]  h . H^T, the hidden-state half of the gate's pre-activation (no bias, no memory term)
        m        fp32 [n, C]        the memory vector cat(c_n forward, c_n backward)

    PACKED, not dense: a dense cache holds every token slot, (32 + 128) slots x 2 tensors x 800 floats = 1 MB per news at the defaults;
    packed it is 2 tensors x 800 floats = 6.4 KB per LIVE token.  ``nbytes`` (``packed_nbytes``), per text:
        2 . sum(lens) . C . 4  +  n . C . 4  +  n . 4  +  (n + 1) . 8.

    ``versions``: the ``_version`` counters of the parameters the cache was built from (word table, both LSTMs, title_H, content_H).
    They move with autograd-visible in-place updates (``load_state_dict``, torch optimizers) but NOT with edits through ``.data`` nor
    with the native Adam step, which writes the flat parameter bucket directly; ``fingerprint`` (int64 device tensor: the sum of each
    parameter's bit patterns) catches those.  ``CNE.cache_is_current`` compares both (another rule than ``kept.weight_state``, which
    needs such a write announced: this cache is the caller's, not the module's)."""

    Text = collections.namedtuple('Text', 'S lens offsets h hh m')

    def __init__(self, title, body, versions, fingerprint):
        self.title, self.body, self.versions, self.fingerprint = title, body, versions, fingerprint
        self.n_news = title.lens.numel()
        self.nbytes = sum(t.numel() * t.element_size() for text in (title, body) for t in text[1:])

    @staticmethod
    def packed_nbytes(lens_title, lens_body, hidden_dim):
        """``nbytes`` of a cache over news with these title and body lengths (the formula of the class docstring)."""
        C = 2 * hidden_dim
        return sum(2 * sum(lens) * C * 4 + len(lens) * C * 4 + len(lens) * 4 + (len(lens) + 1) * 8 for lens in (lens_title, lens_body))


class CNE(NewsEncoder):
    """newsEncoders.py:439-532, the collaborative news encoder of CNE-SUE: title and body each through a bidirectional LSTM, cross-selective
    gates (each text's LSTM output gated by the OTHER text's memory vector), a masked additive self attention and a scaled-dot-product
    cross attention whose query is the other text's self-attention output.  -> [B, n, 4 hidden_dim + 100].

    The recurrence is the LSTM step kernel (csrc/lstm_f32.hip, ops.lstm): the input projection of every token and both directions is
    one GEMM with the word rows gathered into its A operand, then one launch per time step.  The gates are a GEMM with the memory term
    as a broadcast residual and ops.gate_mul; the attentions are linear(tanh) / gate_mul + additive_pool.

    Reference behaviour kept:
      * mask slot 0 (:492-493): title_mask[:, 0] = content_mask[:, 0] = 1, so every length is >= 1 and an all-padding text runs one
        step on word row 0.  Applied to COPIES here; the reference edits the caller's tensors in place.
      * lengths and masks (:494-495, :503-504, :524-528): the length is the SUM of the mask, the LSTM runs over the FIRST `length` token
        slots (pack_padded_sequence), the attentions mask by the mask's own positions.  The two agree for prefix masks.
      * h is zero behind the length (pad_packed_sequence, :514-515); the memory vector is cat(c_n forward, c_n backward) (:512-513).
      * each gate reads the other text's memory vector (:517-518), each cross attention the other text's self attention (:527-528).
      * WHICH news' memory vector a gate reads (:496-499, :517-521): the reference sorts the titles by title length and the bodies by
        body length, each for its own pack_padded_sequence, and applies the gates in SORTED order before it undoes the sorts -- the
        title at sorted position j is gated by the body memory at sorted position j, which belongs to another news unless the two
        orders agree.  The partner of a news therefore depends on every length in the call.  ``pair_groups`` (the news counts of the
        reference's calls: candidates, history) reproduces it, TIED lengths in input order (the reference leaves their order to the torch build)
        (``reference_pairs``; the goldens pin it).  ``encode_flat`` without ``pair_groups`` gives the encoder as published: every news
        reads its OWN other text's memory vector.  A paired pass shares nothing between news, so CNE has no compacted form.
      * category_embedding is re-created (:447) and trains; subCategory_embedding stays frozen.
      * dropout acts on both word-embedding gathers (:501-502) and in feature_fusion (training path: training.cne_content).

    The body mask is required: a missing one raises TypeError (it is never guessed from the ids).  hidden_dim must be a multiple of 16
    (ops.LSTM_UNIT_TILE: a workgroup of the step kernel owns 16 hidden units with their four gates); fp32 only.

    Memory: gi is 2 . 4 hidden_dim floats per token (12.8 KB at hidden_dim 400; MAX_TOKENS_PER_PASS would allow 51 GB), so the recurrence
    runs in chunks of news whose gi stays within GI_BYTES_PER_PASS (``lstm_chunks``).  hout and c_n of all chunks are kept (2 hidden_dim
    floats per token), and the gates pair over the whole call: a call has no size limit but memory.

    Evaluation can take the recurrence from a per-news cache: lengths, LSTM outputs, H h_t and memory vectors depend on the news alone
    (``build_recurrence_cache`` -> CNERecurrenceCache), the partners on the call (``encode_cached_flat``: pairing, M m_partner + b, one
    gate launch from the packed rows, then the same attentions)."""

    GI_BYTES_PER_PASS = 4 << 30
    reads_content_mask = True

    def __init__(self, config):
        super().__init__(config)
        if getattr(config, 'compute_dtype', 'fp32') != 'fp32':
            raise NotImplementedError("compute_dtype %r: the CNE content encoder is built for fp32 (compute_dtype='fp32')" % config.compute_dtype)
        h = config.hidden_dim
        if h <= 0 or h % ops.LSTM_UNIT_TILE:
            raise NotImplementedError('hidden_dim %d: the LSTM step kernel is built for multiples of %d' % (h, ops.LSTM_UNIT_TILE))
        if config.word_embedding_dim % 4 or config.attention_dim % 4:
            raise NotImplementedError('the CNE encoder needs multiples of 4 for word_embedding_dim and attention_dim')
        self.max_title_length = config.max_title_length
        self.max_content_length = config.max_abstract_length
        self.hidden_dim = h
        self.news_embedding_dim = 4 * h + config.category_embedding_dim + config.subCategory_embedding_dim          # :446
        self.category_embedding = nn.Embedding(config.category_num, config.category_embedding_dim)                  # trainable (re-created, :447)
        E = config.word_embedding_dim
        self.title_lstm = LSTMHolder(E, h, batch_first=True, bidirectional=True)
        self.content_lstm = LSTMHolder(E, h, batch_first=True, bidirectional=True)
        self.title_H = LinearHolder(2 * h, 2 * h, bias=False)
        self.title_M = LinearHolder(2 * h, 2 * h, bias=True)
        self.content_H = LinearHolder(2 * h, 2 * h, bias=False)
        self.content_M = LinearHolder(2 * h, 2 * h, bias=True)
        self.title_self_attention = Attention(2 * h, config.attention_dim)
        self.content_self_attention = Attention(2 * h, config.attention_dim)
        self.title_cross_attention = ScaledDotProduct_CandidateAttention(2 * h, 2 * h, config.attention_dim)
        self.content_cross_attention = ScaledDotProduct_CandidateAttention(2 * h, 2 * h, config.attention_dim)

    def initialize(self):                                                                                           # :462-484
        super().initialize()
        for lstm in (self.title_lstm, self.content_lstm):
            for p in lstm.parameters():
                if p.dim() >= 2:
                    nn.init.orthogonal_(p.data)
                else:
                    nn.init.zeros_(p.data)
        gain = nn.init.calculate_gain('sigmoid')
        for lin in (self.title_H, self.title_M, self.content_H, self.content_M):
            nn.init.xavier_uniform_(lin.weight, gain=gain)
        nn.init.zeros_(self.title_M.bias)
        nn.init.zeros_(self.content_M.bias)
        for att in (self.title_self_attention, self.content_self_attention, self.title_cross_attention, self.content_cross_attention):
            att.initialize()
        nn.init.uniform_(self.category_embedding.weight, -0.1, 0.1)

    @staticmethod
    def lstm_weights(lstm):
        """(W_ih of both directions stacked row-wise [8h, E], b_ih + b_hh stacked [8h], W_hh stacked [2, 4h, h])."""
        wih = torch.cat([lstm.weight_ih_l0, lstm.weight_ih_l0_reverse], dim=0)
        bias = torch.cat([lstm.bias_ih_l0 + lstm.bias_hh_l0, lstm.bias_ih_l0_reverse + lstm.bias_hh_l0_reverse], dim=0)
        whh = torch.stack([lstm.weight_hh_l0, lstm.weight_hh_l0_reverse], dim=0)
        return wih, bias, whh

    @staticmethod
    def reference_pairs(lens_t, lens_b, groups, cap):
        """(int32 [cap], int32 [cap]): the news whose body memory gates the title of news i, and whose title memory gates its body, for
        calls of ``groups`` news each (:496-499, :517-521): sorted position j of the one order meets sorted position j of the other.
        Sorted = descending by length, TIED lengths in input order (a stable sort: the reference's default sort leaves the order of
        ties to the torch build, so it is defined here; tools/make_cne_goldens.py runs the reference the same way).

        ``groups``: the news counts of the calls (a list: consecutive ranges), or an int64 device tensor with the call number of every
        news (what a caller with hundreds of calls computes by arithmetic, Model.score_behaviors; the news of a call need not be
        adjacent, their order within the call is their input order).  Device-side and TWO stable sorts whatever the number of calls: the
        key call . 2^32 - length orders a text by call, then by descending length, and both texts have the same calls at the same sorted
        positions, so the two orders meet position by position inside every call.  A list costs one slice fill per call behind the
        first; slots behind the groups pair with themselves."""
        dev = lens_t.device
        if isinstance(groups, torch.Tensor):
            gid = groups
        else:
            gid = torch.zeros(sum(groups), dtype=torch.int64, device=dev)
            o = 0
            for g, n in enumerate(groups):
                if g:
                    gid[o:o + n] = g
                o += n
        total = gid.numel()
        pt, pb = torch.arange(cap, device=dev), torch.arange(cap, device=dev)
        st = torch.sort((gid << 32) - lens_t[:total], stable=True).indices
        sc = torch.sort((gid << 32) - lens_b[:total], stable=True).indices
        pt[st] = sc                                                # title at sorted position p <- body memory at sorted position p
        pb[sc] = st
        return pt.to(torch.int32), pb.to(torch.int32)

    @staticmethod
    def slot0_mask(mask):
        """A uint8 COPY of the mask with slot 0 set (:492-493)."""
        m = mask.to(torch.uint8) if mask.dtype != torch.bool else mask.view(torch.uint8).clone()
        if m.data_ptr() == mask.data_ptr():
            m = m.clone()
        m[:, 0] = 1
        return m.contiguous()

    def lstm_chunks(self, n_news, S):
        """[(first, end)] news ranges of the recurrence over n_news texts of S token slots: as few as keep a chunk's gi ([tokens,
        2 . 4 hidden_dim] fp32) within GI_BYTES_PER_PASS, of even size.  Only gi is per chunk; hout and c_n of every chunk are kept, so
        the gates pair over the whole call whatever its size."""
        per = max(1, self.GI_BYTES_PER_PASS // (S * 8 * self.hidden_dim * 4))
        n_chunks = max(1, -(-n_news // per))
        size = -(-n_news // n_chunks)
        return [(r0, min(n_news, r0 + size)) for r0 in range(0, n_news, size)]

    def _encode(self, ids_t, mask_t, ids_b, mask_b, n_dev, pooled, pair_groups=None):
        """`cap` news slots of which the first n_dev (a device int) are live: title ids_t [cap, T] / body ids_b [cap, L] int32, masks uint8
        with slot 0 set -> pooled [cap, 4h] (rows behind n_dev are left alone).  Every launch has the capacity as its shape and the device
        count as its bound."""
        dev = ids_t.device
        cap, h = ids_t.shape[0], self.hidden_dim
        table = self.word_embedding.weight
        texts = []
        for ids, mask, lstm in ((ids_t, mask_t, self.title_lstm), (ids_b, mask_b, self.content_lstm)):
            S = ids.shape[1]
            n_tok = n_dev * S                                                                          # device int: live token rows
            lens = ops.mask_lengths(mask, min_len=1)                                                   # :494-495
            wih, bias, whh = self.lstm_weights(lstm)
            hout = torch.zeros((cap * S, 2 * h), dtype=torch.float32, device=dev)
            m = torch.empty((cap, 2 * h), dtype=torch.float32, device=dev)
            for r0, r1 in self.lstm_chunks(cap, S):
                live = n_dev if r0 == 0 else (n_dev - r0).clamp(min=0)                                 # live news of this chunk
                gi = ops.linear(table, wih, bias, a_ids=ids[r0:r1].reshape(-1), m_dev=live * S)        # :501-502 gather + W_ih x + b
                _, c = ops.lstm(gi, whh, lens[r0:r1], S, n_rows_dev=live, hout=hout[r0 * S:r1 * S])    # :509-510, :514-515
                del gi
                m[r0:r1] = c.transpose(0, 1).reshape(r1 - r0, 2 * h)                                   # :512-513
            texts.append((S, n_tok, mask, hout, m, lens))
        pairs = None
        if pair_groups is not None:
            pairs = self.reference_pairs(texts[0][5], texts[1][5], pair_groups, cap)
        gated = []
        for k, (H_, M_) in enumerate(((self.title_H, self.title_M), (self.content_H, self.content_M))):
            S, n_tok, _, hout, _, _ = texts[k]
            m_other = texts[1 - k][4]
            if pairs is not None:                                                                      # the reference's partner news
                m_other = ops.gather_rows(pairs[k], m_other, torch.empty_like(m_other))
            tm = ops.linear(m_other, M_.weight, M_.bias, m_dev=n_dev)                                  # M(other text's memory vector)
            pre = ops.linear(hout, H_.weight, None, res=tm, res_div=S, m_dev=n_tok)                    # :517-518 before the sigmoid
            gated.append(ops.gate_mul(hout, pre, out=pre, n_rows_dev=n_tok))                           # :520-521 (in place over pre)
        return self._attend(gated, (mask_t, mask_b), n_dev, (texts[0][1], texts[1][1]), pooled)

    def _attend(self, gated, masks, n_dev, n_toks, pooled):
        """The encoder behind the gates (:524-529), from the gated LSTM outputs g [cap S, 2h] of the title and the body (zeros behind every
        length), their masks [cap, S] (uint8, slot 0 set) and the live token rows n_toks = n_dev . S of each (device ints): self attention,
        cross attention with the other text's self attention as the query, their sum -> pooled [cap, 4h].  Shared by the pass that runs the recurrence (``_encode``) and the pass that reads it
        from the per-news cache (``encode_cached_flat``)."""
        cap, h = masks[0].shape[0], self.hidden_dim
        own = []
        for g, mask, n_tok, att in zip(gated, masks, n_toks, (self.title_self_attention, self.content_self_attention)):
            S = mask.shape[1]
            hidden = ops.linear(g, att.affine1.weight, att.affine1.bias, act='tanh', m_dev=n_tok)
            own.append(ops.additive_pool(hidden, att.affine2.weight.view(-1), g, cap, S, mask=mask, n_seq_dev=n_dev))   # :524-525
        ones = _ones(2 * h, gated[0].device)
        for k, att in enumerate((self.title_cross_attention, self.content_cross_attention)):
            g, mask = gated[k], masks[k]
            S = mask.shape[1]
            q = ops.linear(own[1 - k], att.Q.weight, att.Q.bias, m_dev=n_dev)                          # Q(other text's self attention)
            v = ops.linear(q, att.K.weight.t().contiguous(), None, m_dev=n_dev)                        # K^T q: K(h_t) . q = h_t . (K^T q)
            terms = ops.gate_mul(g, v, div=S, scale=1.0 / att.attention_scalar, sigmoid=False, n_rows_dev=n_toks[k])
            cross = ops.additive_pool(terms, ones, g, cap, S, mask=mask, n_seq_dev=n_dev)               # :527-528
            ops.fuse_rows(own[k], cross, out=pooled[:, 2 * h * k:2 * h * (k + 1)])                      # :529
        return pooled

    def encode_flat(self, title_text, title_mask, content_text, category, subCategory, out, content_mask=None, pair_groups=None):
        """pair_groups: the news counts of the reference calls this pass stands for (they add up to M): the gates then read the
        reference's partner news (class docstring).  None: every news reads its own other text (the encoder as published)."""
        _no_train_dropout(self, self.dropout_rate)
        if content_mask is None:
            raise TypeError('the CNE content encoder reads the body mask (content_mask): pass it -- it is never guessed from the ids')
        M, T = title_text.shape
        L = content_text.shape[1]
        h = self.hidden_dim
        dev = title_text.device
        if pair_groups is not None and sum(pair_groups) != M:
            raise ValueError('pair_groups %s do not add up to the %d news of the pass' % (list(pair_groups), M))
        t_mask, b_mask = self.slot0_mask(title_mask.reshape(M, T)), self.slot0_mask(content_mask.reshape(M, L))
        self._encode(_i32(title_text).contiguous(), t_mask, _i32(content_text).contiguous(), b_mask, _row_count(M, dev), out[:, :4 * h],
                     pair_groups)                                                                       # :529 into the first 4h columns
        ops.topic_rep(category, subCategory, self.category_embedding.weight, self.subCategory_embedding.weight,
                      emb_out=out[:, 4 * h:])                                                           # :531, :221-226
        return out

    # ---- per-news recurrence cache (eval: the recurrence and H h_t depend on the news alone; the gates' partners on the call) ----------
    def _cache_sources(self):
        """The parameters a recurrence cache is computed from."""
        return [self.word_embedding.weight] + list(self.title_lstm.parameters()) + list(self.content_lstm.parameters()) + \
               [self.title_H.weight, self.content_H.weight]

    def _cache_state(self):
        ps = self._cache_sources()
        return tuple(p._version for p in ps), torch.stack([p.detach().view(torch.int32).sum(dtype=torch.int64) for p in ps])

    def cache_is_current(self, cache):
        """True while the parameters a CNERecurrenceCache was built from are what they were: the ``_version`` counters on the host first,
        then the bit-pattern sums on the device (one small reduction per parameter and one read-back; see CNERecurrenceCache)."""
        versions, fingerprint = self._cache_state()
        return versions == cache.versions and fingerprint.device == cache.fingerprint.device and bool(torch.equal(fingerprint, cache.fingerprint))

    @torch.no_grad()
    def build_recurrence_cache(self, title_text, title_mask, content_text, content_mask, news_per_pass=None):
        """-> CNERecurrenceCache over the n news title_text [n, T] / content_text [n, L] (int ids) with their masks: every text through the
        input projection, the LSTM and the H GEMM ONCE, in chunks of news (``lstm_chunks``: a chunk's gi stays within
        GI_BYTES_PER_PASS; ``news_per_pass`` caps a chunk further), each chunk's dense [chunk . S, 2h] results packed to the live
        tokens (ops.seq_pack).  Dense this would be 1 MB per news at the defaults, packed it is 6.4 KB per live token
        (CNERecurrenceCache).  One device -> host read per text (the packed row count).  Rebuild it when the weights change."""
        _no_train_dropout(self, self.dropout_rate)
        h = self.hidden_dim
        table = self.word_embedding.weight
        dev = table.device
        n = title_text.shape[0]
        if news_per_pass is not None and news_per_pass < 1:
            raise ValueError('news_per_pass must be positive')
        versions, fingerprint = self._cache_state()
        texts = []
        for ids, mask, lstm, H_ in ((title_text, title_mask, self.title_lstm, self.title_H),
                                    (content_text, content_mask, self.content_lstm, self.content_H)):
            S = ids.shape[1]
            ids = _i32(ids).contiguous()
            lens = ops.mask_lengths(self.slot0_mask(mask.reshape(n, S)), min_len=1)                    # :492-495
            offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            offsets[1:] = torch.cumsum(lens, 0, dtype=torch.int64)
            rows = int(offsets[-1]) if n else 0
            hp = torch.empty((rows, 2 * h), dtype=torch.float32, device=dev)
            hhp = torch.empty((rows, 2 * h), dtype=torch.float32, device=dev)
            m = torch.empty((n, 2 * h), dtype=torch.float32, device=dev)
            wih, bias, whh = self.lstm_weights(lstm)
            for c0, c1 in self.lstm_chunks(n, S) if n else []:
                for r0 in range(c0, c1, news_per_pass or c1 - c0):
                    r1 = min(c1, r0 + (news_per_pass or c1 - c0))
                    gi = ops.linear(table, wih, bias, a_ids=ids[r0:r1].reshape(-1))                    # :501-502 gather + W_ih x + b
                    hout, c = ops.lstm(gi, whh, lens[r0:r1], S)                                        # :509-510, :514-515
                    del gi
                    hh = ops.linear(hout, H_.weight, None)                                             # H h_t of :517-518
                    ops.seq_pack(hout, lens[r0:r1], offsets[r0:r1], hp, S)
                    ops.seq_pack(hh, lens[r0:r1], offsets[r0:r1], hhp, S)
                    m[r0:r1] = c.transpose(0, 1).reshape(r1 - r0, 2 * h)                               # :512-513
            texts.append(CNERecurrenceCache.Text(S, lens, offsets, hp, hhp, m))
        return CNERecurrenceCache(texts[0], texts[1], versions, fingerprint)

    def encode_cached_flat(self, cache, news_index, title_mask, content_mask, category, subCategory, out, pair_groups=None):
        """``encode_flat`` for M news of a CNERecurrenceCache, news_index int32 [M]: ``_encode`` with the recurrence and the H GEMM read
        from the cache.  What still runs per call: the pass's lengths (a gather), the pairing (``reference_pairs`` on them, per
        ``pair_groups``: a list of counts or the per-news call numbers), the partner's memory term M m_partner + b (one small GEMM over
        news, not over tokens), the gate from the packed rows in one launch (ops.cne_gate_cached) and, unchanged, the attentions behind
        it (``_attend``).  title_mask [M, T] / content_mask [M, L] are the masks of the same news: they mask the attentions by position,
        with the slot-0 rule on copies."""
        _no_train_dropout(self, self.dropout_rate)
        idx = _i32(news_index.reshape(-1)).contiguous()
        M, h = idx.numel(), self.hidden_dim
        dev = idx.device
        T, L = cache.title.S, cache.body.S
        if title_mask.numel() != M * T or content_mask.numel() != M * L:
            raise ValueError('the masks must be [%d, %d] and [%d, %d] (the cache\'s token slots), got %s and %s'
                             % (M, T, M, L, tuple(title_mask.shape), tuple(content_mask.shape)))
        if pair_groups is not None and not isinstance(pair_groups, torch.Tensor) and sum(pair_groups) != M:
            raise ValueError('pair_groups %s do not add up to the %d news of the pass' % (list(pair_groups), M))
        masks = (self.slot0_mask(title_mask.reshape(M, T)), self.slot0_mask(content_mask.reshape(M, L)))
        texts = (cache.title, cache.body)
        pairs = None
        if pair_groups is not None:
            long_idx = idx.long()
            pairs = self.reference_pairs(cache.title.lens[long_idx], cache.body.lens[long_idx], pair_groups, M)
        gated = []
        for k, M_ in enumerate((self.title_M, self.content_M)):
            partner = idx if pairs is None else idx[pairs[k].long()]                                   # the reference's partner news
            m_other = ops.gather_rows(partner, texts[1 - k].m, torch.empty((M, 2 * h), dtype=torch.float32, device=dev))
            tm = ops.linear(m_other, M_.weight, M_.bias)                                               # M(partner's memory vector) + b
            gated.append(ops.cne_gate_cached(texts[k].h, texts[k].hh, texts[k].offsets, texts[k].lens, idx, tm, texts[k].S))   # :517-521
        self._attend(gated, masks, _row_count(M, dev), (_row_count(M * T, dev), _row_count(M * L, dev)), out[:, :4 * h])
        ops.topic_rep(category, subCategory, self.category_embedding.weight, self.subCategory_embedding.weight,
                      emb_out=out[:, 4 * h:])                                                           # :531, :221-226
        return out
