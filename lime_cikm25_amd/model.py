"""Drop-in ``Model`` for the LIME-{CROWN,CNN,NAML,MHSA,CNE,KCNN}-{CROWN,ATT,MHSA} scoring path and the baselines without LIME,
{CROWN,CNN,NAML,MHSA,KCNN}-{ATT,MHSA} and CROWN-CROWN (reference model.py:11-187)."""
import functools
import os

import torch
import torch.nn as nn

from . import newsEncoders, ops, serving, training, userEncoders
from .util import RemainingLifetimeWeighting

# positions (in the 26-tensor signature, model.py:151-154) of the inputs the scoring path reads; the others
# (user_ID, *_entity, content masks, user_history_graph / category_mask / category_indices) are ignored by the
# reference too (last bullet)
_USED = (1, 2, 3, 4, 6, 9, 10, 11, 15, 16, 17, 18, 20, 23, 24, 25)
# (candidate tensor, history tensor) pairs the news encoder concatenates: title_text, title_mask, content_text, category,
# subCategory, freshness, user_topic_lifetime
_PAIRS = ((17, 3), (18, 4), (20, 6), (15, 1), (16, 2), (23, 9), (24, 10))
# a content encoder that reads the body masks (CNE) adds user_content_mask / news_content_mask and their pair
_USED_BODY_MASK = tuple(sorted(_USED + (7, 21)))
_PAIRS_BODY_MASK = _PAIRS + ((21, 7),)
# a content encoder that reads the title's entity ids (KCNN) adds user_title_entity / news_title_entity and their pair
_USED_TITLE_ENTITY = tuple(sorted(_USED + (5, 19)))
_PAIRS_TITLE_ENTITY = _PAIRS + ((19, 5),)


_USER_ENCODERS = ('CROWN', 'ATT', 'MHSA')
_CONTENT_ENCODERS = ('CROWN', 'CNN', 'NAML', 'MHSA', 'CNE', 'KCNN')
# config.news_encoder other than 'LIME' (model.py:41-62): the content encoder as the news encoder itself, the baselines of the paper
_PLAIN_NEWS_ENCODERS = ('CROWN', 'CNN', 'NAML', 'MHSA', 'KCNN')
# why the reference's other user encoders (model.py:67-88) stay refused
_REFUSED_USER_ENCODERS = {
    'LSTUR': ' (it needs user_ID embeddings and a GRU)', 'GRU': ' (it needs a GRU over the history)',
    'PUE': ' (it needs user_ID embeddings)', 'CATT': ' (it pools the history per candidate)',
    'MINER': ' (poly attention with per-candidate pooling)', 'SUE': ' (it is not part of this port)',
    'FIM': ' (it needs the HDC news encoder and the FIM click predictor)',
}


# why the reference's other click predictors (model.py:116-128, :185-186) stay refused
_REFUSED_CLICK_PREDICTORS = {
    'sigmoid': ' (the reference\'s forward has no branch for it: model.py:179-186 leaves logits unset)',
    'FIM': ' (it needs the HDC news encoder and the FIM user encoder, model.py:108-110)',
}


# A baseline model's candidates depend on the news alone: the grouped match reads them in place through an index
# (lime_grouped_match_indexed_f32).  LIME_INDEXED_MATCH=0 keeps the gather form for them too -- one materialised row and one Q row per
# (user, candidate) pair, the path LIME models take -- as the yardstick of the indexed one (tools/bench_recommend.py, tools/bench_lists.py).
INDEXED_MATCH = os.environ.get('LIME_INDEXED_MATCH', '1') != '0'
# A LIME candidate under 'add' or 'concat' + project is A[news] + T[occurrence] with everything behind it linear: the grouped match
# composes it from a news table and an occurrence table while it loads the pair's operand (lime_grouped_match_occurrence_f32,
# Model.occurrence_match_applicable), and no row, Q row or nw row exists per (user, candidate) pair.  Off by default: every path is
# then the materialised one, bit for bit; LIME_OCCURRENCE_MATCH=1 turns it on (tools/bench_recommend.py and tools/bench_lists.py
# alternate the two, DESIGN.md "LIME candidates in place").
OCCURRENCE_MATCH = os.environ.get('LIME_OCCURRENCE_MATCH', '0') != '0'
# A schedule of S time slots (Model.score_schedule) moves only the occurrence row and the remaining lifetime of such a candidate, so
# the two big products of the match run once per pair and a slot is an epilogue (lime_grouped_match_schedule_f32,
# Model.schedule_match_applicable).  On by default for that entry; LIME_SCHEDULE_MATCH=0 keeps the shared-user-side route -- the
# existing match once per slot on one user side, bit for bit S score_pool calls -- as its yardstick (tools/bench_schedule.py).
SCHEDULE_MATCH = os.environ.get('LIME_SCHEDULE_MATCH', '1') != '0'


class Model(nn.Module):
    """Same constructor, attributes (``model_name``, ``config``, ``news_encoder``, ``user_encoder``,
    ``news_embedding_dim``), ``initialize()`` and 26-tensor ``forward`` as the reference's Model
    (model.py:12-187); ``state_dict()`` has the reference's key set.  ``forward`` returns logits [B, N].
    ``config.news_encoder``: 'LIME' (the default), or 'CROWN', 'CNN', 'NAML', 'MHSA' or 'KCNN' -- that content encoder as the news
    encoder itself, the baselines of the paper (model.py:41-62: ``model_name`` is "X-Y", ``news_encoder`` IS the content encoder, so the
    keys carry no ``base_news_encoder.`` level, ``config.content_encoder`` is not read, freshness and lifetime inputs are accepted and
    not read; the ATT and MHSA user encoders pair with all five, CROWN with 'CROWN' alone; 'CNE' without LIME stays refused).
    ``config.content_encoder`` picks LIME's base encoder: 'CROWN', 'CNN', 'NAML' (cnn_method 'naive' or 'group3'), 'MHSA', 'CNE' or
    'KCNN' (cnn_method 'naive', 'group3' or 'group4'; it reads the ``*_title_entity`` inputs);
    ``config.user_encoder`` the user encoder: 'CROWN', 'ATT' (NAML's additive attention) or 'MHSA' (NRMS's self-attention), in any
    pairing.
    ``config.click_predictor``: 'dot_product' (the default: the lifetime-weighted dot product) or 'mlp' (model.py:113-115, :182-184:
    ``logits = out(dropout(relu(mlp(cat[user, news]))))`` with ``mlp``: 2 D -> D // 2 and ``out``: D // 2 -> 1, the last four keys of the
    state_dict; no remaining-lifetime weight, ``remaining_lifetime`` is accepted and not read), with any of the models above.

    ``config.alpha`` (config.py:81, the weight of CROWN's category-prediction loss): with a bare CROWN news encoder ('CROWN' with
    the CROWN, ATT or MHSA user encoder) and ``alpha != 0``, a forward on the differentiable path leaves on
    ``model.news_encoder.auxiliary_loss`` a 0-dim tensor with autograd: alpha x the mean over the B H history rows (padded slots
    count, with category 0) of the cross-entropy of ``category_predictor.fc(title intent vector)`` against the news' category
    (newsEncoders.py:358-364), which trainer.py:137-139 adds to the loss -- ``loss = loss + model.news_encoder.auxiliary_loss.mean()``
    works as written.  The reference runs the predictor on the candidate rows as well (model.py:171) and overwrites that value with the
    history call's (userEncoders.py:110): the candidates' value is not computed here.  Every other forward -- scoring, the cached
    passes, the serving entries -- sets the attribute to None (the reference computes the value in eval mode too, where nothing
    reads it).  Under LIME the attribute stays None and ``category_predictor`` untrained whatever ``alpha`` is (the wrapper copies the
    attribute once at construction, newsEncoders.py:100-103), and with ``alpha == 0`` nothing is computed: the reference's term is
    then an exact zero with exact-zero gradients, on which Adam moves nothing (``training.trains_category_predictor``).

    Scoring (eval mode, or any call under ``torch.no_grad()``): the forward pass runs entirely in hand-written HIP
    kernels and records no autograd graph.  In training mode with grad enabled (``model.train(); model(...)``, what
    trainer.py:131 does) ``forward`` takes the differentiable path of ``lime_cikm25_amd.training``.  Candidates and history
    are encoded in one pass over the news-encoder kernels (the reference encodes them in two calls, model.py:171 and userEncoders.py:110).

    The ~75 kernel launches of a forward are captured once per input signature into a HIP graph and replayed
    (``use_graph``, on by default): the forward is launch-bound from Python otherwise (2.5 ms of gaps on 6 ms of
    kernels at batch 32).  Inputs are copied into the graph's static buffers on every call; parameters are read in
    place, so in-place updates (``load_state_dict``, optimizer steps) need no re-capture, while ``.to()/.cuda()``
    drop the captured graphs.
    """

    def __init__(self, config):
        super().__init__()
        self.config = config
        if config.news_encoder == 'LIME':
            if config.content_encoder not in _CONTENT_ENCODERS:
                raise NotImplementedError('content_encoder %r is a baseline outside the scoring path' % config.content_encoder)
            base_encoder = getattr(newsEncoders, config.content_encoder)(config)
            self.news_encoder = newsEncoders.LIME(config=config, base_news_encoder=base_encoder)
        elif config.news_encoder in _PLAIN_NEWS_ENCODERS:
            # the baseline form (model.py:41-62): the content encoder IS the news encoder -- no wrapper, so the state_dict keys are
            # news_encoder.word_embedding.weight, ...; config.content_encoder is not read
            base_encoder = self.news_encoder = getattr(newsEncoders, config.news_encoder)(config)
        elif config.news_encoder == 'CNE':
            raise NotImplementedError('news_encoder \'CNE\' without LIME stays refused: its gates pair the news of an encoder call, so it '
                                      'has no per-news cache, and its 1,700-column representation is outside the refinement kernels -- '
                                      'use news_encoder=\'LIME\' with content_encoder=\'CNE\'')
        else:
            raise NotImplementedError('news_encoder %r: the MI355X path covers LIME (config.py:25) and the baselines %s' % (
                config.news_encoder, ', '.join(_PLAIN_NEWS_ENCODERS)))
        if config.user_encoder not in _USER_ENCODERS:
            raise NotImplementedError('user_encoder %r is outside the scoring path%s: the supported user encoders are %s' % (
                config.user_encoder, _REFUSED_USER_ENCODERS.get(config.user_encoder, ''), ', '.join(sorted(_USER_ENCODERS))))
        if config.user_encoder == 'CROWN' and config.news_encoder not in ('LIME', 'CROWN'):
            # userEncoders.py:103-105: the CROWN user encoder runs news_encoder.category_affine over the 100-wide topic pair
            raise NotImplementedError('user_encoder \'CROWN\' needs the news encoder\'s category_affine over the (category, subCategory) '
                                      'pair (userEncoders.py:103-105): news_encoder %r has %s -- pair it with ATT or MHSA, or put it under LIME'
                                      % (config.news_encoder, 'a category_affine of another shape' if hasattr(self.news_encoder, 'category_affine')
                                         else 'no category_affine'))
        self.user_encoder = getattr(userEncoders, config.user_encoder)(self.news_encoder, config)
        self.plain = config.news_encoder != 'LIME'          # a baseline: the news encoder is the content encoder itself
        self.model_name = (f"{config.news_encoder}-{config.user_encoder}" if self.plain else
                           f"{config.news_encoder}-{config.content_encoder}-{config.user_encoder}")     # model.py:92-95
        self.news_embedding_dim = self.news_encoder.news_embedding_dim
        self.dropout = nn.Dropout(p=config.dropout_rate)
        self.use_user_embedding = False
        self.click_predictor = config.click_predictor
        if self.click_predictor == 'mlp':                    # model.py:113-115
            self.mlp = nn.Linear(in_features=self.news_embedding_dim * 2, out_features=self.news_embedding_dim // 2, bias=True)
            self.out = nn.Linear(in_features=self.news_embedding_dim // 2, out_features=1, bias=True)
        elif self.click_predictor != 'dot_product':
            raise NotImplementedError('click_predictor %r stays refused%s: the supported click predictors are dot_product (config.py:109) '
                                      'and mlp' % (self.click_predictor, _REFUSED_CLICK_PREDICTORS.get(self.click_predictor, '')))
        self.remaining_lifetime_weighting = RemainingLifetimeWeighting(config)
        self._regular_offsets = {}
        self.use_graph = True
        self._graphs = {}
        # the inputs the captured graph copies in, per model: the body masks only where the content encoder reads them
        self.reads_content_mask = bool(getattr(base_encoder, 'reads_content_mask', False))
        self.reads_title_entity = bool(getattr(base_encoder, 'reads_title_entity', False))
        self._used = _USED_BODY_MASK if self.reads_content_mask else _USED_TITLE_ENTITY if self.reads_title_entity else _USED
        self._pairs = _PAIRS_BODY_MASK if self.reads_content_mask else _PAIRS_TITLE_ENTITY if self.reads_title_entity else _PAIRS

    @property
    def content_encoder(self):
        """The content encoder: LIME's base encoder, or the news encoder itself in the baseline form."""
        return self.news_encoder if self.plain else self.news_encoder.base_news_encoder

    def _apply(self, fn, *args, **kwargs):
        self._graphs = {}                      # parameter storage moves: captured pointers are stale
        self._regular_offsets = {}
        self._graphs_kept_key = None         # (the content encoder drops what it keeps across forwards in its own _apply)
        return super()._apply(fn, *args, **kwargs)

    def weights_changed(self):
        """Tell the model that parameter memory was written in a way torch does not record: an edit through ``p.data`` (it moves
        neither ``p._version`` nor the address), or a kernel handed a raw pointer.  What is kept across scoring forwards
        (``newsEncoders.WeightProducts``) is recomputed, in place, before the next one.  In-place torch ops on the parameters,
        ``load_state_dict``, ``TrainStep`` and ``.to()`` need no such call."""
        ops.note_param_write()

    def _kept_key(self):
        """What the captured graphs depend on beyond their inputs: the ``kept_key()`` of the news encoder and, below LIME, of the content
        encoder (``kept.key``: buffer generations and whether the forward takes them).  Brings what they keep up to date, in place and
        on the current stream, on the way."""
        ne = self._modules['news_encoder']                  # (no attribute walk through nn.Module.__getattr__ in front of every replay)
        return ne.kept_key() if self.plain else (ne._modules['base_news_encoder'].kept_key(), ne.kept_key())

    def _sync_kept(self):
        """Before a scoring forward: bring what the encoders keep across forwards up to date (in place, on the current stream) and drop
        the captured graphs if one of those buffers had to move or the forward changed between taking them and computing its own.  An
        in-place refresh keeps the graphs."""
        key = self._kept_key()
        if key != self.__dict__.get('_graphs_kept_key'):
            self._graphs_kept_key = key
            self._graphs = {}

    def initialize(self):
        self.news_encoder.initialize()
        self.user_encoder.initialize()
        if self.click_predictor == 'mlp':                    # model.py:139-141 (``out`` keeps nn.Linear's default initialisation)
            nn.init.xavier_uniform_(self.mlp.weight, gain=nn.init.calculate_gain('relu'))
            nn.init.zeros_(self.mlp.bias)
        self.remaining_lifetime_weighting.initialize()

    def forward(self, user_ID, user_category, user_subCategory, user_title_text, user_title_mask, user_title_entity,
                user_content_text, user_content_mask, user_content_entity, user_freshness, user_user_topic_lifetime,
                user_history_mask, user_history_graph, user_history_category_mask, user_history_category_indices, news_category,
                news_subCategory, news_title_text, news_title_mask, news_title_entity, news_content_text, news_content_mask,
                news_content_entity, news_freshness, news_user_topic_lifetime, remaining_lifetime):
        args = (user_ID, user_category, user_subCategory, user_title_text, user_title_mask, user_title_entity,
                user_content_text, user_content_mask, user_content_entity, user_freshness, user_user_topic_lifetime,
                user_history_mask, user_history_graph, user_history_category_mask, user_history_category_indices, news_category,
                news_subCategory, news_title_text, news_title_mask, news_title_entity, news_content_text, news_content_mask,
                news_content_entity, news_freshness, news_user_topic_lifetime, remaining_lifetime)
        self.news_encoder.auxiliary_loss = None        # only the differentiable path below leaves a term (no stale tensor survives)
        if self.training and (torch.is_grad_enabled() or self.news_encoder.training or self.user_encoder.training):
            # trainer.py:131-145: model.train(); logits = model(...); loss.backward() -- the differentiable path.  It is also the
            # path with the training-mode dropouts (model.train() under no_grad: the layer's p = 0.2 dropout of layers.py:74 is
            # active whatever config.dropout_rate says); `model.eval(); model.training = True` keeps the [B, K] shape on the
            # fused scoring kernels (children in eval mode)
            return training.forward_train(self, user_category, user_subCategory, user_title_text, user_title_mask,
                                          user_content_text, user_freshness, user_user_topic_lifetime, user_history_mask,
                                          news_category, news_subCategory, news_title_text, news_title_mask, news_content_text,
                                          news_freshness, news_user_topic_lifetime, remaining_lifetime,
                                          user_content_mask=user_content_mask if self.reads_content_mask else None,
                                          news_content_mask=news_content_mask if self.reads_content_mask else None,
                                          user_title_entity=user_title_entity if self.reads_title_entity else None,
                                          news_title_entity=news_title_entity if self.reads_title_entity else None)
        if (self.use_graph and ops.PROFILE is None and user_category.is_cuda
                and not torch.cuda.is_current_stream_capturing()):
            self._sync_kept()                  # (an eager forward brings them up to date where it uses them: CROWN.encode_flat)
            return self._forward_graphed(args)
        return self._forward_impl(*args)

    def _forward_graphed(self, args):
        _USED = self._used
        used = [args[i] for i in _USED]
        key = (self.training,) + tuple((tuple(t.shape), t.dtype) for t in used)
        entry = self._graphs.get(key)
        if entry is None:
            static = list(args)
            for i, t in zip(_USED, self._packed_like(args, _USED, self._pairs)):
                static[i] = t
            ops.multi_copy([(static[i], args[i]) for i in _USED])
            with torch.no_grad():
                self._forward_impl(*static)                 # eager warm-up: lazy one-time set-up stays out of the capture
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = self._forward_impl(*static)
            entry = (graph, [static[i] for i in _USED], out)
            self._graphs[key] = entry
            self._graphs_kept_key = self._kept_key()            # (the warm-up may have built the weight products / tables this graph reads)
        graph, static_used, out = entry
        keep = ops.multi_copy(list(zip(static_used, used)))          # one launch for all the inputs
        graph.replay()
        del keep
        return out.clone()

    @staticmethod
    def _packed_like(args, _USED=_USED, _PAIRS=_PAIRS):
        """Static input buffers for the graph: ONE allocation, with every candidate tensor directly in front of its
        history counterpart (news_title_text | user_title_text, ...) so that the encoder's `cat` of the two groups is a
        view of the buffer instead of a copy kernel (newsEncoders.LIME.encode_many)."""
        order = list(_USED)
        for n_i, u_i in _PAIRS:                                      # news tensor, then the user tensor right behind it
            order.remove(u_i)
            order.insert(order.index(n_i) + 1, u_i)
        offs, total = {}, 0
        for i in order:
            t = args[i]
            adjacent = any(i == u and args[n].dtype == t.dtype for n, u in _PAIRS)
            if not adjacent:
                total = (total + 255) // 256 * 256                   # 256-byte aligned unless glued to its partner
            offs[i] = total
            total += t.numel() * t.element_size()
        buf = torch.empty(total + 256, dtype=torch.uint8, device=args[_USED[0]].device)
        base = (-buf.data_ptr()) % 256
        out = []
        for i in _USED:
            t = args[i]
            nbytes = t.numel() * t.element_size()
            out.append(buf[base + offs[i]:base + offs[i] + nbytes].view(t.dtype).view(t.shape))
        return out

    @torch.no_grad()
    def score_impressions(self, user_category, user_subCategory, user_title_text, user_title_mask, user_content_text,
                          user_freshness, user_user_topic_lifetime, user_history_mask, news_category, news_subCategory,
                          news_title_text, news_title_mask, news_content_text, news_freshness, news_user_topic_lifetime,
                          remaining_lifetime, n_src=None, rows_per_pass=16384, user_content_mask=None, news_content_mask=None,
                          user_title_entity=None, news_title_entity=None):
        """Scoring-only layout of BASELINE config 5: B impressions with K candidates each -> logits [B, K] with the
        reference's EVAL semantics (util.py:86-111: every (impression, candidate) pair is its own row with N = 1, Q16),
        but every history is encoded ONCE instead of once per candidate.

        user_* [B, H, ...], news_* [B, K, ...] (news_user_topic_lifetime may be [B] or [B, K]), remaining_lifetime [B, K].
        ``n_src``: the GraphSAGE closed form averages over the first n_src node slots, and the reference takes n_src =
        rows of the forward, i.e. its eval batch size (Q7); default: B * K capped at H + config.batch_size, which is what
        one reference forward over all pairs would use.  The result equals ``forward`` in eval mode on the B * K expanded
        rows (tested), the history encoder just runs B * H instead of B * K * H times.
        ``user_content_mask`` [B, H, L] / ``news_content_mask`` [B, K, L]: the body masks, for a content encoder that reads them (CNE).
        Under CNE a history's encoding is NOT a function of the history alone -- the reference gates every text with the memory vector
        of the news at the same length-sorted position of the encoder call (newsEncoders.CNE) -- so nothing can be shared between the
        K candidates of an impression: the B * K expanded rows go through the eval forward as they are, in one pass.
        ``user_title_entity`` [B, H, T] / ``news_title_entity`` [B, K, T]: the titles' entity ids, for the content encoder that reads
        them (KCNN); a KCNN representation depends on the news alone, so the histories are still encoded once.
        """
        B, K = news_category.shape
        H = user_category.shape[1]
        if self.reads_content_mask:
            if user_content_mask is None or news_content_mask is None:
                raise TypeError('the CNE content encoder reads the body masks (user_content_mask, news_content_mask): pass them -- '
                                'a body mask is never guessed from the ids')
            if self.training:
                raise RuntimeError('score_impressions is the eval-mode function: call model.eval() first')
            rows = lambda t: t.reshape((B * K,) + tuple(t.shape[2:]))                        # candidate tensors without the N axis
            rep = lambda t: t.repeat_interleave(K, dim=0)                                    # the impression's history, once per candidate
            if news_user_topic_lifetime.dim() == 1:
                news_user_topic_lifetime = news_user_topic_lifetime.unsqueeze(1).expand(B, K)
            if news_freshness.dim() == 1:
                news_freshness = news_freshness.unsqueeze(1).expand(B, K)
            logits = self._forward_impl(None, rep(user_category), rep(user_subCategory), rep(user_title_text), rep(user_title_mask), None,
                                        rep(user_content_text), rep(user_content_mask), None, rep(user_freshness),
                                        rep(user_user_topic_lifetime), rep(user_history_mask), None, None, None, rows(news_category),
                                        rows(news_subCategory), rows(news_title_text), rows(news_title_mask), None,
                                        rows(news_content_text), rows(news_content_mask), None, rows(news_freshness.contiguous()),
                                        rows(news_user_topic_lifetime.contiguous()), rows(remaining_lifetime))
            return logits.view(B, K)
        ne, ue = self.news_encoder, self.user_encoder
        if self.reads_title_entity and (user_title_entity is None or news_title_entity is None):
            raise TypeError('the KCNN content encoder reads the title entity ids (user_title_entity, news_title_entity): pass them -- '
                            'the ids are never guessed')
        if not self.reads_title_entity:
            user_title_entity = news_title_entity = None
        if news_user_topic_lifetime.dim() == 1:
            news_user_topic_lifetime = news_user_topic_lifetime.unsqueeze(1).expand(B, K)
        if news_freshness.dim() == 1:
            news_freshness = news_freshness.unsqueeze(1).expand(B, K)
        cand, hist = ne.encode_many([
            (news_title_text, news_title_mask, news_content_text, news_category, news_subCategory, news_freshness.contiguous(),
             news_user_topic_lifetime.contiguous(), None, news_title_entity),
            (user_title_text, user_title_mask, user_content_text, user_category, user_subCategory, user_freshness,
             user_user_topic_lifetime, None, user_title_entity)])                     # [B, K, D], [B, H, D]
        rows = B * K
        if n_src is None and hasattr(ue, 'user_node_embedding'):      # CROWN's GraphSAGE alone; the other user encoders ignore n_src
            n_src = min(rows, H + ue.user_node_embedding.shape[0])
        out = torch.empty((B, K), dtype=torch.float32, device=cand.device)
        per = max(1, rows_per_pass // K)                                              # impressions per pass ...
        n_pass = (B + per - 1) // per
        per = (B + n_pass - 1) // n_pass          # ... evened out: the passes then take the same kernels (a short last pass would
                                                  # fall under the row counts from which the big-M GEMM kernels take over)
        rl = remaining_lifetime.float()
        gate_y = ue.gate_projection(hist)                                             # once for every pass's histories (one GEMM shape)
        for b0 in range(0, B, per):
            b1 = min(B, b0 + per)
            n = (b1 - b0) * K
            # the history side (embeddings, topic ids, mask) is shared by the K candidate rows of an impression: hist_div
            logits = self._row_logits(hist[b0:b1], news_category[b0:b1].reshape(n, 1), news_subCategory[b0:b1].reshape(n, 1),
                                      user_category[b0:b1], user_subCategory[b0:b1], user_history_mask[b0:b1],
                                      cand[b0:b1].reshape(n, 1, -1), rl[b0:b1].reshape(n, 1), n_src=n_src, hist_div=K,
                                      gate_y=None if gate_y is None else gate_y[b0 * H:b1 * H])
            out[b0:b1] = logits.view(b1 - b0, K)
        return out

    @torch.no_grad()
    def build_news_cache(self, device_corpus, rows_per_pass=8192):
        """Content cache for ``score_behaviors``: every news of a ``DeviceCorpus`` through the token encoders ONCE.

        Under CNE no part of LIME's representation that this cache could hold depends on the news alone (the gates read the memory
        vector of the news at the same length-sorted position of the encoder call, newsEncoders.CNE): the cache is an empty
        [n_news, 0] tensor and ``score_behaviors`` encodes the rows' news as the uncached forward does."""
        c = device_corpus
        if self.reads_content_mask:
            return torch.empty((c.news_title_text.shape[0], 0), dtype=torch.float32, device=c.news_title_text.device)
        return self.news_encoder.build_content_cache(c.news_title_text, c.news_title_mask, c.news_abstract_text, c.news_category,
                                                     c.news_subCategory, rows_per_pass=rows_per_pass,
                                                     title_entity=c.news_title_entity if self.reads_title_entity else None)

    def build_recurrence_cache(self, device_corpus, news_per_pass=None):
        """CNE alone: the per-news recurrence cache of ``score_behaviors(..., recurrence_cache=...)`` -- every news of a ``DeviceCorpus``
        through the input projection, the LSTM and the H GEMM once (newsEncoders.CNE.build_recurrence_cache; packed, 6.4 KB per live
        token at the defaults).  Any other content encoder has ``build_news_cache`` for this and is refused with a ValueError."""
        if self.config.content_encoder != 'CNE':
            raise ValueError('content_encoder %r has no recurrence cache (it is the CNE content encoder\'s): use build_news_cache'
                             % self.config.content_encoder)
        c = device_corpus
        return self.news_encoder.base_news_encoder.build_recurrence_cache(c.news_title_text, c.news_title_mask, c.news_abstract_text,
                                                                          c.news_abstract_mask, news_per_pass=news_per_pass)

    @torch.no_grad()
    def score_behaviors(self, behaviors, rows, news_cache, n_src=None, recurrence_cache=None, rows_per_forward=None):
        """Scores of the (impression, candidate) rows `rows` of a dev / test ``DeviceBehaviors`` -- the function of
        util.compute_scores' forward (util.py:86-111, eval mode, N = 1 per row) -- from the news cache: no token encoder
        runs, the history and the candidate of a row are looked up by news index and only their freshness half, the user
        encoder and the match are computed.  ``n_src`` as in score_impressions (default: the number of rows, capped).
        Under CNE (an empty cache, ``build_news_cache``) the rows' batch goes through the eval forward instead: a dev / test split and
        a model in eval mode.

        ``recurrence_cache`` (CNE alone, ``build_recurrence_cache``; ValueError under another content encoder): the candidates and the
        histories of the rows are encoded from it in one pass -- no LSTM step and no hidden-state GEMM runs, only the gates, the
        attentions, LIME's freshness tail and the match.  ``rows_per_forward`` = p: the pass stands for the reference forwards over the
        consecutive chunks of p rows (the last may be short) -- the gates read the partners those forwards give (their news counts are
        p candidates and p . H history news per chunk) and the GraphSAGE source count defaults to the chunk's rows -- however many rows
        the pass holds; None: one forward over all rows.  A cache built from other parameter values raises RuntimeError: rebuild it
        after the weights change."""
        if recurrence_cache is not None:
            if self.config.content_encoder != 'CNE':
                raise ValueError('content_encoder %r does not read a recurrence cache (it is the CNE content encoder\'s)'
                                 % self.config.content_encoder)
            return self._score_from_recurrence(behaviors, rows, recurrence_cache, n_src, rows_per_forward)
        b = behaviors
        dev = news_cache.device
        rows = torch.as_tensor(rows, device=dev).long().reshape(-1)
        R, H = rows.numel(), b.hist_index.shape[1]
        ne, ue, c = self.news_encoder, self.user_encoder, b.corpus
        hist_idx, cand_idx = b.hist_index[rows], b.cand_index[rows]                       # [R, H], [R, 1]
        flat_h, flat_c = hist_idx.reshape(-1).long(), cand_idx.reshape(-1).long()
        remaining = self._remaining_lifetime(b, rows, cand_idx)
        if self.reads_content_mask:
            # CNE: the rows' batch through the eval forward (see build_news_cache) -- the scores of util.compute_scores over these rows
            return self._forward_impl(*b.assemble(rows), remaining.view(R)).view(R)
        hist = ne.encode_cached(news_cache, hist_idx, b.user_freshness[rows], b.user_lifetime[rows]).view(R, H, -1)
        cand = ne.encode_cached(news_cache, cand_idx, b.cand_freshness[rows], b.cand_lifetime[rows]).view(R, 1, -1)
        if n_src is None and hasattr(ue, 'user_node_embedding'):
            n_src = min(R, H + ue.user_node_embedding.shape[0])
        logits = self._row_logits(hist, c.news_category[flat_c].view(R, 1), c.news_subCategory[flat_c].view(R, 1),
                                  c.news_category[flat_h].view(R, H), c.news_subCategory[flat_h].view(R, H), b.hist_mask[rows],
                                  cand, remaining.view(R, 1), n_src=n_src)
        return logits.view(R)

    def _remaining_lifetime(self, behaviors, rows, cand_idx):
        """The remaining lifetime of the rows' candidates per config.lifetime_type, as util.py:98-106 derives it from the batch."""
        b = behaviors
        return self._lifetime_rule(b.cand_freshness[rows], lambda: b.cand_lifetime[rows],
                                   lambda: b.corpus.news_category[cand_idx.reshape(-1).long()])

    def _lifetime_rule(self, freshness, lifetime, category):
        """util.py:98-106: the remaining lifetime of candidates from their freshness and, per config.lifetime_type, the fixed lifetime,
        the lifetime of their category or their own (user, topic) lifetime.  ``lifetime`` / ``category``: callables that give the
        tensor (shaped like ``freshness`` / with as many elements), asked only under the type that reads it."""
        lt = getattr(self.config, 'lifetime_type', 'user_topic')
        if lt == 'fixed':
            return self.config.fixed_lifetime - freshness
        if lt == 'topic_wise':
            cmap = torch.as_tensor(self.config.category_lifetime_map, dtype=torch.float32, device=freshness.device)
            return cmap[category().long()].view_as(freshness) - freshness
        if lt == 'user_topic':
            return lifetime() - freshness
        raise ValueError('Invalid lifetime_type')

    _NO_CONTENT_CACHE = ('content_encoder \'CNE\' has no per-news content cache (its gates read the partner news of the encoder call, '
                         'build_news_cache): score_pool / recommend cannot serve it -- score the pairs with score_behaviors')

    def grouped_by(self):
        """What the user side reads of a candidate, as the ``by`` of recommend.pool_plan / topic_table."""
        crown = hasattr(self.user_encoder, 'user_node_embedding')
        return None if not self.user_encoder.use_candidate_aware_attn else 'topic' if crown else 'category'

    @torch.no_grad()
    def score_pool(self, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_index, cand_freshness,
                   cand_lifetime, n_src=None, pairs_per_pass=1 << 18, exclude_history=False):
        """Scores [U, C] of U users against ONE shared pool of C candidate news, from the news cache: ``scores[u, j]`` is the
        eval-mode score (N = 1, util.py:86-111) of the row (history u, candidate ``cand_index[j]``) -- what ``score_behaviors``
        returns for that row with the same ``n_src``.

        ``corpus``: the DeviceCorpus the cache was built from; ``hist_index`` / ``hist_mask`` / ``user_freshness`` /
        ``user_lifetime`` [U, H]: the fields of a DeviceBehaviors row; ``cand_index`` [C]; ``cand_freshness`` [C] or [U, C];
        ``cand_lifetime`` [U, C] (or [C], broadcast).  The remaining lifetime follows config.lifetime_type.  ``n_src``: as in
        score_impressions (default min(U C, H + config.batch_size) under the CROWN user encoder; ignored otherwise).

        Under the eval shape the candidate enters the user side only through its topic (layers.py:66-81), so the refinement, the
        user encoder's own step and the operands of the match are computed once per (user, candidate topic) -- (user, category) under
        ATT / MHSA, once per user with the candidate-aware attention off -- and every pair is left with two dot products per history
        slot and the epilogue (lime_grouped_match_f32; recommend.pool_plan for the grouping).  Users go through in passes that keep
        the candidate rows (users x C) and the refined history rows (users x topics x H) within ``pairs_per_pass`` rows each, at
        least one user a pass: the default keeps the scratch around 1 GB at the full-size model.
        ``exclude_history``: a pair whose candidate sits in a masked-in slot of the user's history scores -inf.
        CNE has no per-news cache and is refused (ValueError).
        A baseline model (no LIME): a candidate's row depends on the news alone, so the pool's C rows (and their Q) are made once per
        call and every pair reads them in place through its pool position (lime_grouped_match_indexed_f32, ``_candidate_tables``); the
        passes are then bounded by the refined history rows alone.  LIME_INDEXED_MATCH=0 keeps the per-pair rows.
        A LIME model with LIME_OCCURRENCE_MATCH=1 where ``occurrence_match_applicable()`` holds: the pool's cache rows (with their Q /
        MLP news half) are one set of tables and ``occurrence_tables()`` (with theirs) another, and every pair is composed from a row
        of each in the kernel (lime_grouped_match_occurrence_f32) -- no ``encode_cached``, Q or MLP GEMM runs over the pairs."""
        return serving.score_pool(self, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_index, cand_freshness,
                                  cand_lifetime, n_src, pairs_per_pass, exclude_history)[0]

    def _offsets_of_rows(self, groups, pairs, device):
        """int64 [groups + 1] on the device: the CSR of the regular shape, ``pairs`` pairs per group.  Kept per shape: a captured forward
        reads the tensor its eager warm-up built (no host-made tensor is born inside a capture)."""
        key = (groups, pairs, str(device))
        off = self._regular_offsets.get(key)
        if off is None:
            off = self._regular_offsets[key] = (torch.arange(groups + 1, dtype=torch.int64) * pairs).to(device)
        return off

    def _row_logits(self, hist, category, subCategory, user_category, user_subCategory, user_history_mask, cand, remaining, agg=None,
                    n_src=None, hist_div=1, gate_y=None):
        """The logits [B, N] of the regular shape -- B = hist.shape[0] * hist_div rows with N candidates each, ``ue.match``'s arguments.
        Under the dot-product predictor this IS ``ue.match`` (the match fused into the user encoder's last kernel); under the MLP
        predictor the user encoder stops at its operands and ``serving.click_logits`` takes the rows as groups of N pairs."""
        ue = self.user_encoder
        if self.click_predictor == 'dot_product':
            return ue.match(hist, category, subCategory, user_category, user_subCategory, user_history_mask, cand,
                            remaining_lifetime=remaining, weighting=self.remaining_lifetime_weighting, agg=agg, n_src=n_src,
                            hist_div=hist_div, gate_y=gate_y)[1]
        if self.training and (ue.training or self.dropout.training):
            raise NotImplementedError('the scoring kernel chain has no training-mode dropouts: Model.forward takes the differentiable path')
        B, N, D = cand.shape
        flat = cand.contiguous().view(B * N, D)
        operands = serving.match_operands(self, hist, category, subCategory, user_category, user_subCategory, user_history_mask, cand=flat,
                                          pairs=B * N, agg=agg, n_src=n_src, hist_div=hist_div, gate_y=gate_y)
        groups = operands.kp.shape[0] // operands.H                                      # (ATT / MHSA without refinement: one per history)
        per = B * N // groups
        return serving.click_logits(self, operands, flat, None, self._offsets_of_rows(groups, per, flat.device), regular=per).view(B, N)

    def occurrence_match_applicable(self):
        """Whether a candidate of this model is a row of a news table plus a row of an occurrence table with only linear maps behind it,
        so that the grouped match can compose it in place (lime_grouped_match_occurrence_f32): a LIME model with fusion_method 'add', or
        'concat' with a projection -- rep(news, occurrence) = A[news] + T[b_f nb + b_l] (LIME.occurrence_tables).  A pure host
        predicate of the configuration.  The others stay on the materialised path:
          'gated': the row is g A + (1 - g) T with g a sigmoid of both sides -- not linear in the occurrence;
          'concat' with ``project`` the identity: the occurrence's columns are concatenated behind the news', not added to them;
          CNE: no part of its representation depends on the news alone, so there is no cache to take a table from;
          the composed MLP form (ops.FUSED_MLP_MATCH off): it is the yardstick on existing launches and reads materialised rows;
          a baseline model: no occurrence at all -- it keeps its indexed path (``occurrence_free``)."""
        ne = self.news_encoder
        if self.plain or self.reads_content_mask:
            return False
        if self.click_predictor == 'mlp' and not ops.FUSED_MLP_MATCH:
            return False
        return ne.fusion_method == 'add' or (ne.fusion_method == 'concat' and not isinstance(ne.project, nn.Identity))

    def schedule_match_applicable(self, H=None):
        """Whether a schedule of this model can take the factorised route (lime_grouped_match_schedule_f32): the dot-product predictor
        on a model whose candidate is a news-table row plus an occurrence-table row (``occurrence_match_applicable()``) or the
        news-table row alone (a baseline, ``occurrence_free``), within the kernel's limits -- the [num_buckets^2, H] occurrence terms
        of a group fit its LDS (ops.grouped_match_schedule_fits; H: the history rows the match sees, config.max_history_num under the
        CROWN user encoder, 1 under ATT / MHSA).  A pure host predicate of the configuration (and ``H``, default
        config.max_history_num); the LIME_SCHEDULE_MATCH switch is not part of it."""
        ne = self.news_encoder
        if self.click_predictor != 'dot_product' or self.reads_content_mask:
            return False
        if getattr(ne, 'occurrence_free', False):
            n_occ = 0
        elif self.occurrence_match_applicable():
            n_occ = ne.freshness_encoder.num_buckets ** 2
        else:
            return False
        H = int(self.config.max_history_num if H is None else H)
        return ops.grouped_match_schedule_fits(H if hasattr(self.user_encoder, 'user_node_embedding') else 1, n_occ)

    def schedule_route(self, n_slots, H=None):
        """How ``score_schedule`` serves ``n_slots`` slots -> 'single': one slot is ``score_pool`` itself; 'expand': a baseline under
        the MLP predictor reads no time at all -- one slot, repeated; 'factorised': ``schedule_match_applicable(H)`` with the
        LIME_SCHEDULE_MATCH switch on; 'shared': every other model -- one user side, the existing match once per slot."""
        if int(n_slots) == 1:
            return 'single'
        if self.click_predictor == 'mlp' and getattr(self.news_encoder, 'occurrence_free', False):
            return 'expand'
        return 'factorised' if SCHEDULE_MATCH and self.schedule_match_applicable(H) else 'shared'

    def _candidate_tables(self, news_cache, rows=None, always=False):
        """The ONE place that asks how the candidates are read -> None: ``serving.pass_logits`` materialises a row and a Q row per pair; or
        the ``serving.Tables`` (cand [n, D], qp [n, A], nw, occurrence) that the grouped match reads in place, once per call: the news of
        ``rows`` (the pool, in plan order) or, with ``rows`` None, every news of the cache (the lists: a pair's index is its news id).
        Under ATT / MHSA (a history of one row) qp is never felt: n rows of four zero columns -- the kernel reads both tables at one index.
        Under the MLP click predictor a third table stands beside them: nw [n, D // 2] = cand W_n^T + mlp.bias, the news half of the
        predictor's hidden layer, once per call (None on the composed form and under the dot product).

        A baseline model (``occurrence_free``: the representation depends on the news alone, INDEXED_MATCH): cand is the news' rows
        themselves and ``occurrence`` is None (lime_grouped_match_indexed_f32 / lime_grouped_mlp_match_indexed_f32).
        A LIME model for which ``occurrence_match_applicable()`` holds (OCCURRENCE_MATCH): cand = A, the cache rows, qp = A Q^T + b_Q and
        nw = A W_n^T + mlp.bias, and ``occurrence`` is (ct, qt, nt) = (T, T Q^T, T W_n^T) [num_buckets^2 rows, no bias: it is in
        the news tables] from LIME.occurrence_tables(); a pair adds its bucket pair's row of them in the kernel
        (lime_grouped_match_occurrence_f32 / lime_grouped_mlp_match_occurrence_f32).  Every other model: None.
        ``always``: the tables wherever the model has them, whatever the two switches say (the factorised schedule reads nothing else)."""
        ne, ue = self.news_encoder, self.user_encoder
        plain = (INDEXED_MATCH or always) and getattr(ne, 'occurrence_free', False)
        if not plain and not ((OCCURRENCE_MATCH or always) and self.occurrence_match_applicable()):
            return None
        if plain:
            cand, ct = (news_cache.contiguous() if rows is None else ne.encode_cached(news_cache, rows)), None
        else:
            cand, ct = (news_cache.contiguous() if rows is None else news_cache.index_select(0, rows)), ne.occurrence_tables()[0]
        crown, mlp = hasattr(ue, 'user_node_embedding'), self.click_predictor == 'mlp' and ops.FUSED_MLP_MATCH

        def behind(t, bias):
            """(qp, nw) of the rows t: Q (userEncoders.py:162; four zero columns where it is never felt) and the MLP predictor's news
            half of the hidden layer, a function of the news alone too."""
            qp = (ops.linear(t, ue.Q.weight, ue.Q.bias if bias else None) if crown else
                  torch.zeros((t.shape[0], 4), dtype=torch.float32, device=t.device))
            return qp, (ops.linear(t, self.mlp.weight[:, t.shape[1]:], self.mlp.bias if bias else None) if mlp else None)
        return serving.Tables(cand, *behind(cand, True), None if ct is None else serving.Occurrence(ct, *behind(ct, False)))

    @torch.no_grad()
    def recommend(self, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_index, cand_freshness,
                  cand_lifetime, k, n_src=None, pairs_per_pass=1 << 18, exclude_history=False, max_per_topic=None, quota_by='category',
                  mmr_lambda=None, shortlist=None, similarity=None, calibrate_lambda=None, calibrate_by='category',
                  calibrate_alpha=0.01, calibrate_weights=None):
        """The k best news of the pool per user, on the device: ``score_pool`` (same arguments), then lime_topk_rows_f32 ->
        (positions int32 [U, k] into ``cand_index``, scores fp32 [U, k]).  Rows are in descending order of the score; equal scores
        (+0.0 and -0.0 are equal) go lower position first; a NaN ranks after every number, in position order.  With
        ``exclude_history`` a candidate that sits in a masked-in slot of the user's history is never returned; when fewer than k
        candidates remain, the trailing slots hold position -1 and score -inf.  1 <= k <= 128.

        ``max_per_topic`` = q (an integer >= 1; None: no quota, today's launches and bits): at most q news of one group in a user's
        row -- the candidates are walked in the order above and one is taken unless q of its group were taken before it, until k
        are (lime_topk_rows_quota_f32; ``recommend.quota_topk`` states it on the host).  ``quota_by``: 'category', or 'topic' -- the
        (category, subCategory) pair; it is independent of what the user side groups by (``grouped_by()``), so a model without
        candidate-aware attention takes quotas too.  An excluded candidate uses no quota.  A corpus of more than 8192 groups is
        refused (ValueError), as are a ``max_per_topic`` that is no integer >= 1 and an unknown ``quota_by``.

        ``mmr_lambda`` = lam (a real in [0, 1]; None: no MMR, today's launches and bits): the slate is chosen by maximal marginal
        relevance among the ``shortlist`` best (an integer in [k, 128], default min(128, max(k, 64)); under ``max_per_topic`` the
        shortlist is the quota walk's, so the quota bounds it and MMR chooses within it).  Each round takes the shortlist entry of
        the largest lam rel - (1 - lam) pen, rel the score scaled to [0, 1] over the shortlist and pen the largest cosine, 0 at the
        least, to a news already taken (lime_mmr_rows_f32; ``recommend.mmr_select`` states it on the host); lam = 1 is the plain
        slate.  The cosines are those of the rows of ``similarity`` (fp32 [n_news, E], E a multiple of 4, on the cache's device;
        default: the content columns of ``news_cache`` -- the whole row, under 'gated' its first half).  The positions and scores
        returned are the taken entries' in the order taken -- no longer descending --, -1 / -inf behind the last.  Refused
        (ValueError): an ``mmr_lambda`` outside [0, 1], a ``shortlist`` outside [k, 128], a ``similarity`` of another type or shape,
        and ``shortlist`` or ``similarity`` without ``mmr_lambda``.

        ``calibrate_lambda`` = lam (a real in [0, 1]; None: no calibration, today's launches and bits): the slate's topic mix follows
        the reader's own (calibrated re-ranking, Steck 2018).  The target p is the distribution of the groups -- ``calibrate_by``:
        'category' or 'topic' -- over the masked-in slots of the user's history, each slot weighing ``calibrate_weights[u, h]`` (fp32
        [U, H] on the cache's device; None: 1 each; a weight that is not finite or not > 0 removes the slot).  Among the ``shortlist``
        best (as under ``mmr_lambda``; under ``max_per_topic`` the quota walk's, so the two compose) each round takes the entry of
        the largest lam rel + (1 - lam) gain, gain the drop of KL(p || (1 - alpha) slate + alpha p) that the entry brings, scaled
        to [0, 1] by ln(1 / alpha), alpha = ``calibrate_alpha`` (lime_calibrate_rows_f32; ``recommend.calibrated_select`` states it
        on the host); lam = 1 is the plain slate, and so is a user without a masked-in history slot.  Returned as under
        ``mmr_lambda``.  Refused (ValueError): a ``calibrate_lambda`` that is no real in [0, 1], an unknown ``calibrate_by``, a
        ``calibrate_alpha`` that is no real in (0, 1), ``calibrate_weights`` of another type, shape, dtype or device, any of the three
        away from its default without ``calibrate_lambda``, ``calibrate_lambda`` together with ``mmr_lambda`` (one selection trades
        relevance against one of the two), a corpus of more than 8192 groups, and H > 128."""
        return serving.recommend(self, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_index, cand_freshness,
                                 cand_lifetime, k, n_src, pairs_per_pass, exclude_history, max_per_topic, quota_by, mmr_lambda=mmr_lambda,
                                 shortlist=shortlist, similarity=similarity, calibrate_lambda=calibrate_lambda, calibrate_by=calibrate_by,
                                 calibrate_alpha=calibrate_alpha, calibrate_weights=calibrate_weights)

    @torch.no_grad()
    def score_schedule(self, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_index, cand_freshness,
                       cand_lifetime, slot_offsets, n_src=None, pairs_per_pass=1 << 18, exclude_history=False):
        """``score_pool`` over a schedule of S time slots -> fp32 [S, U, C]: ``scores[s]`` is what ``score_pool`` returns when called
        with ``cand_freshness + slot_offsets[s]`` -- the pool as it will rank ``slot_offsets[s]`` from now, every candidate that much
        older: its freshness bucket moves, its remaining lifetime shrinks, past its lifetime it takes the expired penalty.
        ``slot_offsets``: float [S], S >= 1, in the unit of the freshness inputs, in any order, repeats allowed (the sum is made in
        fp32).  ``cand_lifetime``, the histories and their freshness / lifetime are as given for every slot: a lifetime belongs to the
        (user, topic), a history's freshness to the click.  Every other argument, its checks and its refusals are ``score_pool``'s.

        The user side does not depend on the slot and runs once per call (``match_operands`` once per pass of users).  By
        ``schedule_route(S, H)``:
          'single' (S = 1): ``score_pool`` itself, same launches, same bits;
          'factorised' -- the dot-product predictor where a candidate is A[news] + T[occurrence] with linear maps behind it
            (``occurrence_match_applicable()``) or A[news] alone (a baseline): the news-table products of the match run once per
            pair and every slot adds its occurrence's terms from per-group tables (lime_grouped_match_schedule_f32: one launch per
            pass for all slots; ``scores[s]`` agrees with ``score_pool`` to fp32 rounding, bit for bit on a baseline);
          'shared' -- 'gated', 'concat' with the identity projection, a LIME model under the MLP predictor, shapes beyond the
            kernel's limits, or LIME_SCHEDULE_MATCH=0: the existing match once per slot on the shared operands, bit for bit S
            ``score_pool`` calls;
          'expand' -- a baseline under the MLP predictor reads no time at all: one slot, repeated."""
        return serving.score_pool(self, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_index, cand_freshness,
                                  cand_lifetime, n_src, pairs_per_pass, exclude_history, slot_offsets=torch.as_tensor(slot_offsets))[0]

    @torch.no_grad()
    def recommend_schedule(self, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_index, cand_freshness,
                           cand_lifetime, slot_offsets, k, n_src=None, pairs_per_pass=1 << 18, exclude_history=False, max_per_topic=None,
                           quota_by='category', mmr_lambda=None, shortlist=None, similarity=None, calibrate_lambda=None,
                           calibrate_by='category', calibrate_alpha=0.01, calibrate_weights=None):
        """The k best news of the pool per user in every slot of a schedule: ``score_schedule`` (same arguments), then
        lime_topk_rows_f32 over the [S U, C] view of its scores (in chunks of slots that keep the kernel's 65535 rows) -> (positions
        int32 [S, U, k] into ``cand_index``, scores fp32 [S, U, k]); slot s holds what ``recommend`` returns at
        ``cand_freshness + slot_offsets[s]``, in its order and with its -1 / -inf for excluded or missing slots.  1 <= k <= 128.
        ``max_per_topic`` / ``quota_by``: as in ``recommend``, per (slot, user) row (lime_topk_rows_quota_f32 over the same view; the
        [U, C] mask of ``exclude_history`` is handed over once, row s U + u reads its row u).
        ``mmr_lambda`` / ``shortlist`` / ``similarity``: as in ``recommend``, per (slot, user) row.
        ``calibrate_lambda`` / ``calibrate_by`` / ``calibrate_alpha`` / ``calibrate_weights``: as in ``recommend``, per (slot, user) row;
        the [U, H] histories are handed over once, row s U + u reads user u's."""
        return serving.recommend(self, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_index, cand_freshness,
                                 cand_lifetime, k, n_src, pairs_per_pass, exclude_history, max_per_topic, quota_by, slot_offsets=slot_offsets,
                                 mmr_lambda=mmr_lambda, shortlist=shortlist, similarity=similarity, calibrate_lambda=calibrate_lambda,
                                 calibrate_by=calibrate_by, calibrate_alpha=calibrate_alpha, calibrate_weights=calibrate_weights)

    @torch.no_grad()
    def score_lists(self, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_offsets, cand_index, cand_freshness,
                    cand_lifetime, n_src=None, pairs_per_pass=1 << 18, exclude_history=False):
        """Scores fp32 [P], in list order, of U users against a candidate list of THEIR OWN each, from the news cache: user u's list is
        ``cand_index[cand_offsets[u]:cand_offsets[u + 1]]`` and ``scores[p]`` is the eval-mode score (N = 1, util.py:86-111) of the
        row (history u, candidate ``cand_index[p]``) -- what ``score_behaviors`` returns for that row with the same ``n_src``.

        ``corpus``, the four history arguments [U, H], ``n_src`` (default min(P, H + config.batch_size) under the CROWN user encoder,
        ignored otherwise) and ``exclude_history`` as in ``score_pool``; ``cand_offsets`` [U + 1], host or device (it is checked on the
        host); ``cand_index`` / ``cand_freshness`` / ``cand_lifetime`` [P].  The remaining lifetime follows config.lifetime_type.

        ``score_pool``'s passes over a plan of the lists: the pairs are grouped by (user, candidate topic) on the device
        (ops.list_plan -- its read of the lists' distinct-topic counts is the call's only synchronisation), the user side runs once
        per group and lime_grouped_match_f32 leaves each pair its two dot products per history slot.  The groups keep the regular
        ``hist_div`` layout: every user of a pass gets S_pass slots, the largest number of distinct topics among the pass's lists, and
        a list with fewer topics leaves slots whose refinement nobody reads.  Passes run over consecutive users and keep their pairs
        and their users x S_pass x H refined rows within ``pairs_per_pass`` each, one user a pass at the least.
        CNE has no per-news cache and is refused (ValueError).
        A baseline model (no LIME): the candidates are read in place from the cache through the pair's news id
        (lime_grouped_match_indexed_f32), with Q of every news of the cache computed once per call under the CROWN user encoder.
        A LIME model with LIME_OCCURRENCE_MATCH=1 where ``occurrence_match_applicable()`` holds: the cache itself is the news table, a
        pair's index its news id, and the occurrence is composed in the kernel as in ``score_pool``."""
        return serving.score_lists(self, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_offsets, cand_index,
                                   cand_freshness, cand_lifetime, n_src, pairs_per_pass, exclude_history)[0]

    @torch.no_grad()
    def recommend_lists(self, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_offsets, cand_index,
                        cand_freshness, cand_lifetime, k, n_src=None, pairs_per_pass=1 << 18, exclude_history=False, max_per_topic=None,
                        quota_by='category', mmr_lambda=None, shortlist=None, similarity=None, calibrate_lambda=None,
                        calibrate_by='category', calibrate_alpha=0.01, calibrate_weights=None):
        """The k best news of every user's OWN list, on the device: ``score_lists`` (same arguments), then lime_topk_segments_f32 ->
        (positions int32 [U, k] into the user's list -- candidate ``cand_index[cand_offsets[u] + positions[u, j]]`` --, scores fp32
        [U, k]) in ``recommend``'s order.  With ``exclude_history`` a candidate that sits in a masked-in slot of the user's history is
        never returned; the trailing slots of a list with fewer than k candidates left (all k of an empty list) hold position -1 and
        score -inf.  1 <= k <= 128.
        ``max_per_topic`` / ``quota_by``: as in ``recommend``, per list (lime_topk_segments_quota_f32).
        ``mmr_lambda`` / ``shortlist`` / ``similarity``: as in ``recommend``, per list.
        ``calibrate_lambda`` / ``calibrate_by`` / ``calibrate_alpha`` / ``calibrate_weights``: as in ``recommend``, per list."""
        return serving.recommend_lists(self, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_offsets, cand_index,
                                       cand_freshness, cand_lifetime, k, n_src, pairs_per_pass, exclude_history, max_per_topic, quota_by,
                                       mmr_lambda=mmr_lambda, shortlist=shortlist, similarity=similarity, calibrate_lambda=calibrate_lambda,
                                       calibrate_by=calibrate_by, calibrate_alpha=calibrate_alpha, calibrate_weights=calibrate_weights)

    @torch.no_grad()
    def explain_lists(self, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_offsets, cand_index,
                      cand_freshness, cand_lifetime, top=3, by='contribution', dense=False, n_src=None, pairs_per_pass=1 << 18):
        """Why each pair of ``score_lists`` (same arguments) scores what it scores -> ``serving.Explanation``(score [P], base [P],
        weight [P], slots int32 [P, top], values [P, top], attention [P, H] or None, contribution [P, H] or None), in the caller's
        pair order.  The model's score is a sum over the reader's history slots times the remaining-lifetime weight,
            score = (sum_h attention[h] (g[h] . candidate)) weight = sum_h contribution[h],
        so the explanation is exact, not a surrogate: ``score_lists``' plan, passes, user side and candidate tables, and a last launch
        that keeps the terms it sums (lime_grouped_match_explain_f32; ``recommend.explain_pairs`` states it on the host).  ``score`` has
        ``score_lists``' bits under the CROWN user encoder; under ATT / MHSA the pooled user vector sum_h beta[h] x[h] is taken apart
        the same way (attention = beta, the pool's weights; the sum runs in another order, so the score agrees to fp32 rounding).
        Under MHSA x[h] is the self-attended row of slot h: a contribution belongs to the click in the context of the others.

        ``slots``: the ``top`` history slots of largest contribution (``by`` 'contribution') or attention ('attention'), best first,
        ties lower slot first, among the slots ``hist_mask`` marks -- ``hist_index[u, slot]`` is the clicked news --, -1 (value 0)
        behind the last one; the attention itself is not masked, as in the reference.  ``dense``: the [P, H] terms as well.
        Refused (ValueError, before any launch): ``top`` outside 1 .. min(16, H), an unknown ``by``, ``by`` 'contribution' under the
        MLP click predictor (behind its ReLU the logit is no sum over the slots; 'attention' is served, with contribution None, weight
        1 and score = base from the existing MLP match), CNE, and everything ``score_lists`` refuses."""
        return serving.explain_lists(self, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_offsets, cand_index,
                                     cand_freshness, cand_lifetime, top, by, dense, n_src, pairs_per_pass)

    @torch.no_grad()
    def explain(self, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_index, cand_freshness, cand_lifetime,
                positions, top=3, by='contribution', dense=False, n_src=None, pairs_per_pass=1 << 18):
        """``explain_lists`` for a slate: ``positions`` int [U, k] are the positions into ``cand_index`` that ``recommend`` returned
        for the same pool arguments (or one slot of ``recommend_schedule``'s, with that slot's offset added to ``cand_freshness``)
        -> the same record shaped [U, k, ...].  ``score`` has the bits of ``recommend``'s scores (``n_src`` defaults as there); an
        unfilled entry (-1) comes back as score -inf, slots -1."""
        return serving.explain(self, news_cache, corpus, hist_index, hist_mask, user_freshness, user_lifetime, cand_index, cand_freshness,
                               cand_lifetime, positions, top, by, dense, n_src, pairs_per_pass)

    @torch.no_grad()
    def evaluate_slates(self, behaviors, indices, labels, settings, k=10, **kw):
        """``util.evaluate_slates_on_device`` of this model: the dev split scored once, then every selection setting of ``settings``
        (``recommend_lists``' ``max_per_topic`` / ``mmr_lambda`` ..) evaluated on those scores -- nDCG@k, RR, hit, recall against
        intra-list distance, distinct topics, fill and a value of the caller's -> (the pass's four metrics, one dict per setting).
        ``calibration='category'`` / ``'topic'`` adds every setting's mean miscalibration against the impression's history."""
        from . import util
        return util.evaluate_slates_on_device(self, behaviors, indices, labels, settings, k=k, **kw)

    def _score_from_recurrence(self, behaviors, rows, rc, n_src, rows_per_forward):
        """score_behaviors under CNE from the recurrence cache: one encoder pass over the R candidates and the R . H history news of the
        rows (flat order: candidates, then histories, as ``_forward_impl`` encodes them), paired per chunk of rows_per_forward rows,
        then the match per stretch of rows with one source count."""
        b = behaviors
        ne, ue, c = self.news_encoder, self.user_encoder, b.corpus
        if self.training:
            raise RuntimeError('score_behaviors is the eval-mode function: call model.eval() first')
        if not ne.base_news_encoder.cache_is_current(rc):
            raise RuntimeError('the recurrence cache was built from other parameter values (word table, LSTMs, title_H / content_H): '
                               'rebuild it with build_recurrence_cache after the weights change')
        dev = rc.title.lens.device
        rows = torch.as_tensor(rows, device=dev).long().reshape(-1)
        R, H = rows.numel(), b.hist_index.shape[1]
        p = R if rows_per_forward is None else int(rows_per_forward)
        if p < 1:
            raise ValueError('rows_per_forward must be positive')
        hist_idx, cand_idx = b.hist_index[rows], b.cand_index[rows]                       # [R, H], [R, 1]
        idx = torch.cat([cand_idx.reshape(-1), hist_idx.reshape(-1)])                     # int32 [R + R H]
        flat = idx.long()
        chunk = torch.arange(R, device=dev) // p                                          # the reference forward a row belongs to
        calls = torch.cat([2 * chunk, 2 * chunk.repeat_interleave(H) + 1])                # ... and its two encoder calls: candidates, history
        cat_all, sub_all = c.news_category[flat], c.news_subCategory[flat]
        rep = ne.encode_flat(None, c.news_title_mask[flat], None, newsEncoders._i32(cat_all), newsEncoders._i32(sub_all),
                             torch.cat([b.cand_freshness[rows].reshape(-1), b.user_freshness[rows].reshape(-1)]),
                             torch.cat([b.cand_lifetime[rows].reshape(-1), b.user_lifetime[rows].reshape(-1)]),
                             content_mask=c.news_abstract_mask[flat], pair_groups=calls, recurrence=(rc, idx))
        cand, hist = rep[:R].view(R, 1, -1), rep[R:].view(R, H, -1)
        remaining = self._remaining_lifetime(b, rows, cand_idx).view(R, 1)
        hist_mask = b.hist_mask[rows]
        logits = torch.empty(R, dtype=torch.float32, device=dev)
        full = (R // p) * p
        for r0, r1, n in ((0, full, p), (full, R, R - full)):                             # the full chunks, then the short last one
            if r1 == r0:
                continue
            src = n_src
            if src is None:
                src = min(n, H + ue.user_node_embedding.shape[0]) if hasattr(ue, 'user_node_embedding') else n
            out = self._row_logits(hist[r0:r1], cat_all[r0:r1].view(-1, 1), sub_all[r0:r1].view(-1, 1),
                                   cat_all[R + r0 * H:R + r1 * H].view(-1, H), sub_all[R + r0 * H:R + r1 * H].view(-1, H), hist_mask[r0:r1],
                                   cand[r0:r1], remaining[r0:r1], n_src=src)
            logits[r0:r1] = out.view(-1)
        return logits

    def _forward_impl(self, user_ID, user_category, user_subCategory, user_title_text, user_title_mask, user_title_entity,
                      user_content_text, user_content_mask, user_content_entity, user_freshness, user_user_topic_lifetime,
                      user_history_mask, user_history_graph, user_history_category_mask, user_history_category_indices,
                      news_category, news_subCategory, news_title_text, news_title_mask, news_title_entity, news_content_text,
                      news_content_mask, news_content_entity, news_freshness, news_user_topic_lifetime, remaining_lifetime):
        if not self.training:                                                    # model.py:158-169
            news_category = news_category.unsqueeze(1)
            news_subCategory = news_subCategory.unsqueeze(1)
            news_title_text = news_title_text.unsqueeze(1)
            news_title_mask = news_title_mask.unsqueeze(1)
            news_content_text = news_content_text.unsqueeze(1)
            if self.reads_content_mask:
                news_content_mask = news_content_mask.unsqueeze(1)
            if self.reads_title_entity:
                news_title_entity = news_title_entity.unsqueeze(1)
            news_freshness = news_freshness.unsqueeze(1)
            news_user_topic_lifetime = news_user_topic_lifetime.unsqueeze(1)
            remaining_lifetime = remaining_lifetime.unsqueeze(1)
        if not self.reads_content_mask:
            news_content_mask = user_content_mask = None
        if not self.reads_title_entity:
            news_title_entity = user_title_entity = None
        with torch.no_grad():
            # candidate-aware attention weights depend on topic ids and the history mask only: side stream, joined below
            main = torch.cuda.current_stream()
            side2 = newsEncoders._side_stream(user_category.device, 2)
            side2.wait_stream(main)
            with torch.cuda.stream(side2):
                agg = self.user_encoder.attention_weights(news_category, news_subCategory, user_category, user_subCategory,
                                                          user_history_mask)
            news_representation, history_embedding = self.news_encoder.encode_many([
                (news_title_text, news_title_mask, news_content_text, news_category, news_subCategory, news_freshness,
                 news_user_topic_lifetime, news_content_mask, news_title_entity),     # model.py:171-173
                (user_title_text, user_title_mask, user_content_text, user_category, user_subCategory, user_freshness,
                 user_user_topic_lifetime, user_content_mask, user_title_entity)])    # userEncoders.py:110-112
            main.wait_stream(side2)
            logits = self._row_logits(history_embedding, news_category, news_subCategory, user_category, user_subCategory,
                                      user_history_mask, news_representation, remaining_lifetime.float(), agg=agg)   # model.py:174-184
        return logits


def _clears_auxiliary_loss(fn):
    """An entry that scores, caches or serves leaves no category-prediction term behind: ``news_encoder.auxiliary_loss`` is None after
    it, whatever an earlier training forward stored there."""
    @functools.wraps(fn)
    def entry(self, *args, **kwargs):
        self.news_encoder.auxiliary_loss = None
        return fn(self, *args, **kwargs)
    return entry


for _name in ('score_impressions', 'build_news_cache', 'build_recurrence_cache', 'score_behaviors', 'score_pool', 'recommend',
              'score_schedule', 'recommend_schedule', 'score_lists', 'recommend_lists'):
    setattr(Model, _name, _clears_auxiliary_loss(getattr(Model, _name)))
