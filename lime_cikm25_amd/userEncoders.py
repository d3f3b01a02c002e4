"""Drop-in user encoders of the scoring path: CROWN (reference userEncoders.py:16-175), ATT (:529-558) and MHSA (:447-490)."""
import math

import torch
import torch.nn as nn

from . import ops
from .layers import Attention, CandidateAware_ClickedNewsAttention, MultiHeadAttention


class SAGEConv(nn.Module):
    """Parameter holder with PyG's SAGEConv names: ``lin_l`` (bias) on the aggregate, ``lin_r`` (no bias) on the root."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.lin_l = nn.Linear(in_channels, out_channels, bias=True)
        self.lin_r = nn.Linear(in_channels, out_channels, bias=False)


class GraphSAGE(nn.Module):
    """``torch_geometric.nn.GraphSAGE(in, hidden, num_layers=1, out_channels=...)`` as the reference constructs it
    (userEncoders.py:54-58): one SAGEConv, nothing after it.  PyG is an absent, un-versioned dependency; the
    aggregation is restated from its documented semantics (parity unpinned at this boundary)."""

    def __init__(self, in_channels, hidden_channels, num_layers, out_channels=None, dropout=0.0):
        super().__init__()
        if num_layers != 1:
            raise NotImplementedError('the reference uses num_layers = 1 (userEncoders.py:56)')
        self.convs = nn.ModuleList([SAGEConv(in_channels, out_channels or hidden_channels)])

    def forward_closed_form(self, hist, user_nodes, n_src):
        """hist [B, H, D] (node slots 0..H-1 of every row), user_nodes [n_user, D] (slots H..), n_src = rows per forward.

        create_bipartite_graph (userEncoders.py:91-98) yields edges (u -> i) for u < n_src, i < H applied along the node
        axis of each row, so  out[b, i] = lin_l(mean_{u < n_src} X[b, u]) + lin_r(X[b, i])  for the H history slots that
        survive the slice at :157.
        """
        B, H, D = hist.shape
        conv = self.convs[0]
        flat = hist.reshape(B * H, D)
        m = ops.sage_mean(flat, user_nodes.contiguous(), B, H, n_src, D)
        l = ops.linear(m, conv.lin_l.weight, conv.lin_l.bias)
        g = ops.linear(flat, conv.lin_r.weight, None, res=l, res_div=H)
        return g.view(B, H, D)


class _NoParams(nn.Module):
    """LightGCN / LGConv are constructed and never called by the reference (userEncoders.py:59-62); they hold no
    checkpoint entries."""


class UserEncoder(nn.Module):
    def __init__(self, news_encoder, config):
        super().__init__()
        self.news_embedding_dim = news_encoder.news_embedding_dim
        self.news_encoder = news_encoder
        self.device = torch.device('cuda')
        self.auxiliary_loss = None
        self.word_embedding_dim = config.word_embedding_dim
        self.batch_size = config.batch_size


class CROWN(UserEncoder):
    """userEncoders.py:49-175: history encoding -> candidate-aware clicked-news attention -> GraphSAGE step ->
    history-vs-candidate attention.  ``forward`` keeps the reference's 18-argument signature."""

    def __init__(self, news_encoder, config):
        super().__init__(news_encoder, config)
        self.attention_dim = config.attention_dim
        self.graph_sage = GraphSAGE(in_channels=self.news_embedding_dim, hidden_channels=self.news_embedding_dim, num_layers=1,
                                    out_channels=self.news_embedding_dim, dropout=config.dropout_rate)
        self.lightgcn = _NoParams()
        self.lgconv = _NoParams()
        self.user_node_embedding = nn.Parameter(torch.zeros([config.batch_size, self.news_embedding_dim]))
        self.K = nn.Linear(self.news_embedding_dim, self.attention_dim, bias=False)
        self.Q = nn.Linear(self.news_embedding_dim, self.attention_dim, bias=True)
        self.max_history_num = config.max_history_num
        self.attention_scalar = math.sqrt(float(self.attention_dim))
        self.affine = nn.Linear(self.news_embedding_dim, self.news_embedding_dim, bias=True)      # unused upstream (:171)
        self.dropout_rate = config.dropout_rate
        self.dropout = nn.Dropout(p=config.dropout_rate, inplace=True)
        self.dropout_ = nn.Dropout(p=config.dropout_rate, inplace=False)
        self.use_candidate_aware_attn = config.use_candidate_ware_clicked_news_attention
        if self.use_candidate_aware_attn:
            self.candidate_aware_attn = CandidateAware_ClickedNewsAttention(config, news_encoder)

    def initialize(self):
        nn.init.zeros_(self.user_node_embedding)
        nn.init.xavier_uniform_(self.K.weight)
        nn.init.xavier_uniform_(self.Q.weight)
        nn.init.zeros_(self.Q.bias)
        nn.init.xavier_uniform_(self.affine.weight, gain=nn.init.calculate_gain('relu'))
        nn.init.zeros_(self.affine.bias)
        if self.use_candidate_aware_attn:
            self.candidate_aware_attn.initialize()

    def _topic(self, category, subCategory):
        """userEncoders.py:103-105 / :115-117: LIME's own frozen tables + category_affine."""
        ne = self.news_encoder
        shape = category.shape
        cat = category.reshape(-1)
        sub = subCategory.reshape(-1)
        cat = cat if cat.dtype == torch.int32 else cat.to(torch.int32)
        sub = sub if sub.dtype == torch.int32 else sub.to(torch.int32)
        rep = ops.topic_rep(cat.contiguous(), sub.contiguous(), ne.category_embedding.weight, ne.subCategory_embedding.weight,
                            ne.category_affine.weight, ne.category_affine.bias)
        return rep.view(*shape, -1)

    def attention_weights(self, category, subCategory, user_category, user_subCategory, user_history_mask, hist_div=1):
        """The candidate-aware attention weights agg [B, H] (layers.py:66-81).  They depend on the topic ids and the
        history mask only -- not on any news embedding -- so the model computes them on a side stream while the token
        encoders run."""
        if not self.use_candidate_aware_attn:
            return None
        if self.training and self.candidate_aware_attn.dropout.p > 0:
            raise NotImplementedError('attention_weights() is the scoring kernel: in training mode the layer\'s p = 0.2 dropout '
                                      '(layers.py:36,74) runs on the differentiable path (user_encoder(...) / Model.forward)')
        cand_topic = self._topic(category, subCategory)
        hist_topic = self._topic(user_category, user_subCategory)
        return self.candidate_aware_attn.attention_weights(hist_topic, cand_topic, user_history_mask, hist_div=hist_div)

    def match(self, history_embedding, category, subCategory, user_category, user_subCategory, user_history_mask,
              candidate_news_representation, remaining_lifetime=None, weighting=None, agg=None, n_src=None, hist_div=1,
              gate_y=None):
        """Everything after the history has been encoded (userEncoders.py:103-105, :114-169).

        Returns (user_representation [B, N, D], logits [B, N] or None).  With ``weighting`` (the model's
        RemainingLifetimeWeighting) the dot-product match and the lifetime weight are fused into the last kernel.
        ``agg``: precomputed ``attention_weights(...)``.  ``n_src``: how many node slots the GraphSAGE mean runs over
        (Q7: the reference uses the number of rows of the forward; default B).
        ``hist_div`` > 1 (Model.score_impressions): ``history_embedding`` is [B / hist_div, H, D] -- ONE copy of a history for the
        hist_div consecutive rows (candidates) that share it, and so are the history's topic ids and mask ([B / hist_div, H]); the
        candidates' own ids and ``agg`` (if given) are per row [B, ...].
        ``gate_y``: ``gate_projection(history_embedding)`` computed by the caller (one GEMM over all passes' histories).
        """
        if self.training and (self.dropout_rate > 0 or (self.use_candidate_aware_attn and self.candidate_aware_attn.dropout.p > 0)):
            raise NotImplementedError('match() is the fused scoring kernel chain: with training-mode dropouts active (userEncoders.py:121, '
                                      'layers.py:74) call user_encoder(...) or Model.forward, which take the differentiable path')
        Bh, H, D = history_embedding.shape
        B = Bh * hist_div
        N = candidate_news_representation.shape[1]
        cand = candidate_news_representation.contiguous()
        g, kp, qp = self.match_operands(history_embedding, category, subCategory, user_category, user_subCategory, user_history_mask,
                                        agg=agg, n_src=n_src, hist_div=hist_div, gate_y=gate_y, cand=cand.view(B * N, D))
        w = weighting
        user, logits = ops.interest_match(
            kp, qp, g.reshape(-1), cand.reshape(-1), remaining_lifetime, B, N, H, self.attention_dim, D,
            1.0 / self.attention_scalar,
            w.alpha if w is not None else 0.0, w.beta if w is not None else 0.0,
            bool(w.use_remaining_lifetime_weighting) if w is not None else False,
            bool(w.use_expired_penalty) if w is not None else False,
            want_logits=w is not None, want_user=True)
        return user, logits

    def match_operands(self, history_embedding, category, subCategory, user_category, user_subCategory, user_history_mask, agg=None,
                       n_src=None, hist_div=1, gate_y=None, cand=None):
        """Everything of ``match`` up to the operands of its last kernel: (g [B, H, D], the GraphSAGE step over the refined history,
        kp [B H, A] = K g, qp = Q(cand) [rows of cand, A] or None).  The B = Bh * hist_div rows are ``match``'s rows -- or, from
        Model.score_pool, the (user, candidate topic) GROUPS, user-major with hist_div topics per user: ``category`` / ``subCategory``
        [B, 1] then hold a group's topic, and ``cand`` is left out (the pairs' Q runs once per pass, outside)."""
        Bh, H, D = history_embedding.shape
        B = Bh * hist_div
        n_src = B if n_src is None else n_src
        caa = self.candidate_aware_attn if self.use_candidate_aware_attn else None
        fused = caa is not None and caa.use_residual_connection and D <= 512
        main = torch.cuda.current_stream()
        qp = side6 = None
        if fused and gate_y is None and cand is not None:
            # Q(candidates) (:162) and gate_proj(history) (layers.py:87) do not depend on each other: one grouped launch
            qp, gate_y = ops.linear_group([dict(a=cand, w=self.Q.weight, bias=self.Q.bias),
                                           dict(a=history_embedding.reshape(Bh * H, D), w=caa.gate_proj.weight, bias=None)])
        elif cand is not None:
            # the candidate side of the match (:162) needs the candidates only: branch 6, beside the history chain
            from .newsEncoders import _side_stream
            side6 = _side_stream(cand.device, 6)
            side6.wait_stream(main)
            with torch.cuda.stream(side6):
                qp = ops.linear(cand, self.Q.weight, self.Q.bias)                                             # :162
        if caa is not None and agg is None:
            # (hist_div > 1: user_category / user_subCategory / user_history_mask are [B / hist_div, H] -- one history per hist_div rows)
            agg = self.attention_weights(category, subCategory, user_category, user_subCategory, user_history_mask, hist_div=hist_div)
        conv = self.graph_sage.convs[0]
        if fused:
            # gate_proj sees the history alone (the row scale commutes: layers.py:85-87), so it runs once per HISTORY; the gated
            # residual + LayerNorm of each row's H history rows and the SAGEConv mean over them are one launch, which reads a
            # shared history through row / hist_div (no per-candidate copies) and takes the user-node part of the mean -- the same
            # vector for every row -- as one precomputed sum                                                  :121,:151-157
            hist = history_embedding.reshape(Bh * H, D)
            y = gate_y if gate_y is not None else ops.linear(hist, caa.gate_proj.weight, None)
            node_const = self.user_node_embedding[:n_src - H].sum(dim=0) if n_src > H else None
            refined, m = ops.gate_ln_sage(y, hist, agg.reshape(-1), caa.gate_proj.bias, caa.layernorm.weight, caa.layernorm.bias,
                                          caa.layernorm.eps, B, H, D, hist_div, n_src, node_const)
            l = ops.linear(m, conv.lin_l.weight, conv.lin_l.bias)
            g = ops.linear(refined, conv.lin_r.weight, None, res=l, res_div=H).view(B, H, D)
        else:
            if hist_div > 1:
                history_embedding = history_embedding.repeat_interleave(hist_div, dim=0)
            if caa is not None:
                history_embedding = caa.refine(history_embedding, agg)
            g = self.graph_sage.forward_closed_form(history_embedding, self.user_node_embedding, n_src=n_src)   # :121,:151-157
        kp = ops.linear(g.view(B * H, D), self.K.weight, None)                                               # :161
        if side6 is not None:
            main.wait_stream(side6)
        return g, kp, qp

    def gate_projection(self, history_embedding):
        """W_g x of the candidate-aware attention's gate (layers.py:87) for histories [*, H, D] -> [* H, D], or None when ``match``
        does not take the fused path."""
        caa = self.candidate_aware_attn if self.use_candidate_aware_attn else None
        D = history_embedding.shape[-1]
        if caa is None or not caa.use_residual_connection or D > 512:
            return None
        return ops.linear(history_embedding.reshape(-1, D), caa.gate_proj.weight, None)

    def forward(self, user_title_text, user_title_mask, user_title_entity, user_content_text, user_content_mask,
                user_content_entity, category, subCategory, user_category, user_subCategory, user_history_mask,
                user_history_graph, user_history_category_mask, user_history_category_indices, user_embedding,
                candidate_news_representation, user_freshness, user_user_topic_lifetime):
        history_embedding = self.news_encoder(user_title_text, user_title_mask, user_title_entity, user_content_text,
                                              user_content_mask, user_content_entity, user_category, user_subCategory,
                                              user_embedding, user_freshness, user_user_topic_lifetime)        # :110-112
        from . import training
        p_any = max(self.dropout_rate, self.candidate_aware_attn.dropout.p if self.use_candidate_aware_attn else 0.0)
        if training.wants_train_path(self, p_any):
            # training mode (trainer.py:87): the differentiable path; the candidate representation may carry a graph
            i32 = lambda t: (t if t.dtype == torch.int32 else t.to(torch.int32)).contiguous()
            return training.user_representation(self, history_embedding, candidate_news_representation.float(), i32(category),
                                                i32(subCategory), i32(user_category), i32(user_subCategory),
                                                user_history_mask.contiguous())
        user, _ = self.match(history_embedding, category, subCategory, user_category, user_subCategory, user_history_mask,
                             candidate_news_representation)
        return user


class _PooledUser(UserEncoder):
    """What ATT and MHSA share (userEncoders.py:447-490, :529-558): optional candidate-aware refinement of the history, an encoder-specific
    step over the refined rows (``_sequence``), additive attention pooling WITHOUT a mask (:489, :557 -- padded slots take part in the
    softmax) into ONE user vector per row, returned over the news_num axis.  The topic embeddings of the candidate-aware attention are
    LIME's frozen ``category_embedding`` rows alone (:470,482 / :546,554): no ``category_affine``, no subcategory."""

    p_sequence = 0.0                 # probability of the training-mode dropout inside ``_sequence``

    def _init_candidate_aware(self, news_encoder, config):
        self.use_candidate_aware_attn = config.use_candidate_ware_clicked_news_attention
        if self.use_candidate_aware_attn:
            self.candidate_aware_attn = CandidateAware_ClickedNewsAttention(config, news_encoder)

    def _topic(self, category):
        table = self.news_encoder.category_embedding.weight
        idx = category.reshape(-1)
        idx = (idx if idx.dtype == torch.int32 else idx.to(torch.int32)).contiguous()
        out = torch.empty((idx.numel(), table.shape[1]), dtype=torch.float32, device=table.device)
        ops.gather_rows(idx, table, out)
        return out.view(*category.shape, -1)

    def _train_dropouts(self):
        p_caa = self.candidate_aware_attn.dropout.p if self.use_candidate_aware_attn else 0.0
        return max(self.p_sequence, p_caa)

    def attention_weights(self, category, subCategory, user_category, user_subCategory, user_history_mask, hist_div=1):
        """The candidate-aware attention weights agg [B, H] (layers.py:66-81) from the category ids and the history mask alone (the
        model computes them on a side stream); ``subCategory`` / ``user_subCategory`` are accepted and not read."""
        if not self.use_candidate_aware_attn:
            return None
        if self.training and self.candidate_aware_attn.dropout.p > 0:
            raise NotImplementedError('attention_weights() is the scoring kernel: in training mode the layer\'s p = 0.2 dropout '
                                      '(layers.py:36,74) runs on the differentiable path (user_encoder(...) / Model.forward)')
        return self.candidate_aware_attn.attention_weights(self._topic(user_category), self._topic(category), user_history_mask,
                                                           hist_div=hist_div)

    def gate_projection(self, history_embedding):
        """W_g x of the candidate-aware attention's gate (layers.py:87) for histories [*, H, D] -> [* H, D], or None when ``match``
        does not take the one-launch refinement."""
        caa = self.candidate_aware_attn if self.use_candidate_aware_attn else None
        D = history_embedding.shape[-1]
        if caa is None or not caa.use_residual_connection or D > 512:
            return None
        return ops.linear(history_embedding.reshape(-1, D), caa.gate_proj.weight, None)

    def _sequence(self, x, mask, rows, H, taps=None):
        """x [rows * H, D] refined history rows -> the rows the attention pools (same shape); mask u8 / bool [rows, H]."""
        raise NotImplementedError

    def match(self, history_embedding, category, subCategory, user_category, user_subCategory, user_history_mask,
              candidate_news_representation, remaining_lifetime=None, weighting=None, agg=None, n_src=None, hist_div=1,
              gate_y=None, taps=None):
        """Everything after the history has been encoded.  Returns (user_representation [B, N, D], logits [B, N] or None), the
        interface of ``CROWN.match``; ``n_src`` is CROWN's (GraphSAGE) and is ignored.  ``hist_div`` > 1: ``history_embedding``,
        the history's category ids and mask hold ONE history for hist_div consecutive candidate rows; it is read through
        row / hist_div by the refinement kernel and never repeated in memory before it.  The refined rows do differ per
        candidate row (through ``agg``) and are materialised: with the tanh hidden state (D + A) * 4 bytes per (row, slot) under ATT, the caller bounds
        the rows of a call (Model.score_impressions: rows_per_pass).  ``taps``: optional dict that receives the intermediate
        tensors (tests)."""
        if self.training and self._train_dropouts() > 0:
            raise NotImplementedError('match() is the fused scoring kernel chain: with training-mode dropouts active (userEncoders.py:487, '
                                      'layers.py:74) call user_encoder(...) or Model.forward, which take the differentiable path')
        Bh, H, D = history_embedding.shape
        B = Bh * hist_div
        N = candidate_news_representation.shape[1]
        cand = candidate_news_representation.contiguous()
        x, hidden, rows = self._pool_inputs(history_embedding, category, subCategory, user_category, user_subCategory, user_history_mask,
                                            agg, hist_div, gate_y, taps)
        n_cand = B * N // rows
        att = self.attention
        w = weighting
        rl = remaining_lifetime.reshape(rows, n_cand) if (w is not None and remaining_lifetime is not None) else None
        user, logits = ops.pool_match(
            hidden, att.affine2.weight.view(-1), x, rows, H, cand=cand.view(rows, n_cand, D) if w is not None else None, remaining=rl,
            alpha=w.alpha if w is not None else 0.0, beta=w.beta if w is not None else 0.0,
            use_weight=bool(w.use_remaining_lifetime_weighting) if w is not None else False,
            use_penalty=bool(w.use_expired_penalty) if w is not None else False,
            mask=None, want_user=True, want_logits=w is not None)                                          # layers.py:289-299, util.py:23-49
        if rows != B:
            user = user.unsqueeze(1).expand(Bh, hist_div, D).reshape(B, D)
        return user.unsqueeze(1).expand(B, N, D), (logits.view(B, N) if logits is not None else None)

    def match_operands(self, history_embedding, category, subCategory, user_category, user_subCategory, user_history_mask, agg=None,
                       n_src=None, hist_div=1, gate_y=None):
        """Everything of ``match`` up to the dot product: the pooled user vector of every row, [rows, D] -- rows = Bh * hist_div with the
        candidate-aware attention (from Model.score_pool the (user, candidate category) groups, user-major; ``category`` [rows, 1] holds
        a group's category), rows = Bh without it (one vector per history).  The match of a vector with its candidates is CROWN's last
        kernel with a history of ONE row (lime_grouped_match_f32, H = 1).  ``n_src`` is CROWN's and is ignored."""
        H = history_embedding.shape[1]
        x, hidden, rows = self._pool_inputs(history_embedding, category, subCategory, user_category, user_subCategory, user_history_mask,
                                            agg, hist_div, gate_y, None)
        user, _ = ops.pool_match(hidden, self.attention.affine2.weight.view(-1), x, rows, H, mask=None, want_user=True, want_logits=False)
        return user

    def _pool_inputs(self, history_embedding, category, subCategory, user_category, user_subCategory, user_history_mask, agg, hist_div,
                     gate_y, taps):
        """The rows the attention pools and their tanh hidden state: (x [rows H, D], hidden [rows H, A], rows)."""
        Bh, H, D = history_embedding.shape
        B = Bh * hist_div
        caa = self.candidate_aware_attn if self.use_candidate_aware_attn else None
        mask = user_history_mask
        if caa is None:
            # no refinement: the hist_div rows of a history share ONE user vector -- pool each history once, against its
            # hist_div * N candidates
            rows = Bh
            x = history_embedding.reshape(Bh * H, D)
        else:
            rows = B
            if agg is None:
                agg = self.attention_weights(category, subCategory, user_category, user_subCategory, user_history_mask, hist_div=hist_div)
            if caa.use_residual_connection and D <= 512:
                y = gate_y if gate_y is not None else ops.linear(history_embedding.reshape(Bh * H, D), caa.gate_proj.weight, None)
                # gated residual + LayerNorm of each row's H history rows in one launch, reading a shared history through row / hist_div
                # (the kernel's GraphSAGE column mean is CROWN's and is dropped)
                x, _ = ops.gate_ln_sage(y, history_embedding.reshape(Bh * H, D), agg.reshape(-1), caa.gate_proj.bias, caa.layernorm.weight,
                                        caa.layernorm.bias, caa.layernorm.eps, B, H, D, hist_div, H, None)
            else:
                hist = history_embedding if hist_div == 1 else history_embedding.repeat_interleave(hist_div, dim=0)
                x = caa.refine(hist, agg).view(B * H, D)
            if hist_div > 1:
                mask = mask.repeat_interleave(hist_div, dim=0)
        if taps is not None:
            taps['hist_refined'] = x.view(rows, H, D)
        x = self._sequence(x, mask, rows, H, taps)
        att = self.attention
        hidden = ops.linear(x, att.affine1.weight, att.affine1.bias, act='tanh')                           # layers.py:288
        return x, hidden, rows

    def forward(self, user_title_text, user_title_mask, user_title_entity, user_content_text, user_content_mask,
                user_content_entity, category, subCategory, user_category, user_subCategory, user_history_mask,
                user_history_graph, user_history_category_mask, user_history_category_indices, user_embedding,
                candidate_news_representation, user_freshness, user_user_topic_lifetime):
        history_embedding = self.news_encoder(user_title_text, user_title_mask, user_title_entity, user_content_text,
                                              user_content_mask, user_content_entity, user_category, user_subCategory,
                                              user_embedding, user_freshness, user_user_topic_lifetime)
        from . import training
        if training.wants_train_path(self, self._train_dropouts()):
            i32 = lambda t: (t if t.dtype == torch.int32 else t.to(torch.int32)).contiguous()
            return training.user_representation(self, history_embedding, candidate_news_representation.float(), i32(category),
                                                i32(subCategory), i32(user_category), i32(user_subCategory),
                                                user_history_mask.contiguous())
        user, _ = self.match(history_embedding, category, subCategory, user_category, user_subCategory, user_history_mask,
                             candidate_news_representation)
        return user


class ATT(_PooledUser):
    """userEncoders.py:529-558 (NAML's user encoder): additive attention over the (candidate-aware refined) history."""

    def __init__(self, news_encoder, config):
        super().__init__(news_encoder, config)
        self.attention = Attention(self.news_embedding_dim, config.attention_dim)
        self._init_candidate_aware(news_encoder, config)

    def initialize(self):
        self.attention.initialize()
        if self.use_candidate_aware_attn:
            self.candidate_aware_attn.initialize()

    def _sequence(self, x, mask, rows, H, taps=None):
        return x


class MHSA(_PooledUser):
    """userEncoders.py:447-490 (NRMS's user encoder): masked multi-head self-attention over the refined history, ``affine`` + dropout +
    ReLU, then ATT's pool.  The dropout behind ``affine`` is ``F.dropout(..., training=self.training)`` with no ``p`` (:487): 0.5 in
    training mode whatever config.dropout_rate says.  The self-attention's view (layers.py:224-226) fixes the history length to
    config.max_history_num."""

    p_sequence = 0.5

    def __init__(self, news_encoder, config):
        super().__init__(news_encoder, config)
        self.multiheadAttention = MultiHeadAttention(config.head_num, self.news_embedding_dim, config.max_history_num,
                                                     config.max_history_num, config.head_dim, config.head_dim)
        self.affine = nn.Linear(config.head_num * config.head_dim, self.news_embedding_dim, bias=True)
        self.attention = Attention(self.news_embedding_dim, config.attention_dim)
        self._init_candidate_aware(news_encoder, config)

    def initialize(self):
        self.multiheadAttention.initialize()
        nn.init.xavier_uniform_(self.affine.weight, gain=nn.init.calculate_gain('relu'))
        nn.init.zeros_(self.affine.bias)
        self.attention.initialize()
        if self.use_candidate_aware_attn:
            self.candidate_aware_attn.initialize()

    def check_history_length(self, H):
        mha = self.multiheadAttention
        if H != mha.len_q:
            raise ValueError('the MHSA user encoder attends over exactly config.max_history_num = %d history slots (layers.py:224-226), '
                             'got a history of %d' % (mha.len_q, H))

    def _sequence(self, x, mask, rows, H, taps=None):
        self.check_history_length(H)
        mha = self.multiheadAttention
        c = mha.attend(mha.project(x), rows, H, mask.reshape(-1))                                           # :486, layers.py:222-238
        h = ops.linear(c, self.affine.weight, self.affine.bias, act='relu')                                 # :487 (eval: no dropout)
        if taps is not None:
            taps['self_attention'] = c.view(rows, H, -1)
            taps['post_affine'] = h.view(rows, H, -1)
        return h
