"""The training step of LIME-CROWN-CROWN: a differentiable ``Model.forward`` for
``loss.backward()`` (reference trainer.py:131-148), and the native step that replaces trainer.py:143-148 --
``zero_grad / backward / clip_grad_norm_ / Adam.step`` -- plus the gradient all-reduce of a data-parallel run.

Where the arithmetic runs
  * token encoders (word gather + positional table + post-LN encoder layer + mean pool, 97 % of a step's FLOPs):
    hand-written HIP forward AND backward behind one autograd node (``_TokenEncoder``, over ``_layer_forward`` /
    ``_layer_backward``, which the per-layer node of the two-layer path shares): the forward of the scoring path
    with the LayerNorm rstd kept, backward = LayerNorm / attention / ReLU backward kernels, the MFMA weight-gradient GEMM,
    input gradients on lime_linear_f32 with transposed weights, word-table scatter-add.
  * every nn.Linear of the tail and the user encoder: ``_Linear`` (HIP GEMMs forward and backward).
  * the fused tail kernels of the scoring path with hand-written backward kernels (csrc/tail_backward_f32.hip): intent attention
    + cosine similarity + concat, gated residual + LayerNorm, history-vs-candidate attention + dot product + lifetime weight.
  * candidate-aware attention weights (per-head softmax with the layer's p = 0.2 dropout, query-norm softmax, aggregate
    softmax) forward and backward in one kernel per impression row (cand_attn_train_kernel).
  * still torch ops with torch's autograd: the GraphSAGE mean, a few concatenations and the two feature-fusion dropouts.

Dropout (the reference trains with dropout_rate 0.2): the six dropouts inside a token encoder run on the dropout kernels
with counter-based masks (csrc/dropout.h; torch's Philox stream is not reproduced -- the arithmetic is pinned against a torch
statement of the layer fed with the same masks, tests/test_dropout_gpu.py), and so does the hard-coded p = 0.2 of the
candidate-aware attention.  The dropouts left in the torch glue (feature_fusion, user_node_embedding) use torch's generator.
"""
import math

import torch
import torch.nn as nn

from . import distributed, ops


# ---------------------------------------------------------------------------------------------------------------------
# autograd nodes over the HIP kernels
# ---------------------------------------------------------------------------------------------------------------------
class _Linear(torch.autograd.Function):
    """y = act(x W^T + b) on lime_linear_f32; backward: dX on lime_linear_f32 (W^T as the weight operand), dW on the
    weight-gradient GEMM, db as a column sum."""

    @staticmethod
    def forward(ctx, x, w, b, act):
        x = x if x.stride(-1) == 1 else x.contiguous()
        y = ops.linear(x, w, b, act=act)
        ctx.act = act
        ctx.has_bias = b is not None
        ctx.save_for_backward(x, w, y if act is not None else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dy = dy.contiguous()
        if ctx.act == 'relu':
            dy = ops.relu_bwd_(dy.clone(), y)
        elif ctx.act == 'tanh':
            dy = dy * (1.0 - y * y)
        elif ctx.act == 'sigmoid':
            dy = dy * y * (1.0 - y)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = ops.linear(dy, w.t().contiguous(), None)
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            dw = ops.linear_wgrad(dy, x, want_bias=want_b)
            if want_b:
                dw, db = dw
        elif want_b:
            db = ops.colsum(dy)
        return dx, dw, db, None


def linear(x, lin, act=None):
    """nn.Linear ``lin`` applied to the last axis of x (any leading shape)."""
    shape = x.shape[:-1]
    y = _Linear.apply(x.reshape(-1, x.shape[-1]), lin.weight, lin.bias, act)
    return y.view(*shape, -1)


class _GatherRows(torch.autograd.Function):
    """table[idx] (nn.Embedding forward) on the gather kernel; backward = the scatter-add kernel."""

    @staticmethod
    def forward(ctx, idx, table, hot_id):
        out = torch.empty((idx.numel(), table.shape[1]), dtype=torch.float32, device=table.device)
        ops.gather_rows(idx, table, out)
        ctx.save_for_backward(idx)
        ctx.shape = tuple(table.shape)
        ctx.hot_id = hot_id
        return out

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        dtable = torch.zeros(ctx.shape, dtype=torch.float32, device=dy.device)
        ops.embed_bwd(idx, dy.contiguous(), dtable, hot_id=ctx.hot_id)
        return None, dtable, None


def embedding(table, idx, hot_id=-1):
    """table[idx] for an integer tensor idx of any shape -> [*idx.shape, dim].  ``hot_id``: a row that a large share of the
    indices hit (the padding word), summed per wave before it reaches memory in the backward."""
    flat = idx.reshape(-1)
    flat = (flat if flat.dtype == torch.int32 else flat.to(torch.int32)).contiguous()
    if table.requires_grad and torch.is_grad_enabled():
        out = _GatherRows.apply(flat, table, hot_id)
    else:
        out = torch.empty((flat.numel(), table.shape[1]), dtype=torch.float32, device=table.device)
        ops.gather_rows(flat, table, out)
    return out.view(*idx.shape, table.shape[1])


class _IntentFuse(torch.autograd.Function):
    """[title_i | sim * body_i] [M, 2D] from the k intents of title and body (newsEncoders.py:355-371) on the fused kernel."""

    @staticmethod
    def forward(ctx, intents, hidden, a2_t, a2_b, M, k):
        D, A = intents.shape[1], hidden.shape[1]
        intents, hidden = intents.contiguous(), hidden.contiguous()
        a2_t, a2_b = a2_t.reshape(-1).contiguous(), a2_b.reshape(-1).contiguous()
        out = torch.empty((M, 2 * D), dtype=torch.float32, device=intents.device)
        ops.intent_fuse(intents, hidden, a2_t, a2_b, out, M, k, D, A)
        ctx.dims = (M, k, D, A)
        ctx.save_for_backward(intents, hidden, a2_t, a2_b)
        return out

    @staticmethod
    def backward(ctx, dout):
        intents, hidden, a2_t, a2_b = ctx.saved_tensors
        M, k, D, A = ctx.dims
        d_int, d_hid, da_t, da_b = ops.intent_fuse_bwd(intents, hidden, a2_t, a2_b, dout.contiguous(), M, k, D, A)
        return d_int, d_hid, da_t, da_b, None, None


class _LinearXent(torch.autograd.Function):
    """scale * sum_rows cross_entropy(x w^T + b, target) on lime_linear_xent_f32 (newsEncoders.py:375-393 behind :358-364).  The forward
    launch already writes dlogits and dx; backward scales them by the incoming dloss, dW = dlogits^T x on the weight-gradient GEMM and
    db as a column sum."""

    @staticmethod
    def forward(ctx, x, w, b, target, scale):
        loss, _, dlogits, dx = ops.linear_xent(x, w.contiguous(), b, target, scale)
        ctx.has_bias = b is not None
        ctx.save_for_backward(x, dlogits, dx)
        return loss.squeeze_(0)           # 0-dim without being a view, as _NllSoftmax's

    @staticmethod
    def backward(ctx, dloss):
        x, dlogits, dx = ctx.saved_tensors
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = dx * dloss
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_b:
            d = dlogits * dloss
            if ctx.needs_input_grad[1]:
                gw = ops.linear_wgrad(d, x, want_bias=want_b)
                if want_b:
                    gw, gb = gw
            else:
                gb = ops.colsum(d)
        return gx, gw, gb, None, None


def category_loss(enc, title_intent, category, alpha):
    """The auxiliary loss of the CROWN content encoder ``enc`` for one encoder call (newsEncoders.py:358-364): alpha x the mean over the
    rows of cross_entropy(category_predictor.fc(title_intent), one_hot(category)) -> a 0-dim tensor with autograd.  ``title_intent``
    [M, intent_embedding_dim] may be a column slice; ``category`` int32 [M]."""
    fc = enc.category_predictor.fc
    return _LinearXent.apply(title_intent, fc.weight, fc.bias, category, float(alpha) / title_intent.shape[0])


class _GateLN(torch.autograd.Function):
    """LayerNorm(g s x + (1 - g) x), g = sigmoid(s y + bias) (layers.py:84-89); y = W_g x comes from the caller's GEMM."""

    @staticmethod
    def forward(ctx, y, x, scale, bias, gamma, beta, eps):
        y, x, scale = y.contiguous(), x.contiguous(), scale.contiguous()
        out = ops.gate_ln(y, x, scale, bias, gamma, beta, eps)
        ctx.eps = eps
        ctx.save_for_backward(y, x, scale, bias, gamma, beta)
        return out

    @staticmethod
    def backward(ctx, dout):
        y, x, scale, bias, gamma, beta = ctx.saved_tensors
        dy, dx, dscale, dbias, dgamma, dbeta = ops.gate_ln_bwd(y, x, scale, bias, gamma, beta, ctx.eps, dout)
        return dy.view_as(y), dx.view_as(x), dscale.view_as(scale), dbias, dgamma, dbeta, None


class _CandAttnWeights(torch.autograd.Function):
    """agg [B, H] of CandidateAware_ClickedNewsAttention (layers.py:66-81) from the topic projections, with the layer's own
    dropout (p = 0.2, layers.py:36,74) on the per-head probabilities in training mode."""

    @staticmethod
    def forward(ctx, qp, kp, mask, dims, n_head, p, seed):
        B, N, H, D = dims
        qp, kp, mask = qp.contiguous(), kp.contiguous(), mask.contiguous()
        agg = ops.cand_attn_weights_train(qp.view(-1), kp.view(-1), mask, B, N, H, D, n_head, p, seed, 0)
        ctx.cfg = (dims, n_head, p, seed)
        ctx.save_for_backward(qp, kp, mask)
        return agg

    @staticmethod
    def backward(ctx, dagg):
        qp, kp, mask = ctx.saved_tensors
        (B, N, H, D), n_head, p, seed = ctx.cfg
        dqp, dkp = ops.cand_attn_weights_bwd(qp.view(-1), kp.view(-1), mask, dagg, B, N, H, D, n_head, p, seed, 0)
        return dqp.view_as(qp), dkp.view_as(kp), None, None, None, None, None


class _Dropout(torch.autograd.Function):
    """nn.Dropout on the counter-based masks (csrc/dropout.h): the backward re-applies the mask of (seed, site)."""

    @staticmethod
    def forward(ctx, x, p, seed, site):
        ctx.cfg = (p, seed, site)
        return ops.dropout(x.contiguous(), p, seed, site)

    @staticmethod
    def backward(ctx, dy):
        p, seed, site = ctx.cfg
        return ops.dropout(dy.contiguous(), p, seed, site), None, None, None


class _MaskedAttention(torch.autograd.Function):
    """The attention core of layers.MultiHeadAttention (layers.py:227-237): softmax(Q K^T / sqrt(d_k), key mask -1e9) V on the
    packed [tokens, 3 h d_k] projections.

    ``center_keys`` (the MHSA user encoder): the exact dK of a sequence sums to zero over its live keys in every column -- each
    query's dS row sums to zero, and masked keys get none -- while the kernel's rows keep a common residue (delta times the rounding
    of 1 / sum in its probabilities, some 4e-7 of the largest entry).  The residue is all that the K bias gradient, the column sum
    of dK, consists of.  Subtracting the live keys' column mean per sequence is the projection onto what the exact gradient
    satisfies: it takes error out and no signal."""

    @staticmethod
    def forward(ctx, qkv, mask, n_seq, S, h, dk, center_keys=False):
        W = h * dk
        out = ops.token_attention(qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:], n_seq, S, h, dk, 1.0 / math.sqrt(float(dk)), key_mask=mask)
        ctx.dims = (n_seq, S, h, dk, center_keys)
        ctx.save_for_backward(qkv, mask)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, mask = ctx.saved_tensors
        n_seq, S, h, dk, center_keys = ctx.dims
        W = h * dk
        dqkv = ops.token_attention_bwd(qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:], dout.contiguous(), n_seq, S, h, dk,
                                       1.0 / math.sqrt(float(dk)), key_mask=mask)
        if center_keys:
            live = mask.reshape(n_seq, S, 1).to(dqkv.dtype)
            d_k = dqkv[:, W:2 * W].view(n_seq, S, W)                       # a view: the subtraction lands in dqkv
            mean = (d_k * live).sum(dim=1, keepdim=True) / live.sum(dim=1, keepdim=True).clamp(min=1.0)
            d_k.sub_(mean * live)
        return dqkv, None, None, None, None, None, None


class _AdditivePool(torch.autograd.Function):
    """layers.Attention over the tokens of a sequence (layers.py:285-300 as newsEncoders.py:591-592 calls it): rep [M, D] =
    sum_t softmax_t(mask(hidden_t . a2)) x_t, one kernel each way (lime_additive_pool_f32 / _bwd_f32)."""

    @staticmethod
    def forward(ctx, hidden, a2, x, mask, n_seq, S):
        hidden, x, a2 = hidden.contiguous(), x.contiguous(), a2.contiguous()
        ctx.dims = (n_seq, S)
        ctx.save_for_backward(hidden, a2, x, mask)
        return ops.additive_pool(hidden, a2, x, n_seq, S, mask=mask)

    @staticmethod
    def backward(ctx, dout):
        hidden, a2, x, mask = ctx.saved_tensors
        n_seq, S = ctx.dims
        dh, da2, dx = ops.additive_pool_bwd(hidden, a2, x, dout.contiguous(), n_seq, S, mask=mask)
        return dh, da2, dx, None, None, None


class _InterestMatch(torch.autograd.Function):
    """logits [B, N] = (softmax_h(kp . qp / sqrt(A)) g) . cand * lifetime weight (userEncoders.py:158-169, util.py:23-49)."""

    @staticmethod
    def forward(ctx, kp, qp, g, cand, remaining, dims, scale, alpha, beta, use_weight, use_penalty):
        B, N, H, A, D = dims
        kp, qp, g, cand = kp.contiguous(), qp.contiguous(), g.contiguous(), cand.contiguous()
        remaining = remaining.contiguous()
        _, logits = ops.interest_match(kp.view(-1), qp.view(-1), g.view(-1), cand.view(-1), remaining, B, N, H, A, D, scale, alpha, beta,
                                       use_weight, use_penalty, want_logits=True, want_user=False)
        ctx.cfg = (dims, scale, alpha, beta, use_weight, use_penalty)
        ctx.save_for_backward(kp, qp, g, cand, remaining)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        kp, qp, g, cand, remaining = ctx.saved_tensors
        (B, N, H, A, D), scale, alpha, beta, use_weight, use_penalty = ctx.cfg
        dkp, dqp, dg, dcand = ops.interest_match_bwd(kp.view(-1), qp.view(-1), g.view(-1), cand.view(-1), remaining, dlogits, B, N, H, A, D,
                                                     scale, alpha, beta, use_weight, use_penalty)
        return dkp.view_as(kp), dqp.view_as(qp), dg.view_as(g), dcand.view_as(cand), None, None, None, None, None, None, None


def _unpad_heads(t, groups, hd, hs):
    """[groups * hs, ...] -> [groups * hd, ...]: drop the padding rows ``ops.pad_heads`` inserted."""
    if hs == hd:
        return t
    rest = t.shape[1:]
    return t.view(groups, hs, *rest)[:, :hd].reshape(groups * hd, *rest)


# dropout sites of one encoder call (csrc/dropout.h): the mask of a site is a function of (seed, site, element index)
_SITE_EMB, _SITE_PE, _SITE_ATTN, _SITE_DROP1, _SITE_FF, _SITE_DROP2 = range(6)


def _layer_forward(ctx, x, gather, M, S, nhead, eps1, eps2, p, seed, in_w, in_b, out_w, out_b, l1_w, l1_b, l2_w, l2_b, n1_w, n1_b, n2_w,
                   n2_b, live=None):
    """y [M S, E] = one post-LN TransformerEncoderLayer (newsEncoders.py:244-247): in_proj, attention, out_proj + residual + LayerNorm,
    linear1 + ReLU, linear2 + residual + LayerNorm on the kernels of the scoring path with the LayerNorm rstd kept, or -- p > 0,
    training-mode dropout seeded per call -- with the layer's four dropouts on the dropout kernels (masks are regenerated in the
    backward from (seed, site)).  Leaves on ``ctx`` what ``_layer_backward`` reads.

    The input is ``x`` [M S, E], materialised, or (x None) ``gather`` = (flat ids, table, pe): E[ids] + PE.  With p = 0 that one is
    gathered inside the in_proj GEMM and rebuilt in out_proj's epilogue; with p > 0 it is materialised through its two dropouts (word
    embeddings and positional sum, :311-312, :827).
    live (optional, gathered input, p = 0): (ids, rows) of the non-padding tokens (int32 device tensors, lime_compact_sequences' tok_ids /
    tok_rows cut to their count): in_proj then runs over those only and the padding tokens' q / k / v rows -- a function of the position
    alone -- are copied in from S rows (the reference's batch is 72 % padding tokens: newsEncoders.py:311-312 embeds them all the same)."""
    E = in_w.shape[1]
    hd = E // nhead
    hs = 32 if hd <= 32 else hd
    if hd > 128 or (hd > 32 and hd % 4) or S > 512:
        raise NotImplementedError('the attention kernels cover head_dim <= 32, or 32 < head_dim <= 128 with head_dim %% 4 == 0, '
                                  'and S <= 512 (got %d, %d)' % (hd, S))
    W = nhead * hs
    tok = M * S
    dev = in_w.device
    scale = 1.0 / math.sqrt(hd)
    w_in = ops.pad_heads(in_w, 3 * nhead, hd, hs) if hs != hd else in_w
    b_in = ops.pad_heads(in_b, 3 * nhead, hd, hs) if hs != hd else in_b
    if x is None and p > 0:
        x = ops.embed_pe_dropout(*gather, S, p, seed, _SITE_EMB, _SITE_PE)
    if x is not None:
        qkv = ops.linear(x, w_in, b_in, n_alg=3 * E)
        res = dict(res=x)
    else:
        flat, table, pe = gather
        pew = ops.linear(pe[:S], w_in, b_in)
        if live is not None and live[0].numel() >= 4096:
            tok_ids, tok_rows = live
            qkv = torch.empty((tok, 3 * W), dtype=torch.float32, device=dev)
            ops.linear(table, w_in, None, a_ids=tok_ids, res=pew, res_mod=S, n_alg=3 * E, c_ids=tok_rows, out=qkv)
            pad_rows = ops.linear(table, w_in, None, a_ids=torch.zeros(S, dtype=torch.int32, device=dev), res=pew, res_mod=S)
            ops.fill_pad_rows(flat, pad_rows, qkv, S)
        else:
            qkv = ops.linear(table, w_in, None, a_ids=flat, res=pew, res_mod=S, n_alg=3 * E)
        res = dict(res=table, res_ids=flat, res_pe=pe, res_period=S)
    lse = None
    if p > 0:
        ao = ops.token_attention_dropout(qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:], M, S, nhead, hd, scale, p, seed, _SITE_ATTN,
                                         head_stride=hs)
        x1, rstd1 = ops.dropout_add_layernorm(ops.linear(ao, out_w, out_b), x, n1_w, n1_b, eps1, p, seed, _SITE_DROP1)
        h = ops.linear(x1, l1_w, l1_b, act='relu', dropout=(p, seed, _SITE_FF))     # the dropout behind the ReLU in the GEMM's epilogue
        y, rstd2 = ops.dropout_add_layernorm(ops.linear(h, l2_w, l2_b), x1, n2_w, n2_b, eps2, p, seed, _SITE_DROP2)
    else:
        # S > 128: the forward keeps its softmax statistics, the blocked backward does not recompute them
        lse = torch.empty(tok * nhead, dtype=torch.float32, device=dev) if S > 128 else None
        ao = ops.token_attention(qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:], M, S, nhead, hd, scale, head_stride=hs, lse=lse)
        rstd1 = torch.empty(tok, dtype=torch.float32, device=dev)
        x1 = ops.linear(ao, out_w, out_b, ln=(n1_w, n1_b), ln_eps=eps1, ln_rstd=rstd1, **res)
        h = ops.linear(x1, l1_w, l1_b, act='relu')
        rstd2 = torch.empty(tok, dtype=torch.float32, device=dev)
        y = ops.linear(h, l2_w, l2_b, res=x1, ln=(n2_w, n2_b), ln_eps=eps2, ln_rstd=rstd2)
    ctx.dims = (M, S, E, nhead, hd, hs, p, seed)
    ctx.lse = lse
    ctx.save_for_backward(w_in, out_w, l1_w, l2_w, n1_w, n1_b, n2_w, n2_b, qkv, ao, x1, rstd1, h, y, rstd2, x, *(gather or ()))
    return y


def _layer_backward(ctx, dy, pooled=False):
    """Backward of ``_layer_forward``: LayerNorm / attention / ReLU backward kernels, the MFMA weight-gradient GEMM, input gradients on
    lime_linear_f32 with transposed weights.  dy: the gradient of y [M S, E], or -- ``pooled`` -- of its token means [M, E].
    -> (the gradient of the layer input [M S, E], the gradients of the twelve weights in ``_layer_forward``'s order)."""
    (w_in, out_w, l1_w, l2_w, n1_w, n1_b, n2_w, n2_b, qkv, ao, x1, rstd1, h, y, rstd2, x, *gather) = ctx.saved_tensors
    M, S, E, nhead, hd, hs, p, seed = ctx.dims
    W = nhead * hs
    drop = p > 0
    keep_scale = 1.0 / (1.0 - p) if drop else 1.0
    # norm2 <- mean pool: every token of a sequence receives dpooled / S
    dy_kw = dict(dy_div=S, dy_scale=1.0 / S) if pooled else {}
    if drop:                                                                   # dt2: the branch through dropout2 into linear2, same pass
        dz2, dn2_w, dn2_b, dl2_b, dt2 = ops.layernorm_bwd(dy.contiguous(), y, n2_w, n2_b, rstd2, dropout=(p, seed, _SITE_DROP2), **dy_kw)
    else:                                                                      # dl2_b: column sums of dt2
        dz2, dn2_w, dn2_b, dl2_b = ops.layernorm_bwd(dy.contiguous(), y, n2_w, n2_b, rstd2, **dy_kw)
        dt2 = dz2
    del y
    dl2_w = ops.linear_wgrad(dt2, h)
    # dH = dT2 W2 with the ReLU (and dropout) gradient in the GEMM's epilogue: h > 0 <=> ReLU passed and the mask kept
    dh = ops.linear(dt2, l2_w.t().contiguous(), None, act='relu_grad', res=h, act_scale=keep_scale)
    del h, dt2
    dl1_w, dl1_b = ops.linear_wgrad(dh, x1, want_bias=True)
    dx1 = ops.linear(dh, l1_w.t().contiguous(), None, res=dz2)                 # through linear1 + the residual branch
    del dh, dz2
    if drop:
        dz1, dn1_w, dn1_b, dout_b, dt1 = ops.layernorm_bwd(dx1, x1, n1_w, n1_b, rstd1, dropout=(p, seed, _SITE_DROP1))
    else:
        dz1, dn1_w, dn1_b, dout_b = ops.layernorm_bwd(dx1, x1, n1_w, n1_b, rstd1)
        dt1 = dz1
    del dx1, x1
    dout_w = ops.linear_wgrad(dt1, ao)
    dao = ops.linear(dt1, out_w.t().contiguous(), None)
    dqkv = ops.token_attention_bwd(qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:], dao, M, S, nhead, hd, 1.0 / math.sqrt(hd),
                                   head_stride=hs, out=ao, dropout=(p, seed, _SITE_ATTN) if drop else None, lse=ctx.lse)
    del dao, qkv, ao, dt1
    if x is None:
        x = ops.embed_pe(*gather, S)                                           # the layer input, re-gathered
    din_w, din_b = ops.linear_wgrad(dqkv, x, want_bias=True)
    din_w, din_b = _unpad_heads(din_w, 3 * nhead, hd, hs), _unpad_heads(din_b, 3 * nhead, hd, hs)
    del x
    dx = ops.linear(dqkv, w_in.t().contiguous(), None, res=dz1)                # through in_proj + the residual branch
    return dx, (din_w, din_b, dout_w, dout_b, dl1_w, dl1_b, dl2_w, dl2_b, dn1_w, dn1_b, dn2_w, dn2_b)


class _TokenEncoder(torch.autograd.Function):
    """pooled [M, E] = mean_S(EncoderLayer(E[ids] + PE))  (newsEncoders.py:311-321 for one of title / body): ``_layer_forward`` over
    the gathered input (``*live``: its live-token lists) + the token mean, the word-table scatter-add behind ``_layer_backward``."""

    @staticmethod
    def forward(ctx, ids, nhead, eps1, eps2, p, seed, table, pe, *weights_live):
        M, S = ids.shape
        ctx.n_extra = len(weights_live) - 12
        y = _layer_forward(ctx, None, (ids.reshape(-1).contiguous(), table, pe), M, S, nhead, eps1, eps2, p, seed, *weights_live)
        return ops.mean_pool(y, M, S)

    @staticmethod
    def backward(ctx, dpooled):
        dx0, dweights = _layer_backward(ctx, dpooled, pooled=True)
        flat, table = ctx.saved_tensors[-3:-1]
        p, seed = ctx.dims[-2:]
        dtable = None
        if ctx.needs_input_grad[6]:
            if p > 0:                                                              # back through the two input dropouts, one pass
                ops.dropout2(dx0, p, seed, _SITE_PE, _SITE_EMB, out=dx0)
            dtable = torch.zeros_like(table)
            ops.embed_bwd(flat, dx0, dtable, hot_id=0)
        return (None, None, None, None, None, None, dtable, None) + dweights + (None,) * ctx.n_extra


class _EmbedPE(torch.autograd.Function):
    """x0 [M S, E] = drop(drop(E[ids]) + PE[t]) (newsEncoders.py:311-312, :827): the layer input, materialised -- the entry of the
    num_layers > 1 path (the single-layer node above gathers it inside its in_proj GEMM)."""

    @staticmethod
    def forward(ctx, ids, table, pe, p, seed):
        M, S = ids.shape
        flat = ids.reshape(-1).contiguous()
        ctx.cfg = (S, p, seed)
        ctx.save_for_backward(flat, table)
        if p > 0:
            return ops.embed_pe_dropout(flat, table, pe, S, p, seed, _SITE_EMB, _SITE_PE)
        return ops.embed_pe(flat, table, pe, S)

    @staticmethod
    def backward(ctx, dx0):
        flat, table = ctx.saved_tensors
        S, p, seed = ctx.cfg
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        dx0 = dx0.contiguous()
        if p > 0:                                                                  # back through the two input dropouts
            dx0 = ops.dropout2(dx0, p, seed, _SITE_PE, _SITE_EMB)
        dtable = torch.zeros_like(table)
        ops.embed_bwd(flat, dx0, dtable, hot_id=0)
        return None, dtable, None, None, None


class _EncoderLayer(torch.autograd.Function):
    """y [M S, E] = ``_layer_forward`` over a MATERIALISED input x: what a layer behind the first needs (config.py:70 allows
    num_layers = 2), and the first one on that path too; dx as the input gradient."""

    @staticmethod
    def forward(ctx, x, M, S, nhead, eps1, eps2, p, seed, *weights):
        return _layer_forward(ctx, x.contiguous(), None, M, S, nhead, eps1, eps2, p, seed, *weights)

    @staticmethod
    def backward(ctx, dy):
        dx, dweights = _layer_backward(ctx, dy)
        return (dx, None, None, None, None, None, None, None) + dweights


class _SeqExpand(torch.autograd.Function):
    """pooled[s] = pooled_c[seq_inv[s]]: the compact sequences' pooled vectors back on every slot (all-padding slots share the
    representative's).  Backward: every live compact row has exactly one slot (a gather by seq_src), the representative's
    gradient is the sum over the all-padding slots -- a fixed-order torch reduction, no atomics."""

    @staticmethod
    def forward(ctx, pooled_c, seq_inv, seq_src, n_live):
        out = torch.empty((seq_inv.numel(), pooled_c.shape[1]), dtype=torch.float32, device=pooled_c.device)
        ops.gather_rows(seq_inv, pooled_c.contiguous(), out)
        ctx.save_for_backward(seq_inv, seq_src)
        ctx.n_live = n_live
        return out

    @staticmethod
    def backward(ctx, dout):
        seq_inv, seq_src = ctx.saved_tensors
        n_live = ctx.n_live
        dout = dout.contiguous()
        d = torch.empty((n_live + 1, dout.shape[1]), dtype=torch.float32, device=dout.device)
        if n_live:
            ops.gather_rows(seq_src[:n_live].contiguous(), dout, d[:n_live])
        pad = (seq_inv == n_live).to(dout.dtype).unsqueeze(1)
        d[n_live] = (dout * pad).sum(dim=0)
        return d, None, None, None


# Training with every dropout off (p = 0): an all-padding sequence pools to the same vector in every slot, so the encoder runs on
# the live sequences + one representative, forward and backward (the representative collects the gradients of all its slots).
# With dropout on every slot draws its own masks (the reference's behaviour) and nothing is shared.  LIME_DENSE_TOKENS=1 turns
# it off, as on the scoring path.
def _dedup_sequences(ids):
    from . import newsEncoders
    if not newsEncoders.DEDUP or ids.shape[0] < 64:
        return None
    cmp = ops.compact_sequences(ids)
    n_c, _, n_tok, n_live = (int(v) for v in cmp.counts[:4].tolist())  # one host read per encoder call (the step is eager)
    if n_c >= ids.shape[0]:
        return None                                                    # nothing repeats
    return cmp, n_c, n_live, n_tok


def _draw_seed():
    """A fresh 62-bit seed from torch's CPU generator (torch.manual_seed makes a run repeatable)."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def encode_tokens(ids, table, pos_encoder, transformer, nhead, p_embedding=0.0):
    """``p_embedding``: the probability of the inplace dropout the caller's encoder applies to the word embeddings (0 in eval
    mode).  The HIP layer applies ONE probability to its six dropout sites, which is how the reference builds it
    (config.dropout_rate everywhere); anything else is refused."""
    if transformer.norm is not None:
        raise NotImplementedError('a final encoder norm is not used by the reference (newsEncoders.py:245,247)')
    layers = list(transformer.layers)
    ps = [p_embedding, pos_encoder.dropout.p if pos_encoder.training else 0.0]
    for layer in layers:
        ps += [layer.self_attn.dropout, layer.dropout1.p, layer.dropout.p, layer.dropout2.p] if layer.training else [0.0] * 4
    if max(ps) != min(ps):
        raise NotImplementedError('the HIP encoder layer applies one dropout probability to all of its sites; got %s (embedding, '
                                  'positional, then attention, dropout1, dropout, dropout2 per layer): put the news encoder into one mode' % ps)
    p = float(ps[0])
    ids = ids.contiguous()
    dd = _dedup_sequences(ids) if p == 0 else None
    seed = lambda: _draw_seed() if p > 0 else 0
    weights = lambda l: (l.self_attn.in_proj_weight, l.self_attn.in_proj_bias, l.self_attn.out_proj.weight, l.self_attn.out_proj.bias,
                         l.linear1.weight, l.linear1.bias, l.linear2.weight, l.linear2.bias, l.norm1.weight, l.norm1.bias, l.norm2.weight,
                         l.norm2.bias)
    if len(layers) == 1:
        layer = layers[0]
        run = lambda rows, *live: _TokenEncoder.apply(rows, nhead, layer.norm1.eps, layer.norm2.eps, p, seed(), table, pos_encoder.table(),
                                                      *weights(layer), *live)
    else:
        def run(rows):                                  # num_layers = 2 (config.py:70): materialised input, one node per layer, mean pool
            M, S = rows.shape
            x = _EmbedPE.apply(rows, table, pos_encoder.table(), p, seed())
            for layer in layers:
                x = _EncoderLayer.apply(x, M, S, nhead, layer.norm1.eps, layer.norm2.eps, p, seed(), *weights(layer))
            return x.view(M, S, -1).mean(dim=1)                                                                 # :317 / :321
    if dd is None:
        return run(ids)
    cmp, n_c, n_live, n_tok = dd
    S = ids.shape[1]
    if len(layers) == 1:                                 # the live tokens' (id, compact row) lists: in_proj over them only
        pooled_c = run(cmp.ids_c[:n_c * S].view(n_c, S), (cmp.tok_ids[:n_tok], cmp.tok_rows[:n_tok]))
    else:
        pooled_c = run(cmp.ids_c[:n_c * S].view(n_c, S))
    return _SeqExpand.apply(pooled_c, cmp.seq_inv, cmp.seq_src, n_live)


# ---------------------------------------------------------------------------------------------------------------------
# the differentiable forward
# ---------------------------------------------------------------------------------------------------------------------
def crown_tail(enc, title_p, body_p, category, subCategory):
    """newsEncoders.CROWN.forward after the token encoders (newsEncoders.py:340-373): pooled title / body [M, 300] -> [M, 900]."""
    cat_e = embedding(enc.category_embedding.weight, category)
    sub_e = embedding(enc.subCategory_embedding.weight, subCategory)
    cat_rep = linear(torch.cat([cat_e, sub_e], dim=1), enc.category_affine)                                     # :340-342
    w_int = torch.cat([lin.weight for lin in enc.intent_layers], dim=0)
    b_int = torch.cat([lin.bias for lin in enc.intent_layers], dim=0)
    k, D = enc.intent_num, enc.intent_embedding_dim

    M = title_p.shape[0]
    xin = torch.cat([torch.cat([title_p, cat_rep], dim=1), torch.cat([body_p, cat_rep], dim=1)], dim=0)         # :343-344
    iv = _Linear.apply(xin, w_int, b_int, 'relu').view(2 * M * k, D)                                            # :284-295
    hidden = torch.cat([linear(iv[:M * k], enc.title_intent_attention.affine1, act='tanh'),
                        linear(iv[M * k:], enc.body_intent_attention.affine1, act='tanh')], dim=0)              # layers.py:288
    fused = _IntentFuse.apply(iv, hidden, enc.title_intent_attention.affine2.weight.view(-1),
                              enc.body_intent_attention.affine2.weight.view(-1), M, k)                                                                             # :355-371
    return torch.cat([fused, enc.dropout(cat_e.clone()), enc.dropout(sub_e.clone())], dim=1)                    # :221-225


def pooled_tokens(enc, title_text, content_text):
    """The two token encoders of the CROWN content encoder ``enc`` (newsEncoders.py:311-321) on M flat news -> 2 x [M, 300]."""
    table = enc.word_embedding.weight
    p_emb = enc.dropout.p if enc.training else 0.0                                                              # :311-312
    title_p = encode_tokens(title_text, table, enc.title_pos_encoder, enc.title_transformer, enc.head_num, p_emb)   # :311-317
    body_p = encode_tokens(content_text, table, enc.body_pos_encoder, enc.body_transformer, enc.head_num, p_emb)    # :312-321
    return title_p, body_p


def mhsa_content(enc, title_text, title_mask, category, subCategory):
    """newsEncoders.MHSA.forward (newsEncoders.py:582-595; title only) on M flat news -> [M, h d_k + 100]."""
    M, T = title_text.shape
    if T > 128:
        raise NotImplementedError('the masked attention backward covers sequences of at most 128 tokens (got %d)' % T)
    mha, att = enc.multiheadAttention, enc.attention
    if mha.d_k != mha.d_v:
        raise NotImplementedError('d_k != d_v')
    p = float(enc.dropout.p) if enc.training else 0.0
    seed = _draw_seed() if p > 0 else 0
    x = embedding(enc.word_embedding.weight, title_text, hot_id=0).view(M * T, -1)                              # :588
    if p > 0:
        x = _Dropout.apply(x, p, seed, 0)
    w = torch.cat([mha.W_Q.weight, mha.W_K.weight, mha.W_V.weight], dim=0)
    b = torch.cat([mha.W_Q.bias, mha.W_K.bias, mha.W_V.bias], dim=0)
    mask = title_mask.contiguous()
    c = _MaskedAttention.apply(_Linear.apply(x, w, b, None), mask, M, T, mha.h, mha.d_k)                         # :590, layers.py:222-238
    if p > 0:
        c = _Dropout.apply(c, p, seed, 1)
    hidden = linear(c, att.affine1, act='tanh')                                                                 # layers.py:288
    rep = _AdditivePool.apply(hidden, att.affine2.weight.view(-1), c, mask, M, T)                               # :592, layers.py:289-300
    cat_e = embedding(enc.category_embedding.weight, category)
    sub_e = embedding(enc.subCategory_embedding.weight, subCategory)
    return torch.cat([rep, enc.dropout(cat_e.clone()), enc.dropout(sub_e.clone())], dim=1)                      # :594


class _Conv1D(torch.autograd.Function):
    """layers.Conv1D + ReLU (layers.py:126-130) on M = sequences x T token rows x [M, C]: the convolutions (window, weight [n, C, window],
    bias [n]) write their column slices of one output on the windowed conv GEMM.  Backward: ReLU backward, the data gradient on the
    same kernel with the taps reversed (summed over the convolutions in order), the weight gradient on its windowed sibling kernel, the
    bias gradient as a column sum."""

    @staticmethod
    def forward(ctx, holder, x, T, *params):
        x = x.contiguous()
        ws = params[0::2]                                  # the holder's own weights, as inputs of the graph
        out = holder.relu_into(x, T, torch.empty((x.shape[0], sum(w.shape[0] for w in ws)), dtype=torch.float32, device=x.device))
        ctx.dims = (T, tuple(w.shape[2] for w in ws))
        ctx.save_for_backward(x, out, *ws)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, out, *ws = ctx.saved_tensors
        T, windows = ctx.dims
        M, C = x.shape
        dy = ops.relu_bwd_(dout.contiguous().clone(), out)
        dx = torch.empty((M, C), dtype=torch.float32, device=x.device) if ctx.needs_input_grad[1] else None
        grads = []
        col = 0
        for i, (w, win) in enumerate(zip(ws, windows)):
            n = w.shape[0]
            d = dy[:, col:col + n]
            if dx is not None:
                ops.conv1d_window(d, ops.conv1d_pack_dgrad(w), win, T, out=dx, accumulate=i > 0)
            dw = ops.conv1d_window_wgrad(d, x, win, T).view(n, win, C).permute(0, 2, 1).contiguous()
            grads += [dw, ops.colsum(d)]
            col += n
        return (None, dx, None) + tuple(grads)


def cnn_content(enc, title_text, title_mask, category, subCategory):
    """newsEncoders.CNN.forward (newsEncoders.py:548-563; title only) on M flat news -> [M, cnn_kernel_num + 100].  The dropout sites
    (counter-based masks of one seed): 0 the word embedding (:553), 1 the convolution output (dropout_, :555), 2 / 3 the category /
    subcategory embeddings of feature_fusion (:221-226)."""
    M, T = title_text.shape
    att = enc.attention
    p = float(enc.dropout.p) if enc.training else 0.0
    seed = _draw_seed() if p > 0 else 0
    x = embedding(enc.word_embedding.weight, title_text, hot_id=0).view(M * T, -1)                              # :553
    if p > 0:
        x = _Dropout.apply(x, p, seed, 0)
    c = _conv_c(enc.conv, x, T)                                                                                 # :555, layers.py:126-130
    if p > 0:
        c = _Dropout.apply(c, p, seed, 1)
    mask = title_mask.contiguous()
    hidden = linear(c, att.affine1, act='tanh')                                                                 # layers.py:288
    rep = _AdditivePool.apply(hidden, att.affine2.weight.view(-1), c, mask, M, T)                               # :557, layers.py:289-300
    cat_e = embedding(enc.category_embedding.weight, category)
    sub_e = embedding(enc.subCategory_embedding.weight, subCategory)
    if p > 0:
        cat_e = _Dropout.apply(cat_e, p, seed, 2)
        sub_e = _Dropout.apply(sub_e, p, seed, 3)
    return torch.cat([rep, cat_e, sub_e], dim=1)                                                                # :561, :221-226


class _ConvPool(torch.autograd.Function):
    """layers.Conv2D_Pool (layers.py:165-190) on M = sequences x T token rows of three dense [M, C] sources: per convolution
    (window w, left padding p, pooled positions P; weight [n, C, w, 3], bias [n]) ONE launch of the fused conv + ReLU + max-pool kernel
    into its column slice of the output, the position of every maximum kept.  Backward: the pooling's backward writes the
    pre-activation gradient (dpooled at the kept position, zeros elsewhere); from there the weight gradient per source on the windowed
    weight-gradient kernel, the bias gradient as a column sum and the data gradients on the windowed conv with the taps reversed
    (summed over the convolutions in order) -- an even window as the next odd one behind a zero first tap."""

    @staticmethod
    def forward(ctx, x0, x1, x2, T, specs, *params):
        xs = [x.contiguous() for x in (x0, x1, x2)]
        M = xs[0].shape[0]
        n_seq = M // T
        ws, bs = params[0::2], params[1::2]
        K = sum(w.shape[0] for w in ws)
        out = torch.empty((n_seq, K), dtype=torch.float32, device=x0.device)
        arg = torch.empty((n_seq, K), dtype=torch.int32, device=x0.device)
        col = 0
        for w, b, (win, pad, P) in zip(ws, bs, specs):
            n = w.shape[0]
            ops.conv_pool([(x, None) for x in xs], ops.conv_pool_pack(w), win, pad, P, T, bias=b, out=out[:, col:col + n],
                          arg=arg[:, col:col + n], fused=T <= ops.CONV_POOL_T_MAX)
            col += n
        ctx.dims = (T, specs)
        ctx.save_for_backward(arg, *xs, *ws)
        return out

    @staticmethod
    def backward(ctx, dout):
        arg, x0, x1, x2, *ws = ctx.saved_tensors
        xs = (x0, x1, x2)
        T, specs = ctx.dims
        M, C = x0.shape
        dout = dout.contiguous()
        dxs = [torch.empty((M, C), dtype=torch.float32, device=x0.device) if ctx.needs_input_grad[s] else None for s in range(3)]
        grads = []
        col = 0
        for i, (w, (win, pad, P)) in enumerate(zip(ws, specs)):
            n = w.shape[0]
            wodd, shift = ops.conv_pool_odd_window(win, pad)
            dpre = ops.relu_maxpool_bwd(dout[:, col:col + n], arg[:, col:col + n], T)                    # [M, n]
            dws = []
            for s in range(3):
                if dxs[s] is not None:
                    w_s = nn.functional.pad(w[:, :, :, s], (shift, 0))                                   # [n, C, wodd]: zero first taps
                    ops.conv1d_window(dpre, ops.conv1d_pack_dgrad(w_s), wodd, T, out=dxs[s], accumulate=i > 0)
                dw = ops.conv1d_window_wgrad(dpre, xs[s], wodd, T).view(n, wodd, C)[:, shift:]           # [n, win, C]
                dws.append(dw.permute(0, 2, 1))
            grads += [torch.stack(dws, dim=3).contiguous(), ops.colsum(dpre)]
            col += n
        return tuple(dxs) + (None, None) + tuple(grads)


def kcnn_content(enc, title_text, title_entity, category, subCategory):
    """newsEncoders.KCNN.forward (newsEncoders.py:625-638; title only, no mask) on M flat news -> [M, cnn_kernel_num + 100].  The only
    dropout sites are the two of feature_fusion (:221-226): 0 the category embedding, 1 the subcategory embedding."""
    if title_entity is None:
        raise TypeError('the KCNN content encoder reads the title entity ids (title_entity): the ids are never guessed')
    M, T = title_text.shape
    p = float(enc.dropout.p) if enc.training else 0.0
    seed = _draw_seed() if p > 0 else 0
    x0 = embedding(enc.word_embedding.weight, title_text, hot_id=0).view(M * T, -1)                             # :630
    e = embedding(enc.entity_embedding.weight, title_entity, hot_id=0).view(M * T, -1)                          # :631
    c = embedding(enc.context_embedding.weight, title_entity, hot_id=0).view(M * T, -1)                         # :632
    x1 = linear(e, enc.M_entity, act='tanh')                                                                    # :633
    x2 = linear(c, enc.M_context, act='tanh')
    convs = enc.knowledge_cnn.convs(T)
    params = []
    for conv, _, _, _, _ in convs:
        params += [conv.weight, conv.bias]
    rep = _ConvPool.apply(x0, x1, x2, T, tuple((w, pad, P) for _, _, w, pad, P in convs), *params)              # :635
    cat_e = embedding(enc.category_embedding.weight, category)
    sub_e = embedding(enc.subCategory_embedding.weight, subCategory)
    if p > 0:
        cat_e = _Dropout.apply(cat_e, p, seed, 0)
        sub_e = _Dropout.apply(sub_e, p, seed, 1)
    return torch.cat([rep, cat_e, sub_e], dim=1)                                                                # :637, :221-226


def _conv_c(conv, x, T):
    """layers.Conv1D + ReLU of a parameter holder (layers.Conv1D) over M = sequences x T token rows x [M, C] -> [M, cnn_kernel_num]."""
    params = []
    for c, _ in conv.convs():
        params += [c.weight, c.bias]
    return _Conv1D.apply(conv, x, T, *params)


def naml_content(enc, title_text, content_text, category, subCategory):
    """newsEncoders.NAML.forward (newsEncoders.py:671-695) on M flat news -> [M, cnn_kernel_num].  The word attentions take no mask
    (:686-687).  The dropout sites (counter-based masks of one seed): 0 / 1 the title / body word embeddings (self.dropout, :676-677),
    2 / 3 the title / body convolution outputs (self.dropout_, :681, :684); the category views get none (:689-690).

    Unfused: the attention pools' backward needs the tanh hidden state, so each attention is linear(tanh) + _AdditivePool here while
    the scoring path (NAML.encode_flat) runs the one-launch pool -- the two agree to rounding (summation order), not bit for bit."""
    M, T = title_text.shape
    L = content_text.shape[1]
    p = float(enc.dropout.p) if enc.training else 0.0
    seed = _draw_seed() if p > 0 else 0
    xt = embedding(enc.word_embedding.weight, title_text, hot_id=0).view(M * T, -1)                           # :676
    xb = embedding(enc.word_embedding.weight, content_text, hot_id=0).view(M * L, -1)                         # :677
    if p > 0:
        xt = _Dropout.apply(xt, p, seed, 0)
        xb = _Dropout.apply(xb, p, seed, 1)
    ct = _conv_c(enc.title_conv, xt, T)                                                                         # :681
    cb = _conv_c(enc.content_conv, xb, L)                                                                       # :684
    if p > 0:
        ct = _Dropout.apply(ct, p, seed, 2)
        cb = _Dropout.apply(cb, p, seed, 3)
    views = []
    for c, att, S in ((ct, enc.title_attention, T), (cb, enc.content_attention, L)):                           # :686-687, no mask
        hidden = linear(c, att.affine1, act='tanh')                                                             # layers.py:288
        views.append(_AdditivePool.apply(hidden, att.affine2.weight.view(-1), c, None, M, S))                   # layers.py:289-300
    views.append(linear(embedding(enc.category_embedding.weight, category), enc.category_affine, act='relu'))          # :689
    views.append(linear(embedding(enc.subCategory_embedding.weight, subCategory), enc.subCategory_affine, act='relu'))  # :690
    feature = torch.stack(views, dim=1).view(M * 4, -1)                                                         # :692
    hidden = linear(feature, enc.affine1, act='tanh')                                                           # :693
    return _AdditivePool.apply(hidden, enc.affine2.weight.view(-1), feature, None, M, 4)                        # :693-694


class _LSTMCore(torch.autograd.Function):
    """The recurrence of a bidirectional LSTM (nn.LSTM under pack_padded_sequence, newsEncoders.py:503-515) from the input projections
    gi [n S, 2 . 4h] of every token: -> (hout [n S, 2h], zeros behind each length; c_n [2, n, h]).  Forward: the step kernel with the gate
    activations, c_t and h_{t-1} kept; backward: the gate-gradient step kernel + the carry GEMM per step (ops.lstm_bwd), then dW_hh as one
    weight-gradient GEMM per direction of the pre-activation gradients against the kept h_{t-1} (zero for a direction's first token).
    The gradient of gi goes on to the _Linear node that made it: dW_ih, both biases and the word rows come from there."""

    @staticmethod
    def forward(ctx, gi, whh, lens, S):
        whh = whh.contiguous()
        hout, c, saved = ops.lstm(gi.contiguous(), whh, lens, S, save=True)
        ctx.S = S
        ctx.save_for_backward(whh, lens, *saved)
        return hout, c

    @staticmethod
    def backward(ctx, dhout, dc):
        whh, lens, gates, c_seq, h_prev = ctx.saved_tensors
        h = whh.shape[2]
        dgi = ops.lstm_bwd(dhout.contiguous(), dc, whh, lens, ctx.S, (gates, c_seq, h_prev))
        dwhh = torch.stack([ops.linear_wgrad(dgi[:, d * 4 * h:(d + 1) * 4 * h], h_prev[:, d * h:(d + 1) * h]) for d in (0, 1)], dim=0)
        return dgi, dwhh, None, None


def cne_content(enc, title_text, title_mask, content_text, content_mask, category, subCategory, pair_groups=None):
    """newsEncoders.CNE.forward (newsEncoders.py:486-532) on M flat news -> [M, 4 hidden_dim + 100].  One autograd node per LSTM
    (_LSTMCore, HIP both ways) behind the _Linear node of its input projection; the gates and the cross attention's score terms are torch
    element-wise glue, the GEMMs and the four attention pools the existing nodes.  The dropout sites (counter-based masks of one seed):
    0 / 1 the title / body word embeddings (self.dropout, :501-502), 2 / 3 the category / subcategory embeddings of feature_fusion
    (:221-226).  The mask-slot-0 rule (:492-493) is applied to copies of the masks.  pair_groups: the news counts of the reference calls
    (CNE.reference_pairs: the gates read the reference's partner news); None: every news reads its own other text."""
    from .newsEncoders import CNE
    if content_mask is None:
        raise TypeError('the CNE content encoder reads the body mask (content_mask): pass it -- it is never guessed from the ids')
    M, T = title_text.shape
    L = content_text.shape[1]
    h = enc.hidden_dim
    p = float(enc.dropout.p) if enc.training else 0.0
    seed = _draw_seed() if p > 0 else 0
    table = enc.word_embedding.weight
    texts = []
    for site, (ids, mask, lstm, S) in enumerate(((title_text, title_mask, enc.title_lstm, T), (content_text, content_mask, enc.content_lstm, L))):
        mask = mask.reshape(M, S).bool().clone()
        mask[:, 0] = True                                                                                       # :492-493, on a copy
        x = embedding(table, ids, hot_id=0).view(M * S, -1)                                                     # :501-502
        if p > 0:
            x = _Dropout.apply(x, p, seed, site)
        lens = ops.mask_lengths(mask, min_len=1)                                                                # :494-495
        wih, bias, whh = CNE.lstm_weights(lstm)
        hout, c = _LSTMCore.apply(_Linear.apply(x, wih, bias, None), whh, lens, S)                              # :509-515
        texts.append((S, mask, hout, c.transpose(0, 1).reshape(M, 2 * h), lens))                                # :512-513
    pairs = None
    if pair_groups is not None:
        if sum(pair_groups) != M:
            raise ValueError('pair_groups %s do not add up to the %d news' % (list(pair_groups), M))
        pairs = [p.long() for p in CNE.reference_pairs(texts[0][4], texts[1][4], pair_groups, M)]
    gated = []
    for k, (H_, M_, att) in enumerate(((enc.title_H, enc.title_M, enc.title_self_attention),
                                       (enc.content_H, enc.content_M, enc.content_self_attention))):
        S, mask, hout = texts[k][:3]
        m_other = texts[1 - k][3] if pairs is None else texts[1 - k][3][pairs[k]]                               # :517-518 in sorted order
        tm = _Linear.apply(m_other, M_.weight, M_.bias, None)                                                   # the OTHER text's memory vector
        pre = _Linear.apply(hout, H_.weight, None, None).view(M, S, 2 * h) + tm.unsqueeze(1)
        g = (hout.view(M, S, 2 * h) * torch.sigmoid(pre)).reshape(M * S, 2 * h)                                 # :517-521
        hidden = linear(g, att.affine1, act='tanh')
        gated.append((g, _AdditivePool.apply(hidden, att.affine2.weight.view(-1), g, mask, M, S)))              # :524-525
    ones = torch.ones(2 * h, dtype=torch.float32, device=table.device)
    reps = []
    for k, att in enumerate((enc.title_cross_attention, enc.content_cross_attention)):
        S, mask = texts[k][:2]
        g, own = gated[k]
        q = _Linear.apply(gated[1 - k][1], att.Q.weight, att.Q.bias, None)                                      # the OTHER text's self attention
        v = _Linear.apply(q, att.K.weight.t().contiguous(), None, None)                                         # K(h_t) . q = h_t . (K^T q)
        terms = (g.view(M, S, 2 * h) * (v * (1.0 / att.attention_scalar)).unsqueeze(1)).reshape(M * S, 2 * h)
        reps.append(own + _AdditivePool.apply(terms, ones, g, mask, M, S))                                      # :527-529
    cat_e = embedding(enc.category_embedding.weight, category)
    sub_e = embedding(enc.subCategory_embedding.weight, subCategory)
    if p > 0:
        cat_e = _Dropout.apply(cat_e, p, seed, 2)
        sub_e = _Dropout.apply(sub_e, p, seed, 3)
    return torch.cat(reps + [cat_e, sub_e], dim=1)                                                              # :529-531


def lime_tail(ne, content, freshness, lifetime):
    """LIME.forward, fusion 'concat' (newsEncoders.py:140-153), from the content encoder's output -> [M, 400]."""
    fe = ne.freshness_encoder
    fb = fe.buckets(freshness)
    lb = fe.buckets(lifetime)
    fresh = linear(torch.cat([embedding(fe.freshness_embedding.weight, fb), embedding(fe.lifetime_embedding.weight, lb)], dim=1),
                   fe.dense, act='tanh')
    if ne.fusion_method == 'add':                                                                                   # :154-155
        return content + fresh
    fused = torch.cat([content, fresh], dim=1)
    if ne.fusion_method == 'gated':                                                                                 # :156-159
        gate = linear(fused, ne.gate, act='sigmoid')
        return gate * content + (1 - gate) * fresh
    return fused if isinstance(ne.project, nn.Identity) else linear(fused, ne.project)


def _topic(ne, category, subCategory):
    """userEncoders.py:103-105 / :115-117."""
    x = torch.cat([embedding(ne.category_embedding.weight, category), embedding(ne.subCategory_embedding.weight, subCategory)], dim=-1)
    return linear(x, ne.category_affine)


def candidate_aware(att, hist, hist_topic, cand_topic, mask):
    """CandidateAware_ClickedNewsAttention.forward (layers.py:52-93) -> (refined history [B, H, D], attn_weights_agg [B, H]); the
    value_proj branch is dead there."""
    B, H, D = hist.shape
    N = cand_topic.shape[1]
    if mask is None:
        mask = torch.ones(B, H, dtype=torch.bool, device=hist.device)
    p = float(att.dropout.p) if att.training else 0.0                                                       # layers.py:36,74
    agg = _CandAttnWeights.apply(linear(cand_topic, att.query_proj).reshape(B * N, D), linear(hist_topic, att.key_proj).reshape(B * H, D),
                                 mask, (B, N, H, D), att.num_heads, p, _draw_seed() if p > 0 else 0)           # :66-81
    if not att.use_residual_connection:
        return agg.unsqueeze(-1) * hist, agg
    ln = att.layernorm
    flat = hist.reshape(B * H, D)
    y = _Linear.apply(flat, att.gate_proj.weight, None, None)                       # W_g x; the row scale agg commutes (:87)
    return _GateLN.apply(y, flat, agg.reshape(-1), att.gate_proj.bias, ln.weight, ln.bias, ln.eps).view(B, H, D), agg


def wants_train_path(module, p=0.0):
    """A sub-module called on its own (``news_encoder(...)``, ``user_encoder(...)``, ``candidate_aware_attn(...)``) takes the
    differentiable path of this file when it is in training mode and either autograd is recording or a dropout is active;
    otherwise the fused scoring kernels compute the same function."""
    return module.training and (torch.is_grad_enabled() or p > 0)


def _interest_inputs(ue, hist, cand, category, subCategory, user_category, user_subCategory, user_history_mask, n_src=None):
    """userEncoders.py:103-105, :114-162: candidate-aware refinement, user nodes + GraphSAGE closed form, K / Q projections."""
    B, H, D = hist.shape
    ne = ue.news_encoder
    if ue.use_candidate_aware_attn:
        hist, _ = candidate_aware(ue.candidate_aware_attn, hist, _topic(ne, user_category, user_subCategory),
                                  _topic(ne, category, subCategory), user_history_mask)
    nodes = ue.dropout_(ue.user_node_embedding.unsqueeze(0).expand(B, -1, -1))                                    # :121
    n_src = B if n_src is None else n_src
    if n_src > H + nodes.shape[1]:
        raise IndexError('rows per forward (%d) exceed the node slots H + config.batch_size (SURVEY Q7)' % n_src)
    X = torch.cat([hist, nodes], dim=1)
    conv = ue.graph_sage.convs[0]
    g = linear(X[:, :n_src].mean(dim=1), conv.lin_l).unsqueeze(1) + linear(hist, conv.lin_r)                      # :151-157
    return g, linear(g, ue.K), linear(cand, ue.Q)                                                                 # :161-162


# dropout sites of the pooled user encoders (counter-based masks, csrc/dropout.h): the MHSA user encoder draws one seed per call for
# site 0, the p = 0.5 dropout behind ``affine`` (userEncoders.py:487); the candidate-aware layer draws its own seed for its site 0 (the
# per-head probabilities, layers.py:74), as under CROWN
_SITE_USER_AFFINE = 0


def pooled_user(ue, hist, category, user_category, user_history_mask):
    """userEncoders.ATT / MHSA after the history is encoded (userEncoders.py:546-557, :470-489) -> ONE user vector per row [B, D] with
    autograd: candidate-aware refinement on LIME's frozen category rows alone, (MHSA: masked self-attention, affine + dropout + ReLU,)
    additive attention pooling without a mask."""
    from .userEncoders import MHSA
    B, H, D = hist.shape
    ne = ue.news_encoder
    if ue.use_candidate_aware_attn:
        hist, _ = candidate_aware(ue.candidate_aware_attn, hist, embedding(ne.category_embedding.weight, user_category),
                                  embedding(ne.category_embedding.weight, category), user_history_mask)
    x = hist.reshape(B * H, D)
    if isinstance(ue, MHSA):
        ue.check_history_length(H)
        mha = ue.multiheadAttention
        if mha.d_k != mha.d_v:
            raise NotImplementedError('d_k != d_v')
        if H > 128:
            raise NotImplementedError('the masked attention backward covers sequences of at most 128 rows (got a history of %d)' % H)
        w = torch.cat([mha.W_Q.weight, mha.W_K.weight, mha.W_V.weight], dim=0)
        b = torch.cat([mha.W_Q.bias, mha.W_K.bias, mha.W_V.bias], dim=0)
        c = _MaskedAttention.apply(_Linear.apply(x, w, b, None), user_history_mask.contiguous(), B, H, mha.h, mha.d_k, True)   # :486
        # relu(dropout(z)) of :487 as dropout(relu(z)): the mask scales by 0 or 1 / (1 - p) >= 0, which commutes with the ReLU exactly
        x = _Linear.apply(c, ue.affine.weight, ue.affine.bias, 'relu')
        if ue.training and ue.p_sequence > 0:
            x = _Dropout.apply(x, float(ue.p_sequence), _draw_seed(), _SITE_USER_AFFINE)
    att = ue.attention
    hidden = linear(x, att.affine1, act='tanh')                                                                   # layers.py:288
    return _AdditivePool.apply(hidden, att.affine2.weight.view(-1), x, None, B, H)                                # :489 / :557: no mask


def _is_crown_user(ue):
    from .userEncoders import CROWN
    return isinstance(ue, CROWN)


# the dropout site of the MLP click predictor (model.py:183: Model.dropout behind the ReLU), a number of its own under a seed of its own
_SITE_CLICK_PREDICTOR = 1


def mlp_logits(model, user, cand):
    """The MLP click predictor (model.py:182-184) with autograd: ``out(dropout(relu(mlp(cat[user, news]))))`` for user / cand
    [B, N, D] -> logits [B, N].  ``mlp`` with its ReLU and ``out`` are ``_Linear`` nodes; the dropout is ``Model.dropout`` (p =
    config.dropout_rate, active when that module is in training mode) on the counter-based masks."""
    B, N, D = cand.shape
    x = torch.cat([user.expand(B, N, D), cand], dim=2).reshape(B * N, 2 * D)
    hidden = _Linear.apply(x, model.mlp.weight, model.mlp.bias, 'relu')
    if model.dropout.training and model.dropout.p > 0:
        hidden = _Dropout.apply(hidden, float(model.dropout.p), _draw_seed(), _SITE_CLICK_PREDICTOR)
    return _Linear.apply(hidden, model.out.weight, model.out.bias, None).view(B, N)


def user_logits(ue, weighting, hist, cand, category, subCategory, user_category, user_subCategory, user_history_mask,
                remaining_lifetime, n_src=None, predictor=None):
    """The user encoder's forward after the history is encoded and the lifetime-weighted dot product of model.py:181 / util.py:23-49
    -> logits [B, N].  CROWN: userEncoders.py:103-105, :114-169; ATT / MHSA: ``pooled_user`` + ``lifetime_weighted_logits``.
    ``predictor``: the Model, when its click predictor is not the dot product -- 'mlp' (model.py:182-184): ``user_representation``,
    then ``mlp_logits``; ``remaining_lifetime`` is not read."""
    if predictor is not None and predictor.click_predictor == 'mlp':
        user = user_representation(ue, hist, cand, category, subCategory, user_category, user_subCategory, user_history_mask, n_src)
        return mlp_logits(predictor, user, cand)
    B, H, D = hist.shape
    N = cand.shape[1]
    if not _is_crown_user(ue):
        user = pooled_user(ue, hist, category, user_category, user_history_mask)
        return lifetime_weighted_logits(weighting, user.unsqueeze(1), cand, remaining_lifetime)
    g, kp, qp = _interest_inputs(ue, hist, cand, category, subCategory, user_category, user_subCategory, user_history_mask, n_src)
    A = kp.shape[-1]
    w = weighting
    return _InterestMatch.apply(kp.reshape(B * H, A), qp.reshape(B * N, A), g.reshape(B * H, D), cand.reshape(B * N, D),
                                remaining_lifetime, (B, N, H, A, D), 1.0 / ue.attention_scalar, float(w.alpha), float(w.beta),
                                bool(w.use_remaining_lifetime_weighting), bool(w.use_expired_penalty))               # :163-168


def user_representation(ue, hist, cand, category, subCategory, user_category, user_subCategory, user_history_mask, n_src=None):
    """``user_encoder(...)`` called on its own in training mode (userEncoders.py:101-175) -> user_representation [B, N, D] with
    autograd.  The model's own forward never materialises this tensor (``user_logits`` fuses the attention with the dot product);
    the last two steps (:163-168: softmax over the history, weighted sum) are two batched torch matmuls here.  ATT / MHSA: the pooled
    vector over the news_num axis (:489, :557)."""
    if not _is_crown_user(ue):
        user = pooled_user(ue, hist, category, user_category, user_history_mask)
        return user.unsqueeze(1).expand(-1, cand.shape[1], -1)
    g, kp, qp = _interest_inputs(ue, hist, cand, category, subCategory, user_category, user_subCategory, user_history_mask, n_src)
    a = torch.softmax(torch.bmm(qp, kp.transpose(1, 2)) / ue.attention_scalar, dim=2)                             # [B, N, H]
    return torch.bmm(a, g)


def lifetime_weighted_logits(w, user, news, remaining_lifetime):
    """RemainingLifetimeWeighting.forward (util.py:23-49) as torch ops with autograd (the module called on its own)."""
    base = (user * news).sum(dim=-1)
    if not w.use_remaining_lifetime_weighting:
        return base
    r = remaining_lifetime.float()
    if w.use_expired_penalty:                                                                   # util.py:39-43
        weight = torch.sigmoid(w.alpha * r)
        weight = torch.where(r < 0, w.beta * weight, weight)
    else:
        weight = torch.sigmoid(w.alpha * r.abs())                                               # util.py:46
    return base * weight


def content_flat(enc, title_text, title_mask, content_text, category, subCategory, content_mask=None, pair_groups=None, title_entity=None):
    """The base content encoder (CROWN: newsEncoders.py:302-373, CNN: :548-563, NAML: :671-695, MHSA: :582-595, KCNN: :625-638) on M flat
    news with autograd -> [M, dim]."""
    from .newsEncoders import CNE, CNN, CROWN, KCNN, MHSA, NAML
    if getattr(enc, 'compute_dtype', 'fp32') != 'fp32':
        raise NotImplementedError("compute_dtype %r is a scoring option (BASELINE config 3); the training step is fp32: build the "
                                  "model with compute_dtype='fp32' to train" % enc.compute_dtype)
    if isinstance(enc, CROWN):
        title_p, body_p = pooled_tokens(enc, title_text, content_text)
        return crown_tail(enc, title_p, body_p, category, subCategory)
    if isinstance(enc, MHSA):
        return mhsa_content(enc, title_text, title_mask, category, subCategory)
    if isinstance(enc, CNN):
        return cnn_content(enc, title_text, title_mask, category, subCategory)
    if isinstance(enc, NAML):
        return naml_content(enc, title_text, content_text, category, subCategory)
    if isinstance(enc, CNE):
        return cne_content(enc, title_text, title_mask, content_text, content_mask, category, subCategory, pair_groups)
    if isinstance(enc, KCNN):
        return kcnn_content(enc, title_text, title_entity, category, subCategory)
    raise NotImplementedError('the training path covers the CROWN, CNN, NAML, MHSA, CNE and KCNN content encoders')


def news_flat(ne, title_text, title_mask, content_text, category, subCategory, freshness, lifetime, content_mask=None, pair_groups=None,
              title_entity=None):
    """LIME.forward (newsEncoders.py:140-161) on M flat news with autograd -> [M, 400].  content_mask: the body mask, read by CNE alone;
    title_entity: the title's entity ids, read by KCNN alone.  A content encoder used as the news encoder itself (the baseline form,
    model.py:41-62) is its own representation: freshness and lifetime are not read."""
    if not hasattr(ne, 'base_news_encoder'):
        return content_flat(ne, title_text, title_mask, content_text, category, subCategory, content_mask=content_mask,
                            pair_groups=pair_groups, title_entity=title_entity)
    content = content_flat(ne.base_news_encoder, title_text, title_mask, content_text, category, subCategory, content_mask=content_mask,
                           pair_groups=pair_groups, title_entity=title_entity)
    return lime_tail(ne, content, freshness, lifetime)


def forward_train(model, user_category, user_subCategory, user_title_text, user_title_mask, user_content_text, user_freshness,
                  user_user_topic_lifetime, user_history_mask, news_category, news_subCategory, news_title_text, news_title_mask,
                  news_content_text, news_freshness, news_user_topic_lifetime, remaining_lifetime, user_content_mask=None,
                  news_content_mask=None, user_title_entity=None, news_title_entity=None):
    """Model.forward with [B, N] candidates (model.py:171-187), recording the autograd graph.  Candidates and history go
    through the news encoder as one flat batch of B (N + H) news.  After the token encoders come the content tail, freshness
    and project per news, then the CROWN user encoder and the lifetime-weighted dot product: 3 % of the FLOPs in some 300
    short launches forward + backward (4 ms of kernel time at config 2b -- short kernels, not idle gaps: capturing them into
    HIP graphs with torch.cuda.make_graphed_callables was measured and changed nothing)."""
    ne = model.news_encoder
    B, N = news_category.shape
    H = user_category.shape[1]
    i32 = lambda t: t if t.dtype == torch.int32 else t.to(torch.int32)
    flat2 = lambda c, u: torch.cat([c.reshape(B * N, -1), u.reshape(B * H, -1)], dim=0)
    flat1 = lambda c, u: torch.cat([c.reshape(-1), u.reshape(-1)], dim=0)
    if news_freshness.dim() == 1:
        news_freshness = news_freshness.unsqueeze(1).expand(B, N)
    if news_user_topic_lifetime.dim() == 1:
        news_user_topic_lifetime = news_user_topic_lifetime.unsqueeze(1).expand(B, N)
    category, subCategory = i32(flat1(news_category, user_category)), i32(flat1(news_subCategory, user_subCategory))
    rep = news_flat(ne, i32(flat2(news_title_text, user_title_text)), flat2(news_title_mask, user_title_mask),
                    i32(flat2(news_content_text, user_content_text)), category, subCategory,
                    flat1(news_freshness.float(), user_freshness.float()).contiguous(),
                    flat1(news_user_topic_lifetime.float(), user_user_topic_lifetime.float()).contiguous(),
                    content_mask=None if news_content_mask is None or user_content_mask is None else flat2(news_content_mask, user_content_mask),
                    pair_groups=[B * N, B * H],                # the reference's two encoder calls (model.py:171, userEncoders.py:110)
                    title_entity=None if news_title_entity is None or user_title_entity is None else
                    i32(flat2(news_title_entity, user_title_entity)))
    cand = rep[:B * N].view(B, N, -1)
    hist = rep[B * N:].view(B, H, -1)
    ne.auxiliary_loss = None
    if trains_category_predictor(model):
        # the title intent vector is the first intent_embedding_dim columns of the representation (_IntentFuse's title half, carried
        # through crown_tail's concat untouched); the term is the history call's alone, padded slots (category 0) included
        ne.auxiliary_loss = category_loss(ne, rep[B * N:, :ne.intent_embedding_dim], i32(user_category).reshape(-1).contiguous(), ne.alpha)
    return user_logits(model.user_encoder, model.remaining_lifetime_weighting, hist, cand, i32(news_category).contiguous(),
                       i32(news_subCategory).contiguous(), i32(user_category).contiguous(), i32(user_subCategory).contiguous(),
                       user_history_mask.contiguous(), remaining_lifetime.float().contiguous(),
                       predictor=model if model.click_predictor != 'dot_product' else None)


# ---------------------------------------------------------------------------------------------------------------------
# the native step: flat parameter / gradient / Adam-state buffers, one clip + one Adam launch, one all-reduce
# ---------------------------------------------------------------------------------------------------------------------
def negative_log_softmax(logits):
    """trainer.py:71-73 on the HIP loss kernel (forward and gradient in one launch)."""
    return _NllSoftmax.apply(logits)


class _NllSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits):
        loss, d = ops.nll_softmax(logits.contiguous())
        ctx.save_for_backward(d)
        return loss.squeeze_(0)           # 0-dim without being a view: the trainer's in-place ``loss += ...`` (trainer.py:139) is allowed

    @staticmethod
    def backward(ctx, dloss):
        (d,) = ctx.saved_tensors
        return d * dloss


# parameters the reference constructs and never uses on this path: autograd leaves their .grad at None, Adam and
# clip_grad_norm_ skip them, and so does the flat bucket.  Substrings of the parameter names, for the CROWN user encoder with every
# switch of config.py:60-66 on (``dead_parameters`` is the rule for every model):
_DEAD = ('base_news_encoder.affine.', '.ISAB.', 'category_predictor.', 'user_encoder.affine.', 'candidate_aware_attn.value_proj.')


def trains_category_predictor(model):
    """True when the reference's trainer adds the category-prediction loss for this model (trainer.py:137-139): the news encoder is a
    bare CROWN content encoder (no LIME wrapper: newsEncoders.py:100-103 copies ``auxiliary_loss`` once at construction, while it is
    None, and never again, so under LIME the trainer reads None whatever ``alpha`` is) and ``config.alpha`` is not 0.  At ``alpha == 0``
    the reference's term is an exact zero with exact-zero gradients -- Adam's moments of ``category_predictor.fc`` stay 0 and the
    parameters never move (weight_decay is 0, config.py:47) -- so it is left out altogether: no launch, no attribute, the same bucket
    and the same bits as a model without the option."""
    from .newsEncoders import CROWN
    ne = model.news_encoder
    return isinstance(ne, CROWN) and not hasattr(ne, 'base_news_encoder') and float(ne.alpha) != 0.0


def dead_parameters(model):
    """Names (as ``model.named_parameters()`` first yields them) of the trainable parameters the reference's backward leaves at None
    for this model.  One rule for every user encoder and every setting of the switches:
      * never used: the base encoder's ``affine``, ``candidate_aware_attn.value_proj`` and, where the content encoder has them,
        ``ISAB`` and ``category_predictor`` -- except that a bare CROWN news encoder with ``alpha != 0`` trains
        ``category_predictor.fc`` through its category-prediction loss (``trains_category_predictor``).
      * ``user_encoder.affine``: only the MHSA user encoder applies it (userEncoders.py:487); CROWN constructs it and leaves it alone.
      * ``news_encoder.category_affine`` makes the topic vectors of the CROWN user encoder's candidate-aware attention
        (userEncoders.py:103-105) and nothing else: dead without that layer (``use_candidate_ware_clicked_news_attention`` off), and
        under ATT / MHSA, whose layer reads ``category_embedding`` rows alone (:470,482 / :546,554).
      * ``use_residual_connection`` off: the layer returns agg * x (layers.py:84), its ``gate_proj`` and ``layernorm`` are unused.
    The baseline form (the content encoder is ``news_encoder`` itself, model.py:41-62): the same never-used parameters without the
    ``base_news_encoder.`` level, and ``news_encoder.category_affine`` is the content encoder's own layer, which its representation
    reads whatever the user encoder is (CROWN: newsEncoders.py:340, NAML: :689) -- never dead."""
    from .userEncoders import CROWN, MHSA
    ue = model.user_encoder
    caa = getattr(ue, 'candidate_aware_attn', None)
    plain = not hasattr(model.news_encoder, 'base_news_encoder')
    # prefixes of the names (LIME's ``category_affine``, not the content encoder's own ``base_news_encoder.category_affine``)
    enc = 'news_encoder.' if plain else 'news_encoder.base_news_encoder.'
    dead = [enc + 'affine.', enc + 'ISAB.', 'user_encoder.candidate_aware_attn.value_proj.']
    if not trains_category_predictor(model):
        dead.append(enc + 'category_predictor.')
    if not isinstance(ue, MHSA):
        dead.append('user_encoder.affine.')
    if not plain and not (isinstance(ue, CROWN) and caa is not None):
        dead.append('news_encoder.category_affine.')
    if caa is not None and not caa.use_residual_connection:
        dead += ['user_encoder.candidate_aware_attn.gate_proj.', 'user_encoder.candidate_aware_attn.layernorm.']
    names, seen = [], set()
    for name, p in model.named_parameters():
        if not p.requires_grad or id(p) in seen:
            continue
        seen.add(id(p))
        if name.startswith(tuple(dead)):
            names.append(name)
    return names


class TrainStep:
    """trainer.py:33 + :143-148 for one process (one GPU): Adam(lr, weight_decay) over the parameters that receive
    gradients, ``clip_grad_norm_(gradient_clip_norm)``, and -- under torch.distributed -- ONE all-reduce (RCCL over xGMI on
    ROCm) of the flat gradient bucket before the clip, averaging over ranks as DistributedDataParallel does.

    The loss of ``step`` is the click loss plus, where the model has one, the category-prediction loss the forward left on
    ``model.news_encoder.auxiliary_loss`` (trainer.py:137-139: a bare CROWN news encoder with ``alpha != 0``; None otherwise), and
    ``category_predictor.fc`` is in the bucket exactly then.  Under several ranks each rank's term is the mean over its own rows, and
    the gradient average below equals DistributedDataParallel's.

    Parameters are re-pointed into one flat fp32 buffer (``p.data`` becomes a view, values preserved) and their ``.grad``
    into a second one, so zeroing, the norm, the all-reduce and the Adam update are one launch each.

    One difference from torch's Adam, visible only with ``weight_decay > 0`` (the reference trains with 0, config.py:47): every
    bucket parameter is decayed every step, including one whose gradient happened to be all zero in that step; torch skips a
    parameter whose ``.grad`` is None (the never-used parameters of SURVEY Q20 are outside the bucket and skipped here too).
    """

    def __init__(self, model, lr=1e-4, weight_decay=0.0, gradient_clip_norm=4.0, betas=(0.9, 0.999), eps=1e-8,
                 process_group=None):
        self.model = model
        self.lr, self.weight_decay, self.clip, self.betas, self.eps = lr, weight_decay, gradient_clip_norm, betas, eps
        self.group = process_group
        params = dict(model.named_parameters())
        named = [(n, params[n]) for n in self.bucket_names(model)]
        self.names = [n for n, _ in named]
        self._params = named
        # every parameter starts on a 256-byte boundary of the bucket (the LDS-DMA GEMM wants 16-byte aligned operands);
        # the padding stays zero in all four buffers
        align = lambda n: (n + 63) // 64 * 64
        total = sum(align(p.numel()) for _, p in named)
        dev = named[0][1].device
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        off = 0
        with torch.no_grad():
            for _, p in named:
                n = p.numel()
                self.flat[off:off + n].copy_(p.detach().reshape(-1))
                p.data = self.flat[off:off + n].view(p.shape)
                p.grad = self.grad[off:off + n].view(p.shape)
                off += align(n)
        distributed.broadcast_(self.flat, 0, process_group)      # replicas start from rank 0's parameters (as under DDP)
        ops.note_param_write()                 # the parameters were written through the bucket, not through themselves
        if hasattr(model, '_graphs'):
            model._graphs = {}                  # captured scoring graphs hold the parameters' old addresses
        self.step_count = 0
        self.last_norm = None

    @staticmethod
    def bucket_names(model):
        """The parameters of the flat bucket, in bucket order: every trainable parameter (once: the user encoder's view of the news
        encoder repeats names) that the reference's backward gives a gradient -- ``dead_parameters(model)`` are left out."""
        dead = set(dead_parameters(model)) if hasattr(model, 'user_encoder') else None
        names, seen = [], set()
        for name, p in model.named_parameters():
            if not p.requires_grad or id(p) in seen:
                continue
            seen.add(id(p))
            if name in dead if dead is not None else any(d in name for d in _DEAD):
                continue
            names.append(name)
        return names

    def backward(self, loss):
        """``loss.backward()`` with the gradients landing in the flat bucket.  The parameters' ``.grad`` views are taken away for
        the duration of the backward pass, so autograd hands every parameter its gradient tensor as it is (no accumulation
        kernel: with the views in place AccumulateGrad runs one ``grad += g`` launch per parameter, 72 a step, and the bucket has
        to be zeroed first); the tensors are then gathered into the bucket with one ``lime_multi_copy`` launch per 32
        parameters and the views are put back.  A parameter that received no gradient in this step gets zeros."""
        self._check_bucket()
        views = [p.grad for _, p in self._params]
        for _, p in self._params:
            p.grad = None
        try:
            loss.backward()
            pairs = []
            for (_, p), v in zip(self._params, views):
                if p.grad is None:
                    v.zero_()
                else:
                    pairs.append((v, p.grad))
            keep = ops.multi_copy(pairs)
        finally:
            for (_, p), v in zip(self._params, views):
                p.grad = v
        del keep

    def backward_and_update(self, loss):
        """loss.backward() into the flat bucket, all-reduce, clip, Adam.  Returns the (device) gradient norm."""
        self.backward(loss)
        distributed.allreduce_mean_(self.grad, self.group)
        return self.update()

    def _check_bucket(self):
        """Parameters and their .grad must still be the views into the flat buckets this object set up: ``model.zero_grad()``
        (set_to_none), ``model.to(...)`` or a foreign optimizer would silently detach them."""
        pb, gb = self.flat.data_ptr(), self.grad.data_ptr()
        for name, p in self._params:
            if p.grad is None or p.grad.data_ptr() - gb != p.data_ptr() - pb or not (0 <= p.data_ptr() - pb < self.flat.numel() * 4):
                raise RuntimeError('TrainStep: parameter %s (or its .grad) no longer lives in the flat bucket -- do not call '
                                   'model.zero_grad() / model.to() after constructing TrainStep (it zeroes the bucket itself)' % name)

    def update(self):
        self.step_count += 1
        coef = ops.grad_clip_coef(self.grad, self.clip)
        ops.adam_step_(self.flat, self.grad, self.exp_avg, self.exp_avg_sq, self.step_count, self.lr, self.betas, self.eps,
                       self.weight_decay, grad_scale=coef[1:])
        self.last_norm = coef[:1]
        return self.last_norm

    # ---- checkpoint / resume ------------------------------------------------------------------------------------------
    def state_dict(self):
        """Optimizer state for resuming: Adam's moments per parameter NAME (so it survives a different bucket layout), the step
        count and the hyper-parameters.  The model itself is saved the reference's way: {model_name: model.state_dict()}
        (trainer.py:220), see ``save_checkpoint``."""
        out = {'step': self.step_count, 'lr': self.lr, 'weight_decay': self.weight_decay, 'betas': tuple(self.betas), 'eps': self.eps,
               'gradient_clip_norm': self.clip, 'exp_avg': {}, 'exp_avg_sq': {}}
        for name, (off, n, shape) in self._slots().items():
            out['exp_avg'][name] = self.exp_avg[off:off + n].view(shape).clone()
            out['exp_avg_sq'][name] = self.exp_avg_sq[off:off + n].view(shape).clone()
        return out

    def load_state_dict(self, state):
        slots = self._slots()
        missing = sorted(set(slots) - set(state['exp_avg']))
        if missing:
            raise KeyError('optimizer state lacks %d parameters, e.g. %s' % (len(missing), missing[:3]))
        with torch.no_grad():
            for name, (off, n, shape) in slots.items():
                self.exp_avg[off:off + n].copy_(state['exp_avg'][name].reshape(-1))
                self.exp_avg_sq[off:off + n].copy_(state['exp_avg_sq'][name].reshape(-1))
        self.step_count = int(state['step'])
        self.lr, self.weight_decay, self.eps = state['lr'], state['weight_decay'], state['eps']
        self.betas, self.clip = tuple(state['betas']), state['gradient_clip_norm']

    def _slots(self):
        named = dict(self.model.named_parameters())
        base = self.flat.data_ptr()
        return {n: ((named[n].data_ptr() - base) // 4, named[n].numel(), tuple(named[n].shape)) for n in self.names}

    def step(self, *batch):
        """One training step on a batch in ``Model.forward``'s 26-tensor order; returns the (device) loss: the click loss plus the
        category-prediction loss where the forward left one (the sum the reference's trainer prints)."""
        logits = self.model(*batch)
        loss = negative_log_softmax(logits)
        aux = getattr(getattr(self.model, 'news_encoder', None), 'auxiliary_loss', None)
        if aux is not None:
            loss = loss + aux
        self.backward_and_update(loss)
        return loss.detach()


def save_checkpoint(path, model, train_step=None):
    """The reference's checkpoint file -- torch.save({model.model_name: model.state_dict()}) (trainer.py:220), which main.py:45,
    60 load with ``torch.load(path)[model.model_name]`` -- plus, under the extra key 'optimizer', the TrainStep state when
    one is given (the reference saves none: its runs cannot resume mid-training)."""
    payload = {model.model_name: {k: v.detach().cpu() for k, v in model.state_dict().items()}}
    if train_step is not None:
        st = train_step.state_dict()
        for key in ('exp_avg', 'exp_avg_sq'):
            st[key] = {k: v.cpu() for k, v in st[key].items()}
        payload['optimizer'] = st
    torch.save(payload, path)


def load_checkpoint(path, model, train_step=None, map_location='cpu'):
    """Load a checkpoint written by ``save_checkpoint`` or by the reference's trainer (tensors only: weights_only=True).
    Parameters keep their storage (``load_state_dict`` copies in place), so a TrainStep's flat bucket stays valid."""
    payload = torch.load(path, map_location=map_location, weights_only=True)
    if model.model_name not in payload:
        raise KeyError('checkpoint holds %s, not %r' % (sorted(payload), model.model_name))
    model.load_state_dict(payload[model.model_name])
    if train_step is not None and 'optimizer' in payload:
        train_step.load_state_dict(payload['optimizer'])
    return payload
