"""Drop-ins for the three attention primitives of the scoring path (reference layers.py:15-93,
192-238, 269-300).  The modules own parameters under the reference's names (so reference
checkpoints load); ``forward`` runs the hand-written HIP kernels through lime_cikm25_amd.ops.
"""
import math

import torch
import torch.nn as nn

from . import ops


class CandidateAware_ClickedNewsAttention(nn.Module):
    """layers.py:15-93.  Q/K topic projections on the fp32 MFMA GEMM, per-head softmax + query-weighted
    aggregation in one workgroup per impression row, gate_proj on the GEMM, gated residual + LayerNorm in one
    row kernel.  ``value_proj`` is kept for the state_dict only: its branch is dead in the
    reference (layers.py:68,76-77)."""

    def __init__(self, config, news_encoder):
        super().__init__()
        self.topic_embedding_dim = config.category_embedding_dim
        self.use_residual_connection = config.use_residual_connection
        self.news_embedding_dim = news_encoder.news_embedding_dim
        self.num_heads = 10
        self.head_dim = self.news_embedding_dim // self.num_heads
        assert self.news_embedding_dim % self.num_heads == 0, 'embedding_dim must be divisible by num_heads'
        self.query_proj = nn.Linear(self.topic_embedding_dim, self.news_embedding_dim)
        self.key_proj = nn.Linear(self.topic_embedding_dim, self.news_embedding_dim)
        self.value_proj = nn.Linear(self.news_embedding_dim, self.news_embedding_dim)
        self.scale = self.news_embedding_dim ** 0.5
        self.dropout = nn.Dropout(p=0.2)
        self.gate_proj = nn.Linear(self.news_embedding_dim, self.news_embedding_dim)
        self.layernorm = nn.LayerNorm(self.news_embedding_dim)

    def initialize(self):
        nn.init.xavier_uniform_(self.query_proj.weight)
        nn.init.xavier_uniform_(self.key_proj.weight)
        nn.init.zeros_(self.query_proj.bias)
        nn.init.zeros_(self.key_proj.bias)
        nn.init.xavier_uniform_(self.value_proj.weight)
        nn.init.zeros_(self.value_proj.bias)
        nn.init.xavier_uniform_(self.gate_proj.weight)
        nn.init.zeros_(self.gate_proj.bias)

    def attention_weights(self, clicked_news_topic_embeddings, candidate_topic_embeddings, mask=None, hist_div=1):
        """agg [B, H] of layers.py:66-81: topic projections, per-head masked softmax, query-norm weighting, outer softmax.
        ``hist_div`` > 1: the history side ([B / hist_div, H, .], mask [B / hist_div, H]) is shared by hist_div consecutive candidate rows."""
        Bh, H, _ = clicked_news_topic_embeddings.shape
        B = Bh * hist_div
        N = candidate_topic_embeddings.shape[1]
        D = self.news_embedding_dim
        if mask is None:
            mask = torch.ones(Bh, H, dtype=torch.bool, device=clicked_news_topic_embeddings.device)
        qp = ops.linear(candidate_topic_embeddings.reshape(B * N, -1), self.query_proj.weight, self.query_proj.bias)
        kp = ops.linear(clicked_news_topic_embeddings.reshape(Bh * H, -1), self.key_proj.weight, self.key_proj.bias)
        return ops.cand_attn_weights(qp, kp, mask, B, N, H, D, self.num_heads, hist_div=hist_div)

    def refine(self, clicked_news_embeddings, agg):
        """layers.py:83-91: weighted history, gated residual, LayerNorm."""
        B, H, D = clicked_news_embeddings.shape
        hist = clicked_news_embeddings.reshape(B * H, D)
        if self.use_residual_connection:
            y = ops.linear(hist, self.gate_proj.weight, None)                       # W_g x; the row scale commutes
            out = ops.gate_ln(y, hist, agg.view(-1), self.gate_proj.bias, self.layernorm.weight, self.layernorm.bias,
                              self.layernorm.eps)
        else:
            out = ops.row_scale(hist, agg.view(-1))
        return out.view(B, H, D)

    def forward(self, clicked_news_embeddings, clicked_news_topic_embeddings, candidate_topic_embeddings, mask=None):
        """-> (refined history [B, H, D], attn_weights_agg [B, H]).  In training mode (autograd recording, or the layer's own
        p = 0.2 dropout active, layers.py:36,74) the call takes the differentiable kernels of ``training.candidate_aware``."""
        from . import training
        if training.wants_train_path(self, self.dropout.p):
            return training.candidate_aware(self, clicked_news_embeddings.float(), clicked_news_topic_embeddings.float(),
                                            candidate_topic_embeddings.float(), mask)
        agg = self.attention_weights(clicked_news_topic_embeddings, candidate_topic_embeddings, mask)
        return self.refine(clicked_news_embeddings, agg), agg


class MultiHeadAttention(nn.Module):
    """layers.py:192-238 (self-attention use, Q = K = V): three projections + the masked token-attention kernel."""

    def __init__(self, h, d_model, len_q, len_k, d_k, d_v):
        super().__init__()
        self.h, self.d_model, self.len_q, self.len_k, self.d_k, self.d_v = h, d_model, len_q, len_k, d_k, d_v
        self.out_dim = self.h * self.d_v
        self.attention_scalar = math.sqrt(float(self.d_k))
        self.W_Q = nn.Linear(d_model, self.h * self.d_k, bias=True)
        self.W_K = nn.Linear(d_model, self.h * self.d_k, bias=True)
        self.W_V = nn.Linear(d_model, self.h * self.d_v, bias=True)

    def initialize(self):
        for lin in (self.W_Q, self.W_K, self.W_V):
            nn.init.xavier_uniform_(lin.weight)
            nn.init.zeros_(lin.bias)

    def project(self, x2d=None, table=None, ids=None, m_dev=None):
        """[tokens, 3*h*d_k] packed q|k|v; the operand is either a dense [tokens, d_model] matrix or a gather.  m_dev: optional
        device-side row count (a compacted batch)."""
        assert self.d_k == self.d_v
        hd = self.h * self.d_k
        tokens = x2d.shape[0] if ids is None else ids.numel()
        src = x2d if ids is None else table
        # ONE GEMM against W_Q / W_K / W_V stacked row-wise (they share the input: one gather of the word rows instead of three,
        # and N = 3 h d_k = 600 fills two 320-column tiles where 200 wasted a fifth of a 256-column one)
        w = torch.cat([self.W_Q.weight, self.W_K.weight, self.W_V.weight], dim=0)
        b = torch.cat([self.W_Q.bias, self.W_K.bias, self.W_V.bias], dim=0)
        qkv = ops.linear(src, w, b, a_ids=ids, m_dev=m_dev)
        return qkv

    def attend(self, qkv, n_seq, S, mask, n_seq_dev=None):
        hd = self.h * self.d_k
        return ops.token_attention(qkv[:, :hd], qkv[:, hd:2 * hd], qkv[:, 2 * hd:], n_seq, S, self.h, self.d_k,
                                   1.0 / self.attention_scalar, key_mask=mask, n_seq_dev=n_seq_dev)

    def forward(self, Q, K, V, mask=None):
        if not (Q is K and K is V):
            raise NotImplementedError('only the self-attention use (newsEncoders.py:590) is on the scoring path')
        n_seq, S, _ = Q.shape
        qkv = self.project(Q.reshape(n_seq * S, -1))
        return self.attend(qkv, n_seq, S, mask).view(n_seq, S, self.out_dim)


class Attention(nn.Module):
    """layers.py:269-300: additive attention pooling.  affine1 + tanh on the GEMM, the score / masked softmax /
    weighted sum in one workgroup per sequence."""

    def __init__(self, feature_dim, attention_dim):
        super().__init__()
        self.affine1 = nn.Linear(feature_dim, attention_dim, bias=True)
        self.affine2 = nn.Linear(attention_dim, 1, bias=False)

    def initialize(self):
        nn.init.xavier_uniform_(self.affine1.weight, gain=nn.init.calculate_gain('tanh'))
        nn.init.zeros_(self.affine1.bias)
        nn.init.xavier_uniform_(self.affine2.weight)

    def forward(self, feature, mask=None):
        n_seq, S, D = feature.shape
        x = feature.reshape(n_seq * S, D)
        hidden = ops.linear(x, self.affine1.weight, self.affine1.bias, act='tanh')
        return ops.additive_pool(hidden, self.affine2.weight.view(-1), x, n_seq, S, mask=mask)


class Conv1D(nn.Module):
    """layers.py:98-135: parameter holder for the CNN content encoder's convolution (``conv`` for 'naive'; ``conv1`` .. ``conv3``, windows
    1 / 3 / 5 and cnn_kernel_num / 3 outputs each, for 'group3'), nn.Conv1d default initialisation as the reference leaves it.  The
    arithmetic is the windowed conv GEMM (ops.conv1d_window); ``forward`` is never used on the HIP path.

    Refused, as the reference refuses or fails on them: 'group4' (the assert of :100), 'group5' (its padding concatenation of :131-134
    fails on shape), an even window (output T - 1 long: the view / masked_fill of newsEncoders.py:557-559 fail), and 'group3' with a
    kernel count that is not a multiple of 3 (:105).  Not in the reference: the kernels need multiples of 4 for the per-conv output
    count (the weight gradient's dY rows and the data gradient's source rows are read 16 bytes at a time)."""

    def __init__(self, cnn_method, in_channels, cnn_kernel_num, cnn_window_size):
        super().__init__()
        if cnn_method == 'group4':
            raise ValueError("cnn_method 'group4': the reference's Conv1D asserts against it (layers.py:100)")
        if cnn_method == 'group5':
            raise NotImplementedError("cnn_method 'group5': the reference's padding concatenation fails on shape (layers.py:131-134)")
        if cnn_method not in ('naive', 'group3'):
            raise ValueError('unknown cnn_method %r' % (cnn_method,))
        self.cnn_method = cnn_method
        self.in_channels = in_channels
        if cnn_method == 'naive':
            if cnn_window_size <= 0 or cnn_window_size % 2 == 0:
                raise ValueError('cnn_window_size %d: an even window makes the reference output T - 1 tokens long '
                                 '(newsEncoders.py:557-559 fail)' % cnn_window_size)
            per_conv = cnn_kernel_num
            self.conv = nn.Conv1d(in_channels=in_channels, out_channels=cnn_kernel_num, kernel_size=cnn_window_size,
                                  padding=(cnn_window_size - 1) // 2)
        else:
            if cnn_kernel_num % 3 != 0:
                raise ValueError("cnn_method 'group3' needs cnn_kernel_num %% 3 == 0 (layers.py:105), got %d" % cnn_kernel_num)
            per_conv = cnn_kernel_num // 3
            self.conv1 = nn.Conv1d(in_channels=in_channels, out_channels=per_conv, kernel_size=1, padding=0)
            self.conv2 = nn.Conv1d(in_channels=in_channels, out_channels=per_conv, kernel_size=3, padding=1)
            self.conv3 = nn.Conv1d(in_channels=in_channels, out_channels=per_conv, kernel_size=5, padding=2)
        if per_conv % 4 or in_channels % 4:
            raise NotImplementedError('the windowed conv kernels need multiples of 4 for the outputs per convolution (%d) and the '
                                      'input width (%d)' % (per_conv, in_channels))

    def convs(self):
        """[(nn.Conv1d, first output column)] in the reference's concatenation order."""
        if self.cnn_method == 'naive':
            return [(self.conv, 0)]
        n = self.conv1.out_channels
        return [(self.conv1, 0), (self.conv2, n), (self.conv3, 2 * n)]

    def relu_into(self, a, T, out, ids=None, m_dev=None):
        """Conv1D + ReLU (layers.py:126-130) over M = sequences x T tokens -> out [M, cnn_kernel_num], each convolution into its column
        slice.  The word rows are a [M, C] (ids None) or a[ids]; m_dev: see ops.conv1d_window."""
        for conv, col in self.convs():
            ops.conv1d_window(a, ops.conv1d_pack(conv.weight), conv.kernel_size[0], T, ids=ids, bias=conv.bias, act='relu',
                              out=out[:, col:col + conv.out_channels], m_dev=m_dev)
        return out

    def forward(self, feature):
        raise NotImplementedError('Conv1D is a parameter holder: the CNN encoder runs ops.conv1d_window')


class Conv2D_Pool(nn.Module):
    """layers.py:138-190: parameter holder for the KCNN content encoder's knowledge-aware convolution -- nn.Conv2d(C, O, [w, 3]) over the
    [C, T, 3] stack of word / entity / context rows, i.e. a 1-D convolution over 3 C channels, ReLU, and the maximum over the first P
    positions (``conv`` for 'naive'; ``conv1`` .. ``conv3`` / ``conv4``, windows 1 / 2 / 3 (/ 4), for 'group3' / 'group4'); nn.Conv2d
    default initialisation as the reference leaves it.  The arithmetic is ops.conv_pool; ``forward`` is never used on the HIP path.

    Refused: 'group5' (the reference's assert of :141), group kernel counts that do not divide (:149, :154), and -- not in the
    reference -- a per-convolution output count or input width that is no multiple of 4 (the kernels read and write 16 bytes at a
    time)."""

    def __init__(self, cnn_method, in_channels, cnn_kernel_num, cnn_window_size, last_channel_num):
        super().__init__()
        if cnn_method == 'group5':
            raise NotImplementedError("cnn_method 'group5': the reference's Conv2D_Pool asserts against it (layers.py:141)")
        if cnn_method not in ('naive', 'group3', 'group4'):
            raise ValueError('unknown cnn_method %r' % (cnn_method,))
        self.cnn_method = cnn_method
        self.in_channels = in_channels
        self.last_channel_num = last_channel_num
        self.cnn_window_size = cnn_window_size
        if cnn_method == 'naive':
            if cnn_window_size <= 0:
                raise ValueError('cnn_window_size %d must be positive' % cnn_window_size)
            per_conv = cnn_kernel_num
            self.conv = nn.Conv2d(in_channels, cnn_kernel_num, kernel_size=[cnn_window_size, last_channel_num],
                                  padding=[(cnn_window_size - 1) // 2, 0])
        else:
            groups = 3 if cnn_method == 'group3' else 4
            if cnn_kernel_num % groups != 0:
                raise ValueError('cnn_method %r needs cnn_kernel_num %% %d == 0 (layers.py:149,154), got %d' % (cnn_method, groups, cnn_kernel_num))
            per_conv = cnn_kernel_num // groups
            self.conv1 = nn.Conv2d(in_channels, per_conv, kernel_size=[1, last_channel_num], padding=[0, 0])
            self.conv2 = nn.Conv2d(in_channels, per_conv, kernel_size=[2, last_channel_num], padding=[0, 0])
            self.conv3 = nn.Conv2d(in_channels, per_conv, kernel_size=[3, last_channel_num], padding=[1, 0])
            if groups == 4:
                self.conv4 = nn.Conv2d(in_channels, per_conv, kernel_size=[4, last_channel_num], padding=[1, 0])
        if per_conv % 4 or in_channels % 4:
            raise NotImplementedError('the conv + pool kernels need multiples of 4 for the outputs per convolution (%d) and the input '
                                      'width (%d)' % (per_conv, in_channels))

    def max_window(self):
        return max(conv.kernel_size[0] for conv, _, _, _, _ in self.convs(1 << 20))

    def convs(self, T):
        """[(nn.Conv2d, first output column, window w, left padding p, pooled positions P)] in the reference's concatenation order, for
        sequences of T tokens: 'naive' pools T - w + 1 positions (:169), the group convolutions T, T - 1, T - 2 (, T - 3) (:174-189)."""
        if self.cnn_method == 'naive':
            w = self.cnn_window_size
            return [(self.conv, 0, w, (w - 1) // 2, T - w + 1)]
        n = self.conv1.out_channels
        out = [(self.conv1, 0, 1, 0, T), (self.conv2, n, 2, 0, T - 1), (self.conv3, 2 * n, 3, 1, T - 2)]
        if self.cnn_method == 'group4':
            out.append((self.conv4, 3 * n, 4, 1, T - 3))
        return out

    def forward(self, feature):
        raise NotImplementedError('Conv2D_Pool is a parameter holder: the KCNN encoder runs ops.conv_pool')


class LSTMHolder(nn.LSTM):
    """nn.LSTM as a parameter holder (newsEncoders.py:449-450: one bidirectional layer, batch_first): the reference's parameter names and
    layout (weight_ih_l0 [4h, E], weight_hh_l0 [4h, h], the two biases, and the same four with ``_reverse``; gate order i, f, g, o).  The
    recurrence runs on the LSTM step kernel (ops.lstm); ``forward`` is never used on the HIP path."""

    def forward(self, *args, **kwargs):
        raise NotImplementedError('LSTMHolder is a parameter holder: the CNE encoder runs ops.lstm (csrc/lstm_f32.hip)')


class LinearHolder(nn.Linear):
    """nn.Linear as a parameter holder of the CNE encoder (its GEMMs run on ops.linear with the gate arithmetic fused or behind them)."""

    def forward(self, *args, **kwargs):
        raise NotImplementedError('LinearHolder is a parameter holder: the CNE encoder runs ops.linear')


class ScaledDotProduct_CandidateAttention(nn.Module):
    """layers.py:334-359, parameter holder: a_t = K(feature_t) . Q(query) / sqrt(attention_dim), masked with -1e9, softmax, weighted sum
    of the features.  K has no bias, Q has one.  K(h_t) . q = h_t . (K^T q), so the CNE encoder computes one vector K^T q per sequence
    and pools with it (newsEncoders.CNE)."""

    def __init__(self, feature_dim, query_dim, attention_dim):
        super().__init__()
        self.K = LinearHolder(feature_dim, attention_dim, bias=False)
        self.Q = LinearHolder(query_dim, attention_dim, bias=True)
        self.attention_scalar = math.sqrt(float(attention_dim))

    def initialize(self):
        nn.init.xavier_uniform_(self.K.weight)
        nn.init.xavier_uniform_(self.Q.weight)
        nn.init.zeros_(self.Q.bias)

    def forward(self, *args, **kwargs):
        raise NotImplementedError('ScaledDotProduct_CandidateAttention is a parameter holder: the CNE encoder runs its pooling kernels')
