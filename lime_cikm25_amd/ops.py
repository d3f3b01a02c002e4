"""Tensor-level wrappers over the C ABI (include/lime_hip.h): shape/dtype/device checks on the host,
then one call into liblime_hip.so on torch's current stream.  PyTorch is used here for device memory
and streams only -- every wrapper launches hand-written HIP kernels and nothing else.

2-D operands may be row-strided views (``stride(1) == 1``); the row stride is passed as the leading
dimension, so slices like ``qkv[:, 300:600]`` or ``fused[:, 900:]`` cost nothing.
"""
import collections
import ctypes
import math
import os

import torch

from . import _lib
from ._lib import LinearArgs, LIME_ACT, check


# bench.py sets this to a list to collect (variant, M, N, K, start_event, end_event) per lime_linear_f32 launch:
# HIP events recorded on the launch stream right around the launch (never used otherwise)
PROFILE = None


# Counts the writes to parameter memory that torch cannot see: a kernel handed a raw pointer (the native Adam step over the flat
# bucket) moves no tensor's ``_version``.  Everything derived from weights and kept across forwards (kept.weight_state)
# compares this counter as well; whoever adds such a writer calls ``note_param_write()``.
PARAM_WRITES = 0


def note_param_write():
    global PARAM_WRITES
    PARAM_WRITES += 1


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _mat(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError('%s must be a CUDA tensor (the HIP path has no CPU fallback)' % name)
    if t.dtype != dtype:
        raise TypeError('%s must be %s, got %s' % (name, dtype, t.dtype))
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError('%s must be 2-D with unit column stride, got shape %s strides %s' % (name, tuple(t.shape), t.stride()))
    return t


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _vec(t, name, n=None, dtype=torch.float32):
    if t is None:
        return None
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise TypeError('%s must be a contiguous CUDA %s tensor' % (name, dtype))
    if n is not None and t.numel() != n:
        raise ValueError('%s must have %d elements, got %d' % (name, n, t.numel()))
    return t


def _mask_u8(mask, name):
    """bool/uint8 mask -> uint8 view (zero-copy)."""
    if mask is None:
        return None
    if mask.dtype == torch.bool:
        mask = mask.contiguous().view(torch.uint8)
    return _vec(mask, name, dtype=torch.uint8)


def set_split_gemm(on, force=False):
    """Route the big lime_linear_f32 problems through the split-product kernel (True, the default: fp32-level products on the bf16
    matrix cores, csrc/gemm_sp_f32.hip) or the fp32-MFMA kernels (False).  ``force``: also the launches the dispatcher leaves to the
    other kernels because few 256-row tiles would fill the chip badly, and -- with ``on`` False -- the big-M fp32 kernel for problems the
    dispatcher gives to the 64-row-tile kernel for the same reason (tests).  Returns the previous setting (True / False)."""
    return bool(_lib.load().lime_set_split_gemm((5 if force else 1) if on else (4 if force else 0)) & 1)


def linear(a, w, bias=None, act=None, out=None, a_ids=None, a_pe=None, a_period=0, res=None, res_div=1, res_ids=None,
           res_pe=None, res_period=0, ln=None, ln_eps=1e-5, res_mod=0, pool32=False, ln_rstd=None, n_alg=None, m_dev=None,
           c_ids=None, act_scale=1.0, dropout=None, _build_only=False):
    """C = epilogue(A . W^T + bias) -- see ``lime_linear_f32`` in include/lime_hip.h.

    n_alg: the number of USEFUL output columns when w carries zero padding rows (in_proj with heads padded to 32 columns:
    900 of 960); only bench.py's per-kernel FLOP accounting reads it.
    m_dev: int32 device tensor (1 element): the launch computes min(m_dev, M) rows, M being the capacity of the buffers.
    c_ids: int32 [M]: result row r is stored at out[c_ids[r]] (out is then passed in, any number of rows) and the periodic
    residual is res[c_ids[r] % res_mod] -- the in_proj over a compacted token list (``compact_sequences``).

    a: [M, K] (or the [V, K] table when a_ids is given, M = len(a_ids)); w: [N, K]; out: [M, N] (may be a view).
    ln: (gamma, beta) for the fused LayerNorm (N <= 320); ln_rstd: optional [M] output of the rows' 1 / sqrt(var + eps).
    """
    lib = _lib.load()
    _mat(a, 'a')
    _mat(w, 'w')
    N, K = w.shape
    if a.shape[1] != K:
        raise ValueError('a has %d columns, w has K=%d' % (a.shape[1], K))
    if a_ids is not None:
        _vec(a_ids, 'a_ids', dtype=torch.int32)
        M = a_ids.numel()
    else:
        M = a.shape[0]
    rows_out = M // 32 if pool32 else M
    if pool32 and M % 32:
        raise ValueError('pool32 needs M %% 32 == 0 (M = %d)' % M)
    if out is None:
        out = torch.empty((rows_out, N), dtype=torch.float32, device=a.device)
    _mat(out, 'out')
    if c_ids is not None:
        if out.shape[1] != N or res_mod <= 0:
            raise ValueError('c_ids needs an [*, N] out and a periodic residual (res_mod > 0)')
        args_c_ids = _vec(c_ids, 'c_ids', M, dtype=torch.int32)
    elif tuple(out.shape) != (rows_out, N):
        raise ValueError('out must be [%d, %d], got %s' % (rows_out, N, tuple(out.shape)))
    args = LinearArgs()
    if c_ids is not None:
        args.c_ids = args_c_ids.data_ptr()
    if m_dev is not None:
        args.m_dev = _vec(m_dev, 'm_dev', 1, dtype=torch.int32).data_ptr()
    args.pool32 = 1 if pool32 else 0
    args.a, args.lda = a.data_ptr(), _ld(a)
    args.a_ids = a_ids.data_ptr() if a_ids is not None else None
    if a_pe is not None:
        _mat(a_pe, 'a_pe')
        if a_pe.shape[1] != K or a_pe.shape[0] < a_period or a_period <= 0:
            raise ValueError('a_pe must be [>=a_period, K]')
        args.a_pe, args.lda_pe, args.a_period = a_pe.data_ptr(), _ld(a_pe), a_period
    args.w, args.ldw = w.data_ptr(), _ld(w)
    args.bias = _vec(bias, 'bias', N).data_ptr() if bias is not None else None
    if res is not None:
        _mat(res, 'res')
        if res.shape[1] != N:
            raise ValueError('res must have N=%d columns' % N)
        args.res, args.ldr, args.res_div = res.data_ptr(), _ld(res), res_div
        if res_ids is not None:
            _vec(res_ids, 'res_ids', M, dtype=torch.int32)
            args.res_ids = res_ids.data_ptr()
            if res_pe is not None:
                _mat(res_pe, 'res_pe')
                if res_pe.shape[1] != N or res_pe.shape[0] < res_period or res_period <= 0:
                    raise ValueError('res_pe must be [>=res_period, N]')
                args.res_pe, args.ldr_pe, args.res_period = res_pe.data_ptr(), _ld(res_pe), res_period
        elif res_mod > 0:
            if res.shape[0] < res_mod:
                raise ValueError('res has %d rows, res_mod is %d' % (res.shape[0], res_mod))
            args.res_mod = res_mod
        elif res.shape[0] * res_div < M:
            raise ValueError('res has %d rows, needs >= %d' % (res.shape[0], (M + res_div - 1) // res_div))
    if ln is not None:
        args.ln_gamma = _vec(ln[0], 'ln gamma', N).data_ptr()
        args.ln_beta = _vec(ln[1], 'ln beta', N).data_ptr()
        args.ln_eps = ln_eps
        if ln_rstd is not None:
            args.ln_rstd = _vec(ln_rstd, 'ln_rstd', M).data_ptr()
    args.c, args.ldc = out.data_ptr(), _ld(out)
    args.M, args.N, args.K = M, N, K
    args.act = LIME_ACT[act]
    args.act_scale = act_scale
    if dropout is not None and dropout[0] > 0:          # (p, seed, site): nn.Dropout behind the activation, counter-based mask
        args.dropout_p, args.dropout_seed, args.dropout_site = dropout
    if ln is not None and M >= 4096 and not _SLOW_LN_WARNED and not _friendly16(a, w, out, res):
        # the LayerNorm epilogue of a big problem whose operands are not 16-byte friendly runs on the general kernel's 5-tile-wide
        # instantiation (256 registers in scratch, a tenth of the LDS-DMA kernels' rate): say so once instead of being silently slow
        import warnings
        warnings.warn('lime_linear_f32: LayerNorm epilogue on operands that are not 16-byte aligned with leading dimensions that are '
                      'multiples of 4 (M = %d): this takes the slow general kernel; pass contiguous / aligned views' % M, RuntimeWarning)
        globals()['_SLOW_LN_WARNED'] = True
    if _build_only:
        return args, out
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib.lime_linear_f32(ctypes.byref(args), _stream()), 'lime_linear_f32')
        e1.record()
        m_run = M if m_dev is None else min(M, int(m_dev.item()))      # the rows this launch computed
        gathered = m_run * K * 4 if a_ids is not None else 0          # bytes of table rows this launch gathered as its A operand
        PROFILE.append((lib.lime_last_linear_kernel().decode(), m_run, N, K, n_alg or N, e0, e1, gathered))
        return out
    check(lib.lime_linear_f32(ctypes.byref(args), _stream()), 'lime_linear_f32')
    return out


def linear_plan(*args, n_cu=None, **kw):
    """What ``linear`` would run for the same arguments, without running it (``lime_linear_plan_f32``): a dict with ``family``
    ('sp' split product, 'pp' fp32 LDS-DMA, 'mid', 'general'; None for M = 0), ``kernel`` (the instantiation as
    ``lime_last_linear_kernel()`` names it after the launch), ``relu_bwd`` / ``dropout`` (a second pass over the output follows the
    GEMM), ``mid_shape`` (0 / 1 / 2, -1 off the mid-M kernel) and ``tiles``.  n_cu: the CU count to plan for (None: this device's).
    A call ``linear`` would refuse raises the same LimeHipError."""
    built, _ = linear(*args, _build_only=True, **kw)
    plan = _lib.LinearPlan()
    check(_lib.load().lime_linear_plan_f32(ctypes.byref(built), n_cu or 0, ctypes.byref(plan)), 'lime_linear_plan_f32')
    return dict(family=_lib.LINEAR_FAMILY[plan.family], kernel=plan.name.decode(), relu_bwd=bool(plan.second_pass & _lib.LINEAR_PASS_RELU_BWD),
                dropout=bool(plan.second_pass & _lib.LINEAR_PASS_DROPOUT), mid_shape=plan.mid_shape, tiles=plan.tiles)


_SLOW_LN_WARNED = False


def _friendly16(*tensors):
    return all(t is None or (t.data_ptr() % 16 == 0 and _ld(t) % 4 == 0) for t in tensors)


GROUP_SMALL_GEMMS = True      # False: linear_group issues its problems one by one (A/B runs, tests)


def linear_group(problems):
    """Several INDEPENDENT small GEMMs in one launch (``lime_linear_group_f32``): ``problems`` is a list of dicts of ``linear``'s
    arguments; returns the list of outputs.  The launches around the encoders are latency bound (>= 10 us each however small), so two
    that do not depend on each other cost one launch's time side by side.  Falls back to separate launches when a problem is outside
    the mid-M kernel (large M, LayerNorm, misaligned operands), under bench.py's per-kernel timing pass, or with GROUP_SMALL_GEMMS off."""
    if len(problems) == 1 or not GROUP_SMALL_GEMMS or PROFILE is not None or len(problems) > 8:
        return [linear(**kw) for kw in problems]
    lib = _lib.load()
    built = [linear(_build_only=True, **kw) for kw in problems]
    # A hand-written subset of what lime_linear_f32 routes to the mid-M kernel (linear_route in csrc/gemm_f32.hip; DESIGN.md section 5,
    # "Routing"): M < 4096, or below 12288 rows with an epilogue the split-product kernel takes from there on only (tanh / sigmoid,
    # broadcast or gathered residual without LayerNorm).  The C rule is wider and depends on the split mode: from 4096 rows on it also
    # hands the mid-M kernel every problem with fewer than 160 tiles of 128 x 256, and whatever neither big-M kernel takes; with the
    # fill rules off (set_split_gemm(force=True)) the split-product kernel takes tanh / sigmoid from 4096 rows on, which this
    # predicate still groups.  linear_plan() states the C rule exactly; switching to it changes which launches merge, so it waits
    # for a measurement.
    mid = lambda a: a.M < 4096 or (a.M < 12288 and (a.act in (2, 3) or (a.res and (a.res_ids or a.res_div > 1))))
    if any(not mid(a) or a.ln_gamma or a.pool32 or a.c_ids or a.a_pe or a.res_pe or a.K % 4 or a.N % 4 or a.K < 16 for a, _ in built):
        return [linear(**kw) for kw in problems]
    arr = (LinearArgs * len(built))()
    for i, (a, _) in enumerate(built):
        ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(a), ctypes.sizeof(LinearArgs))
    st = lib.lime_linear_group_f32(arr, len(built), _stream())
    if st == -2:                                       # LIME_ERR_UNSUPPORTED                # e.g. a misaligned view: the general kernels take it
        return [linear(**kw) for kw in problems]
    check(st, 'lime_linear_group_f32')
    return [out for _, out in built]


def embed_pe(ids, table, pe=None, period=0, out=None):
    """out[r] = table[ids[r]] + pe[r % period]; ids int32 [rows]."""
    lib = _lib.load()
    _vec(ids, 'ids', dtype=torch.int32)
    _mat(table, 'table')
    rows, dim = ids.numel(), table.shape[1]
    if out is None:
        out = torch.empty((rows, dim), dtype=torch.float32, device=table.device)
    _mat(out, 'out')
    if pe is not None:
        _mat(pe, 'pe')
    check(lib.lime_embed_pe_f32(_p(ids), _p(table), _ld(table), _p(pe), _ld(pe) if pe is not None else 0, period, _p(out),
                                _ld(out), rows, dim, _stream()), 'lime_embed_pe_f32')
    return out


NOT_APPLICABLE = _lib.CONSTANTS['LIME_NOT_APPLICABLE']


def _token_attention_block(form, q=None, k=None, v=None, n_seq=0, S=0, n_head=0, head_dim=0, scale=1.0, key_mask=None, out=None,
                           head_stride=None, n_seq_dev=None, lse=None, row_map=None, qkv_vocab=None, pos_rows=None, ids=None, p=0.0,
                           seed=0, site=0):
    """(lime_token_attention_args, out, what the block points into and nobody else holds) for the arguments of the fp32 forward wrapper
    of ``form`` ('plain' / 'count' / 'lse': ``token_attention``; 'rows': ``token_attention_rows``; 'vocab': ``token_attention_vocab``;
    'dropout': ``token_attention_dropout``): that wrapper's operand checks, the output where none was given and the dropout form's
    workspace, for the call and for its plan."""
    lib = _lib.load()
    a = _lib.TokenAttentionArgs()
    a.form = _lib.ATTN_FORM[form]
    hs = 32 if form in ('rows', 'vocab') else (head_dim if head_stride is None else head_stride)
    ptr = lambda t: None if t is None else t.data_ptr()
    mask = ws = None
    if form == 'vocab':
        _mat(qkv_vocab, 'qkv_vocab')
        _mat(pos_rows, 'pos_rows')
        W = n_head * 32
        if qkv_vocab.shape[1] != 3 * W or pos_rows.shape[1] != 3 * W or _ld(qkv_vocab) != _ld(pos_rows):
            raise ValueError('qkv_vocab and pos_rows must have 3 * n_head * 32 columns and one leading dimension')
        if pos_rows.shape[0] < S:
            raise ValueError('pos_rows must have at least S rows')
        _vec(ids, 'ids', dtype=torch.int32)
        if ids.numel() < n_seq * S:
            raise ValueError('ids must cover n_seq * S tokens')
        a.q, a.k, a.v = (qkv_vocab.data_ptr() + 4 * W * i for i in range(3))          # q | k | v side by side in the table's rows
        a.ld_qkv, a.pos_rows, a.row_map, device = _ld(qkv_vocab), ptr(pos_rows), ptr(ids), qkv_vocab.device
    else:
        for t, n in ((q, 'q'), (k, 'k'), (v, 'v')):
            _mat(t, n)
            if form == 'rows':
                if t.shape[1] != n_head * 32:
                    raise ValueError('%s must have n_head * 32 columns' % n)
            elif tuple(t.shape) != (n_seq * S, n_head * hs):
                raise ValueError('%s must be [n_seq * S, n_head * head_stride]' % n if form == 'dropout' else
                                 '%s must be [%d, %d]' % (n, n_seq * S, n_head * hs))
        if not (_ld(q) == _ld(k) == _ld(v)):
            raise ValueError('q, k, v must share one leading dimension' if form == 'dropout' else 'q, k and v must share one leading dimension')
        a.q, a.k, a.v, a.ld_qkv, device = ptr(q), ptr(k), ptr(v), _ld(q), q.device
    if form == 'rows':
        _vec(row_map, 'row_map', dtype=torch.int32)
        if row_map.numel() < n_seq * S:
            raise ValueError('row_map must cover n_seq * S tokens')
        a.row_map = ptr(row_map)
    if form in ('rows', 'vocab', 'count') and n_seq_dev is not None:           # a compacted batch: the sequence count lives on the device
        a.n_seq_dev = ptr(_vec(n_seq_dev, 'n_seq_dev', 1, dtype=torch.int32))
    if out is None:
        out = torch.empty((n_seq * S, n_head * head_dim), dtype=torch.float32, device=device)
    _mat(out, 'out')
    if form == 'vocab' and (out.shape[0] != n_seq * S or out.shape[1] != n_head * head_dim):
        raise ValueError('out must be [n_seq * S, n_head * head_dim]')
    if form in ('plain', 'count', 'lse'):
        mask = _mask_u8(key_mask, 'key_mask')
        if mask is not None and mask.numel() != n_seq * S:
            raise ValueError('key_mask must have n_seq * S elements')
        if form == 'lse':
            if mask is not None or n_seq_dev is not None:
                raise ValueError('lse goes with the unmasked, host-counted call')
            a.lse = ptr(_vec(lse, 'lse', n_seq * S * n_head))
        a.key_mask = ptr(mask)
    if form == 'dropout':
        need = 0 if head_dim > 32 else lib.lime_token_attention_stats_workspace(n_seq, S, n_head)      # the wide heads run in one pass
        ws = _workspace(device, need) if need else None
        a.workspace, a.workspace_floats = ptr(ws), ws.numel() if ws is not None else 0
        a.dropout_p, a.dropout_seed, a.dropout_site = p, seed, site
    a.out, a.ldo = out.data_ptr(), _ld(out)
    a.n_seq, a.S, a.n_head, a.head_dim, a.head_stride, a.scale = n_seq, S, n_head, head_dim, hs, scale
    return a, out, (mask, ws)


def _token_attention(form, **kw):
    """The one forward call: ``lime_token_attention_f32`` over the block of ``form``'s wrapper arguments.  None where the vocab form
    does not cover the call (nothing was launched)."""
    a, out, _keep = _token_attention_block(form, **kw)
    st = _lib.load().lime_token_attention_f32(ctypes.byref(a), _stream())
    if st == NOT_APPLICABLE:
        return None
    check(st, 'lime_token_attention_f32')
    return out


def token_attention(q, k, v, n_seq, S, n_head, head_dim, scale, key_mask=None, out=None, head_stride=None, n_seq_dev=None, lse=None):
    """softmax(Q K^T * scale [+mask]) V per (sequence, head); q/k/v: [n_seq*S, n_head*head_stride] views of one pitch
    (head_stride defaults to head_dim, the packed layout); out: [n_seq*S, n_head*head_dim].  ``lse`` (float32 [n_seq*S * n_head], no
    mask): also filled with the softmax statistics ``token_attention_bwd(..., lse=lse)`` reads instead of recomputing them.
    ``n_seq_dev`` (int32 device tensor, 1 element): a compacted batch, whose sequence count lives on the device.
    S <= 512 and either head_dim <= 32 (any head_dim, any head_stride >= head_dim) or the wide heads 32 < head_dim <= 128 with
    head_dim % 4 == 0, head_stride % 4 == 0, leading dimensions that are multiples of 4 and 16-byte aligned tensors."""
    form = 'lse' if lse is not None else ('count' if n_seq_dev is not None else 'plain')
    return _token_attention(form, q=q, k=k, v=v, n_seq=n_seq, S=S, n_head=n_head, head_dim=head_dim, scale=scale, key_mask=key_mask,
                            out=out, head_stride=head_stride, n_seq_dev=n_seq_dev, lse=lse)


def token_attention_rows(q, k, v, row_map, n_seq_dev, n_seq, S, n_head, head_dim, scale, out=None):
    """The rows form of ``lime_token_attention_f32``: attention over compacted sequences.  q / k / v: column views (heads 32 columns
    apart) of one buffer that also holds the S rows shared by the padding tokens; row_map: int32 [n_seq * S] -> row of that buffer;
    n_seq_dev: int32 device tensor (1 element) or None; out: [n_seq * S, n_head * head_dim] (rows of sequences beyond the
    device count are left untouched)."""
    return _token_attention('rows', q=q, k=k, v=v, row_map=row_map, n_seq_dev=n_seq_dev, n_seq=n_seq, S=S, n_head=n_head,
                            head_dim=head_dim, scale=scale, out=out)


def token_attention_vocab(qkv_vocab, pos_rows, ids, n_seq_dev, n_seq, S, n_head, head_dim, scale, out=None):
    """The vocab form of ``lime_token_attention_f32``: the first encoder layer's attention over a per-vocabulary in_proj product.
    qkv_vocab: [V, 3 * n_head * 32] (q | k | v, heads 32 columns apart); pos_rows: [>= S, same columns]; ids: int32 [>= n_seq * S] word
    ids (unchecked in [0, V)); the q / k / v row of token (seq, t) is ``qkv_vocab[ids[seq * S + t]] + pos_rows[t]``.  n_seq_dev as in
    ``token_attention_rows``.  Returns ``out`` [n_seq * S, n_head * head_dim], or None when the form does not cover the call (the
    split product switched off, S outside {32, 64, 128}, head_dim > 32): nothing was launched, the caller keeps the in_proj path."""
    return _token_attention('vocab', qkv_vocab=qkv_vocab, pos_rows=pos_rows, ids=ids, n_seq_dev=n_seq_dev, n_seq=n_seq, S=S, n_head=n_head,
                            head_dim=head_dim, scale=scale, out=out)


def token_attention_plan(form, q=None, k=None, v=None, n_seq=0, S=0, n_head=0, head_dim=0, scale=1.0, key_mask=None, out=None,
                         head_stride=None, n_seq_dev=None, lse=None, row_map=None, qkv_vocab=None, pos_rows=None, ids=None, p=0.0, seed=0,
                         site=0):
    """What the fp32 forward wrapper of ``form`` ('plain' / 'count' / 'lse': ``token_attention``; 'rows': ``token_attention_rows``;
    'vocab': ``token_attention_vocab``; 'dropout': ``token_attention_dropout``) would run for the same arguments, without running it
    (``lime_token_attention_plan_f32``): a dict with ``family`` ('sp', 'sp_long', 'sp_vocab', 'mfma', 'wide', 'dropout',
    'dropout_long'; None where nothing is launched), ``stats_pass`` (None / 'fp32' / 'split') and ``kernels`` (the instantiations in
    launch order, as rocprofv3 prints them).  None where the vocab form does not cover the call; a call the wrapper or the library would
    refuse raises the same error."""
    a, _out, _keep = _token_attention_block(form, q=q, k=k, v=v, n_seq=n_seq, S=S, n_head=n_head, head_dim=head_dim, scale=scale,
                                            key_mask=key_mask, out=out, head_stride=head_stride, n_seq_dev=n_seq_dev, lse=lse,
                                            row_map=row_map, qkv_vocab=qkv_vocab, pos_rows=pos_rows, ids=ids, p=p, seed=seed, site=site)
    plan = _lib.TokenAttentionPlan()
    st = _lib.load().lime_token_attention_plan_f32(ctypes.byref(a), ctypes.byref(plan))
    if st == NOT_APPLICABLE:
        return None
    check(st, 'lime_token_attention_plan_f32')
    return dict(family=_lib.ATTN_FAMILY[plan.family], stats_pass=_lib.ATTN_STATS[plan.stats_pass],
                kernels=[plan.name[i].value.decode() for i in range(plan.n_launches)])


class Compacted:
    """Index lists of ``compact_sequences`` (all int32 device tensors; see lime_compact_sequences in include/lime_hip.h)."""
    __slots__ = ('n_seq', 'S', 'cap', 'seq_inv', 'seq_src', 'ids_c', 'row_map', 'tok_ids', 'tok_rows', 'counts')

    n_compact = property(lambda self: self.counts[0:1])      # device counts as 1-element views (m_dev / n_seq_dev arguments)
    n_rows = property(lambda self: self.counts[1:2])
    n_live_tokens = property(lambda self: self.counts[2:3])
    n_tokens_and_pad_rows = property(lambda self: self.counts[4:5])     # live tokens + the S padding-row entries behind them in tok_ids / tok_rows


def compact_sequences(ids, pad_base=None):
    """ids int32 [n_seq, S] -> ``Compacted``: the live sequences (+ one all-padding representative) and their live tokens.
    pad_base: the q/k/v row where the S padding rows start (default: right behind the (n_seq + 1) * S compact rows)."""
    lib = _lib.load()
    if ids.dim() != 2 or ids.dtype != torch.int32 or not ids.is_cuda or not ids.is_contiguous():
        raise TypeError('ids must be a contiguous CUDA int32 [n_seq, S] tensor')
    n_seq, S = ids.shape
    cap = (n_seq + 1) * S
    c = Compacted()
    c.n_seq, c.S, c.cap = n_seq, S, cap
    dev = ids.device
    buf = torch.empty(n_seq + 4 * cap + 8 + int(lib.lime_compact_sequences_workspace(n_seq)), dtype=torch.int32, device=dev)
    c.seq_inv = buf[:n_seq]
    o = n_seq
    c.ids_c, c.row_map, c.tok_ids, c.tok_rows = (buf[o + i * cap:o + (i + 1) * cap] for i in range(4))
    o += 4 * cap
    c.counts = buf[o:o + 5]
    work = buf[o + 8:]
    c.seq_src = work[n_seq:2 * n_seq + 1]          # compact -> original sequence (-1: the all-padding representative)
    check(lib.lime_compact_sequences(_p(ids), n_seq, S, cap if pad_base is None else pad_base, _p(c.seq_inv), _p(c.ids_c), _p(c.row_map),
                                     _p(c.tok_ids), _p(c.tok_rows), _p(c.counts), _p(work), _stream()), 'lime_compact_sequences')
    return c


class NewsCompacted:
    """News-level lists of ``compact_batch`` (device tensors, capacity n + 1; see lime_compact_batch in include/lime_hip.h)."""
    __slots__ = ('n', 'news_src', 'news_inv', 'title_row', 'body_row', 'cat_c', 'sub_c', 'fresh_c', 'life_c', 'counts', 'count_mult',
                 'ready',                                    # ready: event behind the three launches, for consumers on other streams
                 'pair')                                     # the bucket pairs of the compact keys, once ``news_keys`` has run (else unset)

    n_news = property(lambda self: self.counts[0:1])         # device counts as 1-element views (m_dev arguments)
    n_news_mult = property(lambda self: self.counts[1:2])    # count_mult * n_news


def _compacted_views(c, buf, n_seq, S):
    """Carves ``Compacted``'s lists out of ``buf`` (``compact_sequences``' layout without the workspace); returns the words used."""
    cap = (n_seq + 1) * S
    c.n_seq, c.S, c.cap = n_seq, S, cap
    c.seq_inv = buf[:n_seq]
    o = n_seq
    c.ids_c, c.row_map, c.tok_ids, c.tok_rows = (buf[o + i * cap:o + (i + 1) * cap] for i in range(4))
    o += 4 * cap
    c.counts = buf[o:o + 5]
    return o + 8


def compact_batch(title_ids, body_ids, cat, sub, fresh, life, count_mult=1):
    """``compact_sequences`` for the titles [n, T] and the bodies [n, L] of n news and the news level on top, in three launches
    (``lime_compact_batch``).  cat / sub int32 [n], fresh / life float32 [n]: the rest of a news' key.  Returns
    (``Compacted`` title, ``Compacted`` body, ``NewsCompacted``)."""
    lib = _lib.load()
    for ids in (title_ids, body_ids):
        if ids.dim() != 2 or ids.dtype != torch.int32 or not ids.is_cuda or not ids.is_contiguous():
            raise TypeError('ids must be contiguous CUDA int32 [n, S] tensors')
    n, T = title_ids.shape
    L = body_ids.shape[1]
    if body_ids.shape[0] != n:
        raise ValueError('title_ids and body_ids must have one row per news')
    _vec(cat, 'cat', n, dtype=torch.int32)
    _vec(sub, 'sub', n, dtype=torch.int32)
    _vec(fresh, 'fresh', n)
    _vec(life, 'life', n)
    dev = title_ids.device
    words = lambda S: n + 4 * (n + 1) * S + 8
    buf = torch.empty(words(T) + words(L) + 8 * (n + 1) + 8 + int(lib.lime_compact_batch_workspace(n)), dtype=torch.int32, device=dev)
    t, b, w = Compacted(), Compacted(), NewsCompacted()
    o = _compacted_views(t, buf, n, T)
    o += _compacted_views(b, buf[o:], n, L)
    w.n, w.count_mult = n, count_mult
    w.news_src, w.title_row, w.body_row, w.cat_c, w.sub_c, fc, lc = (buf[o + i * (n + 1):o + (i + 1) * (n + 1)] for i in range(7))
    w.fresh_c, w.life_c = fc.view(torch.float32), lc.view(torch.float32)
    o += 7 * (n + 1)
    w.news_inv = buf[o:o + n]
    o += n + 1
    w.counts = buf[o:o + 4]
    work = buf[o + 8:]
    t.seq_src, b.seq_src = work[n:2 * n + 1], work[4 * n + 2:5 * n + 3]
    check(lib.lime_compact_batch(_p(title_ids), T, t.cap, _p(t.seq_inv), _p(t.ids_c), _p(t.row_map), _p(t.tok_ids), _p(t.tok_rows),
                                 _p(t.counts), _p(body_ids), L, b.cap, _p(b.seq_inv), _p(b.ids_c), _p(b.row_map), _p(b.tok_ids),
                                 _p(b.tok_rows), _p(b.counts), n, _p(cat), _p(sub), _p(fresh), _p(life), count_mult, _p(w.news_src),
                                 _p(w.news_inv), _p(w.title_row), _p(w.body_row), _p(w.cat_c), _p(w.sub_c), _p(w.fresh_c), _p(w.life_c),
                                 _p(w.counts), _p(work), _stream()), 'lime_compact_batch')
    w.ready = torch.cuda.Event()
    w.ready.record()
    return t, b, w


def news_xin(title_blocks, nblk_t, body_blocks, nblk_b, news, xin, dim):
    """``lime_news_xin_f32``: columns [0, dim) of xin [2 (n + 1), >= dim] from the pooled block rows of the distinct news: the title half
    in rows [0, n + 1), the body half behind it; rows at or beyond the device count ``news.n_news`` are left alone."""
    lib = _lib.load()
    _mat(title_blocks, 'title_blocks')
    _mat(body_blocks, 'body_blocks')
    _mat(xin, 'xin')
    cap = news.n + 1
    if title_blocks.shape != (cap * nblk_t, dim) or body_blocks.shape != (cap * nblk_b, dim):
        raise ValueError('title_blocks / body_blocks must be [(n + 1) * nblk, dim]')
    if xin.shape[0] != 2 * cap or xin.shape[1] < dim:
        raise ValueError('xin must be [2 (n + 1), >= dim]')
    check(lib.lime_news_xin_f32(_p(title_blocks), _ld(title_blocks), nblk_t, _p(body_blocks), _ld(body_blocks), nblk_b, _p(news.title_row),
                                _p(news.body_row), _p(news.n_news), _p(xin), _ld(xin), cap, dim, _stream()), 'lime_news_xin_f32')
    return xin


def pad_heads(src, n_blk, head_dim, head_stride):
    """[n_blk * head_dim, cols] (or a vector of n_blk * head_dim) -> rows padded with zeros to head_stride per block."""
    lib = _lib.load()
    vec = src.dim() == 1
    s2 = src.view(-1, 1) if vec else src
    _mat(s2, 'src')
    if s2.shape[0] != n_blk * head_dim:
        raise ValueError('src must have n_blk * head_dim rows')
    dst = torch.empty((n_blk * head_stride, s2.shape[1]), dtype=torch.float32, device=src.device)
    check(lib.lime_pad_heads_f32(_p(s2), _ld(s2), _p(dst), _ld(dst), n_blk, head_dim, head_stride, s2.shape[1], _stream()),
          'lime_pad_heads_f32')
    return dst.view(-1) if vec else dst


def mean_pool(x, n_seq, S, out=None, n_seq_dev=None):
    """out[s] = mean of the S rows of sequence s.  n_seq_dev: optional device-side int32 count (a compacted batch): only the
    first min(n_seq, count) sequences are read and written."""
    lib = _lib.load()
    _mat(x, 'x')
    if x.shape[0] != n_seq * S:
        raise ValueError('x must have n_seq * S rows')
    dim = x.shape[1]
    if out is None:
        out = torch.empty((n_seq, dim), dtype=torch.float32, device=x.device)
    _mat(out, 'out')
    if n_seq_dev is not None:
        _vec(n_seq_dev, 'n_seq_dev', dtype=torch.int32)
        check(lib.lime_mean_pool_count_f32(_p(x), _ld(x), _p(out), _ld(out), n_seq, S, dim, _p(n_seq_dev), _stream()),
              'lime_mean_pool_count_f32')
    else:
        check(lib.lime_mean_pool_f32(_p(x), _ld(x), _p(out), _ld(out), n_seq, S, dim, _stream()), 'lime_mean_pool_f32')
    return out


def bucketize(x, cuts=None):
    """int32 lifetime buckets (newsEncoders.py:53-58), bit-exact by threshold comparison.  cuts: fp32 device tensor of the
    num_buckets - 1 ascending cut points for num_buckets != 10 (the default table is built into the kernel)."""
    lib = _lib.load()
    x = _vec(x.contiguous(), 'x')
    out = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    if cuts is not None:
        _vec(cuts, 'cuts')
        check(lib.lime_bucketize_cuts_f32(_p(x), _p(cuts), cuts.numel(), _p(out), x.numel(), _stream()), 'lime_bucketize_cuts_f32')
        return out
    check(lib.lime_bucketize_f32(_p(x), _p(out), x.numel(), _stream()), 'lime_bucketize_f32')
    return out


def mhsa_live_ids(ids, mask):
    """``lime_mhsa_live_ids``: ids int32 [n, T], mask bool/uint8 [n, T] -> ids with the -1 sentinel of all-zero sequences that must be encoded."""
    lib = _lib.load()
    n, T = ids.shape
    m = _mask_u8(mask, 'mask')
    out = torch.empty_like(ids)
    check(lib.lime_mhsa_live_ids(_p(ids), _p(m), n, T, _p(out), _stream()), 'lime_mhsa_live_ids')
    return out


def mhsa_compact_mask(cmp, mask):
    """``lime_mhsa_compact_mask``: clamps ``cmp.ids_c`` in place and returns the key mask in compact order, uint8 [(n_seq + 1), S]."""
    lib = _lib.load()
    m = _mask_u8(mask, 'mask')
    mask_c = torch.empty((cmp.n_seq + 1, cmp.S), dtype=torch.uint8, device=cmp.ids_c.device)
    check(lib.lime_mhsa_compact_mask(_p(cmp.ids_c), _p(cmp.seq_src), _p(m), cmp.n_seq + 1, cmp.S, _p(mask_c), _stream()), 'lime_mhsa_compact_mask')
    return mask_c


def fuse_rows(a, b, gate=None, out=None):
    """LIME's 'add' / 'gated' fusion (newsEncoders.py:154-159): a + b, or gate * a + (1 - gate) * b; [rows, cols] matrices."""
    lib = _lib.load()
    _mat(a, 'a')
    _mat(b, 'b')
    if a.shape != b.shape or (gate is not None and gate.shape != a.shape):
        raise ValueError('a, b (and gate) must have one shape')
    if gate is not None:
        _mat(gate, 'gate')
    if out is None:
        out = torch.empty(tuple(a.shape), dtype=torch.float32, device=a.device)
    _mat(out, 'out')
    check(lib.lime_fuse_rows_f32(_p(a), _ld(a), _p(b), _ld(b), _p(gate), _ld(gate) if gate is not None else 0, _p(out), _ld(out),
                                 a.shape[0], a.shape[1], _stream()), 'lime_fuse_rows_f32')
    return out


def gather_rows(idx, table, out):
    lib = _lib.load()
    _vec(idx, 'idx', dtype=torch.int32)
    _mat(table, 'table')
    _mat(out, 'out')
    if out.shape[0] != idx.numel() or out.shape[1] != table.shape[1]:
        raise ValueError('out must be [len(idx), table.shape[1]]')
    check(lib.lime_gather_rows_f32(_p(idx), _p(table), _ld(table), _p(out), _ld(out), idx.numel(), table.shape[1], _stream()),
          'lime_gather_rows_f32')
    return out


# LIME.encode_cached with fusion_method 'concat' + project: the freshness half as lime_cached_occurrence_f32 (True) or as today's
# launches (False, the default: bucketize x 2, gather x 2, dense + tanh, the freshness half of `project` with the cache as a gathered
# residual).  The two forms associate the same sums differently (equal to fp32 rounding, DESIGN.md "Cached occurrences"), so the
# default stays until it is flipped on purpose; LIME_FUSED_OCCURRENCE=1 selects the kernel for the whole process.  'add' and 'gated'
# have the kernel only.
FUSED_OCCURRENCE = os.environ.get('LIME_FUSED_OCCURRENCE', '0') == '1'
OCC_MODES = {'concat': _lib.CONSTANTS['LIME_OCC_CONCAT'], 'add': _lib.CONSTANTS['LIME_OCC_ADD'], 'gated': _lib.CONSTANTS['LIME_OCC_GATED']}


def cached_occurrence(mode, idx, freshness, lifetime, A, T, P=None, Q=None, cuts=None, out=None):
    """``lime_cached_occurrence_f32``: out[r] = A[idx[r]] + T[pair[r]] ('concat', 'add') or g A[idx[r]] + (1 - g) T[pair[r]] with
    g = sigmoid(P[idx[r]] + Q[pair[r]]) ('gated'), pair = bucket(freshness) * nb + bucket(lifetime) -- the bucket rule of ``bucketize``
    (``cuts`` as there).  idx int32 [R] (every id in [0, A.shape[0]): not checked, like ``gather_rows``: a check would cost a host
    synchronise), freshness / lifetime fp32 [R]; A, P [n, D] and T, Q [nb^2, D] may be row-strided views (D % 4 == 0, 16-byte rows)."""
    lib = _lib.load()
    if mode not in OCC_MODES:
        raise ValueError('cached_occurrence: mode must be one of %s, got %r' % (sorted(OCC_MODES), mode))
    gated = mode == 'gated'
    if gated and (P is None or Q is None):
        raise ValueError("cached_occurrence: 'gated' needs P and Q")
    _mat(A, 'A')
    _mat(T, 'T')
    D = A.shape[1]
    R = _vec(idx, 'idx', dtype=torch.int32).numel()
    _vec(freshness, 'freshness', R)
    _vec(lifetime, 'lifetime', R)
    _vec(cuts, 'cuts')
    if T.shape[1] != D:
        raise ValueError('cached_occurrence: T has %d columns, A has %d' % (T.shape[1], D))
    if gated and (_mat(P, 'P').shape != A.shape or _mat(Q, 'Q').shape != T.shape):
        raise ValueError('cached_occurrence: P / Q must have the shapes of A / T')
    if out is None:
        out = torch.empty((R, D), dtype=torch.float32, device=A.device)
    if tuple(_mat(out, 'out').shape) != (R, D):
        raise ValueError('cached_occurrence: out must be [%d, %d], got %s' % (R, D, tuple(out.shape)))
    check(lib.lime_cached_occurrence_f32(OCC_MODES[mode], _p(idx), _p(freshness), _p(lifetime), _p(cuts), cuts.numel() if cuts is not None else 0,
                                         _p(A), _ld(A), _p(P) if gated else None, _ld(P) if gated else 0, _p(T), _ld(T),
                                         _p(Q) if gated else None, _ld(Q) if gated else 0, T.shape[0], _p(out), _ld(out), R, D, _stream()),
          'lime_cached_occurrence_f32')
    return out


def topic_rep(cat, sub, cat_table, sub_table, w=None, bias=None, out=None, emb_out=None):
    """category_affine(cat[cat_emb, sub_emb]) into ``out`` and/or the raw embedding pair into ``emb_out``."""
    lib = _lib.load()
    _vec(cat, 'cat', dtype=torch.int32)
    _vec(sub, 'sub', cat.numel(), dtype=torch.int32)
    _mat(cat_table, 'cat_table')
    _mat(sub_table, 'sub_table')
    if not (cat_table.is_contiguous() and sub_table.is_contiguous()):
        raise ValueError('embedding tables must be contiguous')
    rows, dc, ds = cat.numel(), cat_table.shape[1], sub_table.shape[1]
    dout = 0
    if w is not None:
        _mat(w, 'w')
        if not w.is_contiguous() or w.shape[1] != dc + ds:
            raise ValueError('w must be contiguous [dout, dc + ds]')
        dout = w.shape[0]
        if out is None:
            out = torch.empty((rows, dout), dtype=torch.float32, device=cat.device)
        _mat(out, 'out')
        if tuple(out.shape) != (rows, dout):
            raise ValueError('out must be [rows, dout]')
        _vec(bias, 'bias', dout)
    if emb_out is not None:
        _mat(emb_out, 'emb_out')
        if tuple(emb_out.shape) != (rows, dc + ds):
            raise ValueError('emb_out must be [rows, dc + ds]')
    check(lib.lime_topic_rep_f32(_p(cat), _p(sub), _p(cat_table), _p(sub_table), dc, ds, _p(w), _p(bias), dout,
                                 _p(out) if w is not None else None, _ld(out) if w is not None else 0, _p(emb_out),
                                 _ld(emb_out) if emb_out is not None else 0, rows, _stream()), 'lime_topic_rep_f32')
    return out


def news_keys(news, nb, cuts, cat_table, sub_table, w, bias, xin, col0, emb_out):
    """``lime_news_keys_f32``: one launch over the capacity of ``news`` (``NewsCompacted``) for what the tail takes from the compact
    keys -- returns pair int32 [n + 1] = bucket(fresh_c) * nb + bucket(life_c) (``bucketize``'s rule, ``cuts`` as there), and writes the
    ``topic_rep`` row of every compact news into columns [col0, col0 + dout) of both halves of xin [2 (n + 1), ldx], zeros into the
    columns behind them, and the raw embedding pair into emb_out [n + 1, dc + ds].  Columns [0, col0) of xin are left alone."""
    lib = _lib.load()
    rows = news.n + 1
    _mat(cat_table, 'cat_table')
    _mat(sub_table, 'sub_table')
    _mat(w, 'w')
    if not (cat_table.is_contiguous() and sub_table.is_contiguous()):
        raise ValueError('embedding tables must be contiguous')
    dc, ds = cat_table.shape[1], sub_table.shape[1]
    if not w.is_contiguous() or w.shape[1] != dc + ds:
        raise ValueError('w must be contiguous [dout, dc + ds]')
    dout = w.shape[0]
    _vec(bias, 'bias', dout)
    _vec(cuts, 'cuts')
    if cuts.numel() + 1 != nb if cuts is not None else nb != 10:
        raise ValueError('news_keys: %d buckets need %d cut points (None: the 10 buckets built in)' % (nb, nb - 1))
    _mat(xin, 'xin')
    if xin.shape[0] != 2 * rows or col0 < 0 or xin.shape[1] < col0 + dout or not xin.is_contiguous():
        raise ValueError('xin must be contiguous [2 (n + 1), >= col0 + dout]')
    _mat(emb_out, 'emb_out')
    if tuple(emb_out.shape) != (rows, dc + ds):
        raise ValueError('emb_out must be [n + 1, dc + ds]')
    pair = torch.empty((rows,), dtype=torch.int32, device=xin.device)
    check(lib.lime_news_keys_f32(_p(news.cat_c), _p(news.sub_c), _p(news.fresh_c), _p(news.life_c), _p(cuts),
                                 cuts.numel() if cuts is not None else 0, nb, _p(cat_table), _p(sub_table), dc, ds, _p(w), _p(bias), dout,
                                 _p(xin), xin.shape[1], col0, _p(emb_out), _ld(emb_out), _p(pair), rows, _stream()), 'lime_news_keys_f32')
    return pair


def intent_fuse(intents, att_hidden, affine2_t, affine2_b, content, M, k, D, A, m_dev=None):
    """intents [2*M*k, D], att_hidden [2*M*k, A] contiguous; writes content[:, :2D] (content may be a view).  m_dev (int32 device
    tensor, 1 element): only the first min(M, m_dev) news are read and written."""
    lib = _lib.load()
    _mat(intents, 'intents')
    _mat(att_hidden, 'att_hidden')
    if not (intents.is_contiguous() and att_hidden.is_contiguous()):
        raise ValueError('intents / att_hidden must be contiguous')
    if tuple(intents.shape) != (2 * M * k, D) or tuple(att_hidden.shape) != (2 * M * k, A):
        raise ValueError('intents / att_hidden have the wrong shape')
    _mat(content, 'content')
    if content.shape[0] != M or content.shape[1] < 2 * D:
        raise ValueError('content must be [M, >= 2D]')
    if m_dev is not None:
        check(lib.lime_intent_fuse_count_f32(_p(intents), _p(att_hidden), _p(_vec(affine2_t, 'affine2_t', A)),
                                             _p(_vec(affine2_b, 'affine2_b', A)), _p(content), _ld(content), M, k, D, A,
                                             _p(_vec(m_dev, 'm_dev', 1, dtype=torch.int32)), _stream()), 'lime_intent_fuse_count_f32')
        return content
    check(lib.lime_intent_fuse_f32(_p(intents), _p(att_hidden), _p(_vec(affine2_t, 'affine2_t', A)),
                                   _p(_vec(affine2_b, 'affine2_b', A)), _p(content), _ld(content), M, k, D, A, _stream()),
          'lime_intent_fuse_f32')
    return content


def additive_pool(hidden, affine2, x, n_seq, S, mask=None, out=None, n_seq_dev=None):
    """layers.Attention over the S tokens of each sequence (layers.py:285-300).  ``n_seq_dev`` (int32 device tensor, 1 element): only
    that many sequences are pooled (a compacted batch), the other output rows are left alone."""
    lib = _lib.load()
    _mat(hidden, 'hidden')
    _mat(x, 'x')
    A, D = hidden.shape[1], x.shape[1]
    if hidden.shape[0] != n_seq * S or x.shape[0] != n_seq * S:
        raise ValueError('hidden and x must have n_seq * S rows')
    if out is None:
        out = torch.empty((n_seq, D), dtype=torch.float32, device=x.device)
    _mat(out, 'out')
    m = _mask_u8(mask, 'mask')
    if n_seq_dev is not None:
        _vec(n_seq_dev, 'n_seq_dev', 1, dtype=torch.int32)
    check(lib.lime_additive_pool_count_f32(_p(hidden), _ld(hidden), _p(_vec(affine2, 'affine2', A)), A, _p(x), _ld(x), D, _p(m),
                                           _p(n_seq_dev), _p(out), _ld(out), n_seq, S, _stream()), 'lime_additive_pool_f32')
    return out


def fill_pad_rows(ids, src, dst, S):
    """dst[r] = src[r % S] for the rows r whose id is the padding word 0 (``lime_fill_pad_rows_f32``); returns dst."""
    lib = _lib.load()
    _vec(ids, 'ids', dtype=torch.int32)
    _mat(src, 'src')
    _mat(dst, 'dst')
    if dst.shape[0] != ids.numel() or src.shape[0] < S or src.shape[1] != dst.shape[1]:
        raise ValueError('fill_pad_rows: dst must be [len(ids), cols], src [>= S, cols]')
    check(lib.lime_fill_pad_rows_f32(_p(ids), _p(src), _ld(src), _p(dst), _ld(dst), ids.numel(), S, dst.shape[1], _stream()),
          'lime_fill_pad_rows_f32')
    return dst


def additive_pool_bwd(hidden, affine2, x, dout, n_seq, S, mask=None):
    """Backward of ``additive_pool``: -> (dhidden [n_seq * S, A], daffine2 [A], dx [n_seq * S, D])."""
    lib = _lib.load()
    _mat(hidden, 'hidden')
    _mat(x, 'x')
    _mat(dout, 'dout')
    A, D = hidden.shape[1], x.shape[1]
    if hidden.shape[0] != n_seq * S or x.shape[0] != n_seq * S or tuple(dout.shape) != (n_seq, D):
        raise ValueError('hidden and x must have n_seq * S rows, dout must be [n_seq, D]')
    dh = torch.empty((n_seq * S, A), dtype=torch.float32, device=x.device)
    dx = torch.empty((n_seq * S, D), dtype=torch.float32, device=x.device)
    part = torch.empty((max(n_seq, 1), A), dtype=torch.float32, device=x.device)
    m = _mask_u8(mask, 'mask')
    check(lib.lime_additive_pool_bwd_f32(_p(hidden), _ld(hidden), _p(_vec(affine2, 'affine2', A)), A, _p(x), _ld(x), D, _p(m), _p(dout),
                                         _ld(dout), _p(dh), _ld(dh), _p(dx), _ld(dx), _p(part), n_seq, S, _stream()), 'lime_additive_pool_bwd_f32')
    da2 = colsum(part[:n_seq]) if n_seq else torch.zeros(A, dtype=torch.float32, device=x.device)
    return dh, da2, dx


CAND_ATTN_BY_HEAD = True      # False: the one-workgroup-per-row kernel (tests compare the two)


def cand_attn_weights(qp, kp, mask, B, N, H, D, n_head, hist_div=1):
    """agg [B, H] of layers.py:66-81.  ``hist_div`` > 1: kp [B / hist_div, H, D] and mask [B / hist_div, H] hold one history for hist_div
    consecutive rows (the candidates of one impression)."""
    lib = _lib.load()
    if B % hist_div:
        raise ValueError('B must be a multiple of hist_div')
    Bh = B // hist_div
    _vec(qp, 'qp', B * N * D)
    _vec(kp, 'kp', Bh * H * D)
    m = _mask_u8(mask, 'mask')
    if m.numel() != Bh * H:
        raise ValueError('mask must be [B / hist_div, H]')
    agg = torch.empty((B, H), dtype=torch.float32, device=qp.device)
    by_head = (N + H) * (D // n_head + 1) * 4 <= 64 * 1024
    if hist_div > 1 and not (CAND_ATTN_BY_HEAD and by_head):
        kp, m, hist_div = kp.view(Bh, H * D).repeat_interleave(hist_div, dim=0).view(-1), m.view(Bh, H).repeat_interleave(hist_div, dim=0), 1
    if CAND_ATTN_BY_HEAD and by_head:
        # (row, head)-parallel: two short launches through a workspace (B = 32 rows alone leave 7 of 8 CUs idle)
        n_ws = int(lib.lime_cand_attn_weights_workspace(B, N, H, n_head))
        ws = torch.empty(max(n_ws, 1), dtype=torch.float32, device=qp.device)
        check(lib.lime_cand_attn_weights_shared_f32(_p(qp), _p(kp), _p(m), _p(agg), B, N, H, D, n_head, hist_div, _p(ws), n_ws, _stream()),
              'lime_cand_attn_weights_shared_f32')
        return agg
    check(lib.lime_cand_attn_weights_f32(_p(qp), _p(kp), _p(m), _p(agg), B, N, H, D, n_head, _stream()),
          'lime_cand_attn_weights_f32')
    return agg


def gate_ln_sage(y, x, scale, bias, gamma, beta, eps, groups, H, D, row_div, n_src, node_const=None):
    """``gate_ln`` over the H history rows of each of `groups` user rows + the GraphSAGE aggregate of the result in one launch:
    -> (refined [groups * H, D], mean [groups, D]).  x / y are [groups // row_div, H, D] (one history per row_div rows)."""
    lib = _lib.load()
    src_rows = (groups // row_div) * H * D
    x = _vec(x.contiguous(), 'x', src_rows)
    y = _vec(y.contiguous(), 'y', src_rows)
    scale = _vec(scale.contiguous(), 'scale', groups * H)
    out = torch.empty((groups * H, D), dtype=torch.float32, device=x.device)
    mean = torch.empty((groups, D), dtype=torch.float32, device=x.device)
    nc = _vec(node_const.contiguous(), 'node_const', D) if node_const is not None else None
    check(lib.lime_gate_ln_sage_f32(_p(y), _p(x), _p(scale), _p(_vec(bias, 'bias', D)), _p(_vec(gamma, 'gamma', D)), _p(_vec(beta, 'beta', D)),
                                    eps, _p(out), _p(nc) if nc is not None else None, _p(mean), groups, H, D, row_div, n_src, _stream()),
          'lime_gate_ln_sage_f32')
    return out, mean


def gate_ln(y, x, scale, bias, gamma, beta, eps=1e-5):
    """LayerNorm(g * (s x) + (1 - g) x), g = sigmoid(s y + bias): the gated residual of layers.py:84-89."""
    lib = _lib.load()
    D = x.shape[-1]
    x = _vec(x.contiguous(), 'x')
    y = _vec(y.contiguous(), 'y', x.numel())
    rows = x.numel() // D
    out = torch.empty_like(x)
    check(lib.lime_gate_ln_f32(_p(y), _p(x), _p(_vec(scale.contiguous(), 'scale', rows)), _p(_vec(bias, 'bias', D)),
                               _p(_vec(gamma, 'gamma', D)), _p(_vec(beta, 'beta', D)), eps, _p(out), rows, D, _stream()),
          'lime_gate_ln_f32')
    return out


def sage_mean(hist, user_nodes, B, H, n_src, D):
    lib = _lib.load()
    _vec(hist, 'hist', B * H * D)
    _vec(user_nodes, 'user_nodes')
    n_user = user_nodes.numel() // D
    out = torch.empty((B, D), dtype=torch.float32, device=hist.device)
    check(lib.lime_sage_mean_f32(_p(hist), _p(user_nodes), _p(out), B, H, n_user, n_src, D, _stream()), 'lime_sage_mean_f32')
    return out


def interest_match(kp, qp, g, cand, remaining, B, N, H, A, D, scale, alpha, beta, use_weight, use_penalty, want_logits=True,
                   want_user=True):
    lib = _lib.load()
    _vec(kp, 'kp', B * H * A)
    _vec(qp, 'qp', B * N * A)
    _vec(g, 'g', B * H * D)
    _vec(cand, 'cand', B * N * D)
    if want_logits and use_weight:
        remaining = _vec(remaining.contiguous(), 'remaining', B * N)
    user = torch.empty((B, N, D), dtype=torch.float32, device=kp.device) if want_user else None
    logits = torch.empty((B, N), dtype=torch.float32, device=kp.device) if want_logits else None
    check(lib.lime_interest_match_f32(_p(kp), _p(qp), _p(g), _p(cand), _p(remaining) if want_logits and use_weight else None,
                                      _p(user), _p(logits), B, N, H, A, D, scale, alpha, beta, int(use_weight),
                                      int(use_penalty), _stream()), 'lime_interest_match_f32')
    return user, logits


def lifetime_score(user, news, remaining, alpha, beta, use_weight, use_penalty):
    lib = _lib.load()
    D = user.shape[-1]
    user = _vec(user.contiguous(), 'user')
    news = _vec(news.contiguous(), 'news', user.numel())
    rows = user.numel() // D
    if use_weight:
        remaining = _vec(remaining.contiguous(), 'remaining', rows)
    logits = torch.empty(user.shape[:-1], dtype=torch.float32, device=user.device)
    check(lib.lime_lifetime_score_f32(_p(user), _p(news), _p(remaining) if use_weight else None, _p(logits), rows, D, alpha,
                                      beta, int(use_weight), int(use_penalty), _stream()), 'lime_lifetime_score_f32')
    return logits


# The tail of the pooled user encoders (userEncoders.ATT / MHSA): one launch (True) or lime_additive_pool_f32 + lime_lifetime_score_f32
# on an expanded copy of the user vector (False).  The default is the faster form at the eval shape (DESIGN.md "ATT and MHSA user
# encoders"); LIME_FUSED_POOL_MATCH=0 / 1 selects the other one.
FUSED_POOL_MATCH = os.environ.get('LIME_FUSED_POOL_MATCH', '1') == '1'


def pool_match(hidden, affine2, x, B, H, cand=None, remaining=None, alpha=0.0, beta=0.0, use_weight=False, use_penalty=False, mask=None,
               want_user=True, want_logits=True, fused=None):
    """``lime_pool_match_f32``: additive attention pool over the H history rows of each of B users (layers.py:288-299 from the tanh
    hidden state), and the lifetime-weighted dot product of the pooled vector with the user's N candidates (util.py:23-49).
    hidden [B H, A], x [B H, D] (row-strided views allowed), cand [B, N, D], remaining [B, N] -> (user [B, D] or None, logits [B, N] or
    None).  ``fused`` False: the same function on the two existing kernels (default: FUSED_POOL_MATCH)."""
    lib = _lib.load()
    _mat(hidden, 'hidden')
    _mat(x, 'x')
    A, D = hidden.shape[1], x.shape[1]
    if hidden.shape[0] != B * H or x.shape[0] != B * H:
        raise ValueError('hidden and x must have B * H rows')
    if not (want_user or want_logits):
        raise ValueError('pool_match: nothing to compute')
    N = 1
    if want_logits:
        if cand is None or cand.dim() != 3 or cand.shape[0] != B or cand.shape[2] != D:
            raise ValueError('cand must be [B, N, D]')
        N = cand.shape[1]
        cand = _vec(cand.contiguous(), 'cand', B * N * D)
        if use_weight:
            remaining = _vec(remaining.contiguous(), 'remaining', B * N)
    if not (FUSED_POOL_MATCH if fused is None else fused):
        user = additive_pool(hidden, affine2, x, B, H, mask=mask)
        logits = None
        if want_logits:
            logits = lifetime_score(user.unsqueeze(1).expand(B, N, D), cand, remaining, alpha, beta, use_weight, use_penalty)
        return (user if want_user else None), logits
    m = _mask_u8(mask, 'mask')
    if m is not None and m.numel() != B * H:
        raise ValueError('mask must have B * H elements')
    user = torch.empty((B, D), dtype=torch.float32, device=x.device) if want_user else None
    logits = torch.empty((B, N), dtype=torch.float32, device=x.device) if want_logits else None
    check(lib.lime_pool_match_f32(_p(hidden), _ld(hidden), _p(_vec(affine2, 'affine2', A)), _p(x), _ld(x), _p(m), _p(cand) if want_logits else None,
                                  _p(remaining) if want_logits and use_weight else None, alpha, beta, int(use_weight), int(use_penalty),
                                  _p(user), _p(logits), B, N, H, A, D, _stream()), 'lime_pool_match_f32')
    return user, logits


def _occurrence_tables(index, occ, tables, n_occ):
    """The host checks of the occurrence-composed forms: ``tables`` = ((tensor, name, columns), ...), the occurrence tables beside
    the news tables; occ int32 [P] like index -> (occ, n_occ: the first rows of each that occ may name, default all of the first's)."""
    if index is None or occ is None:
        raise ValueError('occ names rows of the occurrence tables next to index: give index, occ and the tables together')
    for t, name, cols in tables:
        if t is None:
            raise ValueError('the occurrence-composed form needs %s' % name)
        _mat(t, name)
        if not t.is_contiguous():
            raise ValueError('%s must be contiguous' % name)
    n_occ = tables[0][0].shape[0] if n_occ is None else int(n_occ)
    if any(t.shape[1] != cols for t, _, cols in tables) or not 0 <= n_occ <= min(t.shape[0] for t, _, _ in tables):
        raise ValueError('%s with n_occ = %d, got %s' % (' and '.join('%s must be [>= n_occ, %d]' % (name, cols) for _, name, cols in tables),
                                                         n_occ, ' and '.join(str(tuple(t.shape)) for t, _, _ in tables)))
    return _vec(occ, 'occ', index.numel(), dtype=torch.int32), n_occ


def _grouped_operands(kp, g, qp, v, names, H, index, n, occurrence, plain=True):
    """The host checks the grouped matches open with, under the caller's operand ``names``: kp [G H, A] and g [G H, W] per group; qp
    and v per pair -- [P, A] and [P, W] (the plain form, where the entry has one: ``plain``), or tables of at least ``n`` rows read
    through index int32 [P] (default: all of qp's) -> (G, P, A, W, index, n, composed: whether one of the ``occurrence`` arguments
    (occ, the two tables, n_occ) is given -- ``_occurrence_tables`` then checks them, behind the caller's own)."""
    for t, name in zip((kp, g, qp, v), names):
        _mat(t, name)
        if not t.is_contiguous():
            raise ValueError('%s must be contiguous' % name)
    (A, W), (k_, g_, q_, v_) = (kp.shape[1], g.shape[1]), names
    if H < 1 or kp.shape[0] % H or g.shape[0] != kp.shape[0]:
        raise ValueError('%s and %s must have G * H rows each, got %d and %d with H = %d' % (k_, g_, kp.shape[0], g.shape[0], H))
    if plain and index is None:
        if n is not None:
            raise ValueError('n is the table size of the indexed form: give index too')
        P = qp.shape[0]
        if qp.shape[1] != A or v.shape != (P, W):
            raise ValueError('%s must be [P, %d] and %s [P, %d], got %s and %s' % (q_, A, v_, W, tuple(qp.shape), tuple(v.shape)))
    else:
        P = index.numel()
        index = _vec(index, 'index', P, dtype=torch.int32)
        n = qp.shape[0] if n is None else int(n)
        if qp.shape[1] != A or v.shape[1] != W or not 0 <= n <= min(qp.shape[0], v.shape[0]):
            raise ValueError('%s must be [>= n, %d] and %s [>= n, %d] with n = %d, got %s and %s'
                             % (q_, A, v_, W, n, tuple(qp.shape), tuple(v.shape)))
    return kp.shape[0] // H, P, A, W, index, n, any(t is not None for t in occurrence)


def grouped_match(kp, g, qp, cand, remaining, offsets, H, scale, alpha=0.0, beta=0.0, use_weight=False, use_penalty=False, index=None,
                  n=None, occ=None, qt=None, ct=None, n_occ=None):
    """``lime_grouped_match_f32``: the history-vs-candidate attention, the dot-product match and the remaining-lifetime weight for
    groups of pairs that share one refined history.  kp [G H, A], g [G H, D] per group; qp [P, A], cand [P, D], remaining [P] per
    pair; offsets int64 [G + 1] (device): the pairs of group i are rows offsets[i] .. offsets[i + 1] - 1 -> logits [P] (pairs outside
    every group keep what ``torch.empty`` gave them).  1 <= H <= 128; A, D multiples of 4 up to 2048.

    ``index`` int32 [P] (``lime_grouped_match_indexed_f32``): qp and cand are tables and pair p reads row index[p] of both -- the first
    ``n`` rows of each (default: all of qp's; cand has at least as many); the kernel clamps an index outside [0, n) into it.  A pair's
    bits are those of the plain form on ``qp[index]``, ``cand[index]``.

    ``occ`` int32 [P] with ``qt`` [n_occ, A] and ``ct`` [n_occ, D] next to ``index`` (``lime_grouped_match_occurrence_f32``): the
    pair's operands are composed in the kernel, ``qp[index] + qt[occ]`` and ``cand[index] + ct[occ]`` (one fp32 add per element; occ
    is clamped into [0, n_occ), default all of qt's rows).  A pair's bits are those of the plain form on those sums."""
    lib = _lib.load()
    G, P, A, D, index, n, composed = _grouped_operands(kp, g, qp, cand, ('kp', 'g', 'qp', 'cand'), H, index, n, (occ, qt, ct, n_occ))
    if composed:
        occ, n_occ = _occurrence_tables(index, occ, ((qt, 'qt', A), (ct, 'ct', D)), n_occ)
    _vec(offsets, 'offsets', G + 1, dtype=torch.int64)
    if use_weight:
        remaining = _vec(remaining.contiguous(), 'remaining', P)
    logits = torch.empty((P,), dtype=torch.float32, device=qp.device)
    if index is None:
        check(lib.lime_grouped_match_f32(_p(kp), _p(g), _p(qp), _p(cand), _p(remaining) if use_weight else None, _p(offsets), _p(logits),
                                         G, P, H, A, D, scale, alpha, beta, int(use_weight), int(use_penalty), _stream()),
              'lime_grouped_match_f32')
    elif composed:
        check(lib.lime_grouped_match_occurrence_f32(_p(kp), _p(g), _p(qp), _p(cand), _p(qt), _p(ct), _p(remaining) if use_weight else None,
                                                    _p(offsets), _p(index), n, _p(occ), n_occ, _p(logits), G, P, H, A, D, scale, alpha, beta,
                                                    int(use_weight), int(use_penalty), _stream()), 'lime_grouped_match_occurrence_f32')
    else:
        check(lib.lime_grouped_match_indexed_f32(_p(kp), _p(g), _p(qp), _p(cand), _p(remaining) if use_weight else None, _p(offsets),
                                                 _p(index), n, _p(logits), G, P, H, A, D, scale, alpha, beta, int(use_weight),
                                                 int(use_penalty), _stream()), 'lime_grouped_match_indexed_f32')
    return logits


PairTerms = collections.namedtuple('PairTerms', 'logits base weight attn contrib top_slot top_value')
EXPLAIN_BY = {'contribution': _lib.CONSTANTS['LIME_EXPLAIN_BY_CONTRIBUTION'], 'attention': _lib.CONSTANTS['LIME_EXPLAIN_BY_ATTENTION']}


def grouped_match_explain(kp, g, qp, cand, remaining, offsets, H, scale, alpha=0.0, beta=0.0, use_weight=False, use_penalty=False,
                          mask=None, hist_div=1, m=3, by='contribution', dense=True, index=None, n=None, occ=None, qt=None, ct=None,
                          n_occ=None):
    """``lime_grouped_match_explain_f32``: ``grouped_match`` with its terms kept -> PairTerms(logits [P] -- the bits of
    ``grouped_match`` on the same operands, in each of its three forms --, base [P], weight [P], attn [P, H], contrib [P, H],
    top_slot int32 [P, m], top_value [P, m]).  attn = softmax_h(s), contrib[p, h] = attn[p, h] (g[i, h] . cand[p]) weight[p], so a
    row of contrib sums to its logit; ``dense`` off: attn and contrib are not written (None).  top_slot / top_value: the m slots of
    largest contrib (``by`` 'contribution') or attn ('attention') among those whose byte of ``mask`` (bool / uint8
    [ceil(G / hist_div), H]; group i reads row i // hist_div; None: every slot) is set, larger first, equal values lower slot first,
    -1 / 0.0 behind the last eligible one (``recommend.explain_pairs`` states all of it on the host).  1 <= m <= min(16, H).
    Pairs outside every group keep what ``torch.empty`` gave them."""
    lib = _lib.load()
    if by not in EXPLAIN_BY:
        raise ValueError("by must be 'contribution' or 'attention', got %r" % (by,))
    G, P, A, D, index, n, composed = _grouped_operands(kp, g, qp, cand, ('kp', 'g', 'qp', 'cand'), H, index, n, (occ, qt, ct, n_occ))
    if composed:
        occ, n_occ = _occurrence_tables(index, occ, ((qt, 'qt', A), (ct, 'ct', D)), n_occ)
    _vec(offsets, 'offsets', G + 1, dtype=torch.int64)
    if use_weight:
        remaining = _vec(remaining.contiguous(), 'remaining', P)
    hist_div, m = int(hist_div), int(m)
    if hist_div < 1:
        raise ValueError('hist_div must be >= 1, got %d' % hist_div)
    mk = _mask_u8(mask, 'mask')
    if mk is not None and mk.numel() != (G + hist_div - 1) // hist_div * H:
        raise ValueError('mask must be [ceil(G / hist_div), H] = [%d, %d], got %s' % ((G + hist_div - 1) // hist_div, H, tuple(mask.shape)))
    new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=kp.device)
    out = PairTerms(new((P,)), new((P,)), new((P,)), new((P, H)) if dense else None, new((P, H)) if dense else None,
                    new((P, max(m, 0)), torch.int32), new((P, max(m, 0))))
    check(lib.lime_grouped_match_explain_f32(_p(kp), _p(g), _p(qp), _p(cand), _p(qt) if composed else None, _p(ct) if composed else None,
                                             _p(remaining) if use_weight else None, _p(offsets), _p(index), n if index is not None else 0,
                                             _p(occ) if composed else None, n_occ if composed else 0, _p(mk), hist_div, m, EXPLAIN_BY[by],
                                             _p(out.logits), _p(out.base), _p(out.weight), _p(out.attn), _p(out.contrib), _p(out.top_slot),
                                             _p(out.top_value), G, P, H, A, D, scale, alpha, beta, int(use_weight), int(use_penalty),
                                             _stream()), 'lime_grouped_match_explain_f32')
    return out


def grouped_match_schedule_fits(H, n_occ):
    """Whether ``lime_grouped_match_schedule_f32`` takes a history of H rows with n_occ occurrence rows: 1 <= H <= 128 and its LDS
    bound, 2048 T + 8 n_occ Hs <= 65536 bytes (T = 1, 2, 4, 8 for H <= 16, 32, 64, 128; Hs = H rounded up to 4).  Pure host arithmetic."""
    if not 1 <= H <= 128 or n_occ < 0:
        return False
    T = 1 if H <= 16 else 2 if H <= 32 else 4 if H <= 64 else 8
    return 2048 * T + 8 * n_occ * ((H + 3) // 4 * 4) <= 65536


def grouped_match_schedule(kp, g, qa, ca, remaining, offsets, index, H, scale, alpha=0.0, beta=0.0, use_weight=False, use_penalty=False,
                           n=None, occ=None, qt=None, ct=None, n_occ=None, slots=None):
    """``lime_grouped_match_schedule_f32``: ``grouped_match``'s occurrence form for S time slots of every pair in one launch.  kp
    [G H, A], g [G H, D] per group; the news tables qa [n, A] and ca [n, D] read through ``index`` int32 [P]; ``remaining`` fp32 [S, P]
    (read under ``use_weight``); offsets int64 [G + 1] (device) -> logits fp32 [S, P].

    ``occ`` int32 [S, P] with ``qt`` [n_occ, A] and ``ct`` [n_occ, D]: slot s of pair p is the match of ``qa[index] + qt[occ[s]]`` and
    ``ca[index] + ct[occ[s]]`` in the factorised form -- the news-table products once per pair, the occurrence terms from per-group
    tables the kernel forms in LDS (2048 T + 8 n_occ Hs bytes <= 65536: ``LimeHipError`` beyond).  Without them (a baseline model) only
    the weight moves with the slot and a slot's bits are those of ``grouped_match``'s indexed form.  ``slots``: S, where neither
    ``occ`` nor ``remaining`` gives it."""
    lib = _lib.load()
    G, P, A, D, index, n, composed = _grouped_operands(kp, g, qa, ca, ('kp', 'g', 'qa', 'ca'), H, index, n, (occ, qt, ct, n_occ),
                                                       plain=False)
    given = [t.shape[0] for t in (occ, remaining if use_weight else None) if t is not None] + ([int(slots)] if slots is not None else [])
    if not given or min(given) != max(given) or given[0] < 1:
        raise ValueError('the slot count S >= 1 comes from occ [S, P], remaining [S, P] or slots, and they must agree: got %s' % (given,))
    S = given[0]
    if composed:
        if occ is None or tuple(occ.shape) != (S, P):
            raise ValueError('occ must be [S, P] = [%d, %d], got %s' % (S, P, None if occ is None else tuple(occ.shape)))
        occ = occ.contiguous()
        _, n_occ = _occurrence_tables(index, occ[0], ((qt, 'qt', A), (ct, 'ct', D)), n_occ)        # the tables' checks, on one slot
        occ = _vec(occ.view(-1), 'occ', S * P, dtype=torch.int32)
    _vec(offsets, 'offsets', G + 1, dtype=torch.int64)
    if use_weight:
        if tuple(remaining.shape) != (S, P):
            raise ValueError('remaining must be [S, P] = [%d, %d], got %s' % (S, P, tuple(remaining.shape)))
        remaining = _vec(remaining.contiguous().view(-1), 'remaining', S * P)
    logits = torch.empty((S, P), dtype=torch.float32, device=qa.device)
    check(lib.lime_grouped_match_schedule_f32(_p(kp), _p(g), _p(qa), _p(ca), _p(qt) if composed else None, _p(ct) if composed else None,
                                              _p(remaining) if use_weight else None, _p(offsets), _p(index), n,
                                              _p(occ) if composed else None, n_occ if composed else 0, _p(logits), G, P, S, H, A, D, scale,
                                              alpha, beta, int(use_weight), int(use_penalty), _stream()), 'lime_grouped_match_schedule_f32')
    return logits


# The MLP click predictor's match (config.click_predictor = 'mlp'): one launch per pass that keeps the pooled hidden row of a pair in
# registers (True, lime_grouped_mlp_match_f32), or the composed form on existing launches -- the pairs' user rows, then
# ``linear(cat[user, news], mlp, act='relu')``, then the product with ``out`` -- which writes a [pairs, D] user row and a [pairs, D // 2]
# hidden row per pair (False).  The composed form is the fallback and the yardstick of the fused one's error
# (tests/test_grouped_mlp_match_gpu.py, tools/bench_mlp_match.py).  LIME_FUSED_MLP_MATCH=0 selects it.
FUSED_MLP_MATCH = os.environ.get('LIME_FUSED_MLP_MATCH', '1') != '0'


def grouped_mlp_match(kp, gu, qp, nw, w_out, b_out, offsets, H, scale, index=None, n=None, occ=None, qt=None, nt=None, n_occ=None):
    """``lime_grouped_mlp_match_f32``: the history-vs-candidate attention and the MLP click predictor for groups of pairs that share one
    refined history.  kp [G H, A] and gu = g W_u^T [G H, Dh] per group; qp [P, A] and nw = cand W_n^T + mlp.bias [P, Dh] per pair; w_out
    [Dh] (out.weight), b_out [1] (out.bias; None: 0); offsets int64 [G + 1] (device) -> logits [P] (pairs outside every group keep what
    ``torch.empty`` gave them).  1 <= H <= 128; A a multiple of 4, Dh even, both up to 2048.

    ``index`` int32 [P] (``lime_grouped_mlp_match_indexed_f32``): qp and nw are tables and pair p reads row index[p] of both -- the
    first ``n`` rows of each (default: all of qp's); the kernel clamps an index outside [0, n) into it.  A pair's bits are those of the
    plain form on ``qp[index]``, ``nw[index]``.

    ``occ`` int32 [P] with ``qt`` [n_occ, A] and ``nt`` [n_occ, Dh] next to ``index`` (``lime_grouped_mlp_match_occurrence_f32``): the
    pair's operands are composed in the kernel, ``qp[index] + qt[occ]`` and ``nw[index] + nt[occ]`` -- the rules of
    ``grouped_match``'s occurrence form."""
    lib = _lib.load()
    G, P, A, Dh, index, n, composed = _grouped_operands(kp, gu, qp, nw, ('kp', 'gu', 'qp', 'nw'), H, index, n, (occ, qt, nt, n_occ))
    if composed:
        occ, n_occ = _occurrence_tables(index, occ, ((qt, 'qt', A), (nt, 'nt', Dh)), n_occ)
    _vec(offsets, 'offsets', G + 1, dtype=torch.int64)
    w_out = _vec(w_out.reshape(-1), 'w_out', Dh)
    if b_out is not None:
        b_out = _vec(b_out.reshape(-1), 'b_out', 1)
    logits = torch.empty((P,), dtype=torch.float32, device=qp.device)
    if index is None:
        check(lib.lime_grouped_mlp_match_f32(_p(kp), _p(gu), _p(qp), _p(nw), _p(w_out), _p(b_out), _p(offsets), _p(logits), G, P, H, A, Dh,
                                             scale, _stream()), 'lime_grouped_mlp_match_f32')
    elif composed:
        check(lib.lime_grouped_mlp_match_occurrence_f32(_p(kp), _p(gu), _p(qp), _p(nw), _p(qt), _p(nt), _p(w_out), _p(b_out), _p(offsets),
                                                        _p(index), n, _p(occ), n_occ, _p(logits), G, P, H, A, Dh, scale, _stream()),
              'lime_grouped_mlp_match_occurrence_f32')
    else:
        check(lib.lime_grouped_mlp_match_indexed_f32(_p(kp), _p(gu), _p(qp), _p(nw), _p(w_out), _p(b_out), _p(offsets), _p(index), n,
                                                     _p(logits), G, P, H, A, Dh, scale, _stream()), 'lime_grouped_mlp_match_indexed_f32')
    return logits


def mlp_predictor(user, news, mlp_w, mlp_b, out_w, out_b):
    """The MLP click predictor on materialised rows, the composed form (reference model.py:182-184 in eval mode):
    ``out(relu(mlp(cat[user, news])))`` for user [P, D], news [P, D] -> logits [P], on lime_linear_f32."""
    hidden = linear(torch.cat([user, news], dim=1), mlp_w, mlp_b, act='relu')
    return linear(hidden, out_w.reshape(1, -1), out_b).view(-1)


def topk_rows(scores, k):
    """``lime_topk_rows_f32``: per row of scores [U, C] (a row-strided view is fine) the k best -> (positions int32 [U, k], scores fp32
    [U, k]) in descending order; equal scores (+0.0 == -0.0) lower position first, NaN behind every number; slots behind the C-th hold
    -1 / -inf.  1 <= k <= 128."""
    lib = _lib.load()
    _mat(scores, 'scores')
    U, C = scores.shape
    k = int(k)
    if k < 1 or C < 1:
        raise ValueError('topk_rows needs k >= 1 and at least one column, got k = %d, C = %d' % (k, C))
    positions = torch.empty((U, k), dtype=torch.int32, device=scores.device)
    top = torch.empty((U, k), dtype=torch.float32, device=scores.device)
    need = int(lib.lime_topk_rows_workspace(U, C))
    ws = _workspace(scores.device, need) if need else None
    check(lib.lime_topk_rows_f32(_p(scores), _ld(scores), U, C, k, _p(positions), _p(top), _p(ws), need, _stream()), 'lime_topk_rows_f32')
    return positions, top


def list_plan(keys, offsets, slots=None, n_keys=8192, n_distinct=None):
    """``lime_list_plan_count`` + ``lime_list_plan``: ``recommend.list_plan`` on the device, bit for bit.  keys int32 [P] (device,
    0 <= key < ``n_keys`` <= 8192), offsets int64 [U + 1] (device) -> recommend.ListPlan(order int64 [P], group_offsets int64
    [U S + 1], slot_key int32 [U S] -- device tensors -- and n_distinct int32 [U], a host array).

    The count runs first and ``n_distinct`` is read back ONCE, to pick S = max(1, n_distinct.max()) (or to check ``slots``: a smaller
    one is a ValueError): that small device -> host copy is the only synchronisation of the candidate-list path.  A caller that
    already holds the counts of these very lists passes them as ``n_distinct`` (host) and adds none."""
    import numpy as np
    from .recommend import ListPlan
    lib = _lib.load()
    _vec(keys, 'keys', dtype=torch.int32)
    P = keys.numel()
    _vec(offsets, 'offsets', dtype=torch.int64)
    U = offsets.numel() - 1
    if U < 0:
        raise ValueError('offsets must hold U + 1 >= 1 entries')
    dev = keys.device
    if n_distinct is None:
        nd_dev = torch.empty((U,), dtype=torch.int32, device=dev)
        check(lib.lime_list_plan_count(_p(keys), _p(offsets), U, P, int(n_keys), _p(nd_dev), _stream()), 'lime_list_plan_count')
        n_distinct = nd_dev.cpu().numpy()
    else:
        n_distinct = np.asarray(n_distinct, dtype=np.int32).reshape(-1)
        if n_distinct.shape[0] != U:
            raise ValueError('n_distinct must have U = %d entries, got %d' % (U, n_distinct.shape[0]))
    need = max(1, int(n_distinct.max())) if U else 1
    S = need if slots is None else int(slots)
    if S < need:
        raise ValueError('slots = %d, but a list holds %d distinct keys' % (S, need))
    order = torch.empty((P,), dtype=torch.int64, device=dev)
    group_offsets = torch.empty((U * S + 1,), dtype=torch.int64, device=dev)
    slot_key = torch.empty((U * S,), dtype=torch.int32, device=dev)
    check(lib.lime_list_plan(_p(keys), _p(offsets), U, P, int(n_keys), S, _p(order), _p(group_offsets), _p(slot_key), _stream()),
          'lime_list_plan')
    return ListPlan(order, group_offsets, slot_key, n_distinct)


def topk_segments(scores, offsets, k):
    """``lime_topk_segments_f32``: the k best of every segment of scores fp32 [P]; offsets int64 [U + 1] (device): segment u is
    scores[offsets[u]:offsets[u + 1]] -> (positions int32 [U, k] WITHIN the segment, scores fp32 [U, k]) in ``topk_rows``' order;
    slots behind a segment's length (all of an empty segment's) hold -1 / -inf.  1 <= k <= 128."""
    lib = _lib.load()
    _vec(scores, 'scores')
    _vec(offsets, 'offsets', dtype=torch.int64)
    U, P, k = offsets.numel() - 1, scores.numel(), int(k)
    if U < 0 or not 1 <= k <= 128:
        raise ValueError('topk_segments needs 1 <= k <= 128 and U + 1 >= 1 offsets, got k = %d, %d offsets' % (k, U + 1))
    positions = torch.empty((U, k), dtype=torch.int32, device=scores.device)
    top = torch.empty((U, k), dtype=torch.float32, device=scores.device)
    need = int(lib.lime_topk_segments_workspace(U, P))
    ws = _workspace(scores.device, need) if need else None
    check(lib.lime_topk_segments_f32(_p(scores), _p(offsets), U, P, k, _p(positions), _p(top), _p(ws), ws.numel() if need else 0, _stream()),
          'lime_topk_segments_f32')
    return positions, top


def topk_rows_quota(scores, keys, quota, k, drop=None, n_keys=8192):
    """``lime_topk_rows_quota_f32``: ``topk_rows`` with at most ``quota`` entries of one group per row (``recommend.quota_topk`` on
    the device, bit for bit).  keys int32 [C] (device): column j belongs to group keys[j], 0 <= key < ``n_keys`` <= 8192 (a key
    outside drops the column); drop: None or bool / uint8 [R, C] (device, contiguous), row u masked by drop[u % R]: a set entry takes
    no part -> (positions int32 [U, k], scores fp32 [U, k]) in walk order, -1 / -inf behind the last taken entry.  1 <= k <= 128."""
    lib = _lib.load()
    _mat(scores, 'scores')
    U, C = scores.shape
    k, quota = int(k), int(quota)
    if k < 1 or C < 1 or quota < 1:
        raise ValueError('topk_rows_quota needs k >= 1, quota >= 1 and at least one column, got k = %d, quota = %d, C = %d' % (k, quota, C))
    _vec(keys, 'keys', C, dtype=torch.int32)
    rows = 0
    if drop is not None:
        if drop.dim() != 2 or drop.shape[1] != C or drop.shape[0] < 1:
            raise ValueError('drop must be [R, C] = [R, %d] with R >= 1, got %s' % (C, tuple(drop.shape)))
        rows = drop.shape[0]
        drop = _mask_u8(drop.reshape(-1), 'drop')
    positions = torch.empty((U, k), dtype=torch.int32, device=scores.device)
    top = torch.empty((U, k), dtype=torch.float32, device=scores.device)
    need = int(lib.lime_topk_rows_quota_workspace(U, C))
    ws = _workspace(scores.device, need) if need else None
    check(lib.lime_topk_rows_quota_f32(_p(scores), _ld(scores), U, C, _p(keys), int(n_keys), quota, _p(drop), rows, k, _p(positions), _p(top),
                                       _p(ws), need, _stream()), 'lime_topk_rows_quota_f32')
    return positions, top


def topk_segments_quota(scores, offsets, keys, quota, k, drop=None, n_keys=8192):
    """``lime_topk_segments_quota_f32``: ``topk_segments`` with at most ``quota`` entries of one group per segment
    (``recommend.quota_topk_segments`` on the device, bit for bit).  keys int32 [P] and drop (None or bool / uint8 [P]) lie beside
    scores [P] -> (positions int32 [U, k] WITHIN the segment, scores fp32 [U, k]).  1 <= k <= 128."""
    lib = _lib.load()
    _vec(scores, 'scores')
    _vec(offsets, 'offsets', dtype=torch.int64)
    U, P, k, quota = offsets.numel() - 1, scores.numel(), int(k), int(quota)
    if U < 0 or not 1 <= k <= 128 or quota < 1:
        raise ValueError('topk_segments_quota needs 1 <= k <= 128, quota >= 1 and U + 1 >= 1 offsets, got k = %d, quota = %d, %d offsets'
                         % (k, quota, U + 1))
    _vec(keys, 'keys', P, dtype=torch.int32)
    if drop is not None:
        drop = _vec(_mask_u8(drop, 'drop'), 'drop', P, dtype=torch.uint8)
    positions = torch.empty((U, k), dtype=torch.int32, device=scores.device)
    top = torch.empty((U, k), dtype=torch.float32, device=scores.device)
    need = int(lib.lime_topk_segments_quota_workspace(U, P))
    ws = _workspace(scores.device, need) if need else None
    check(lib.lime_topk_segments_quota_f32(_p(scores), _p(offsets), U, P, _p(keys), int(n_keys), quota, _p(drop), k, _p(positions), _p(top),
                                           _p(ws), ws.numel() if need else 0, _stream()), 'lime_topk_segments_quota_f32')
    return positions, top


def mmr_rows(scores, ids, table, lam, k):
    """``lime_mmr_rows_f32``: maximal marginal relevance over a shortlist per row (``recommend.mmr_select`` on the device).  scores
    fp32 [R, M] and ids int32 [R, M] (device, contiguous): a row's shortlist, best first, and the row of ``table`` fp32 [n, E] (a
    row-strided view is fine) behind each entry; an entry whose id is outside [0, n) or whose score is not finite is dead -> picks
    int32 [R, k], the shortlist ranks in the order taken, -1 behind the last.  1 <= k <= M <= 128, E a multiple of 4, 0 <= lam <= 1."""
    lib = _lib.load()
    _mat(scores, 'scores')
    _mat(table, 'table')
    R, M = scores.shape
    n, E = table.shape
    k, lam = int(k), float(lam)
    if not 1 <= k <= M or n < 1 or E < 1 or not 0.0 <= lam <= 1.0:
        raise ValueError('mmr_rows needs 1 <= k <= M, a table of at least one row and column and 0 <= lam <= 1, got k = %d, M = %d, '
                         'table %s, lam = %r' % (k, M, (n, E), lam))
    if not scores.is_contiguous():
        raise ValueError('scores must be contiguous, got strides %s' % (scores.stride(),))
    _vec(ids, 'ids', R * M, dtype=torch.int32)
    picks = torch.empty((R, k), dtype=torch.int32, device=scores.device)
    if R == 0:                                                    # (an empty tensor has no address to hand over)
        return picks
    check(lib.lime_mmr_rows_f32(_p(scores), _p(ids), R, M, _p(table), _ld(table), n, E, lam, k, _p(picks), _stream()), 'lime_mmr_rows_f32')
    return picks


def _history(hist_keys, hist_weight, device, who):
    """The checks of a calibration target's operands -> (hist_rows, H): hist_keys int32 [hist_rows, H] and hist_weight fp32 like it or
    None, contiguous, on ``device``; H <= 128; at least one row where H > 0."""
    _mat(hist_keys, 'hist_keys', dtype=torch.int32)
    rows, H = hist_keys.shape
    if not hist_keys.is_contiguous() or (H > 0 and rows < 1) or H > 128:
        raise ValueError('%s needs contiguous hist_keys [hist_rows, H] with H <= 128 and hist_rows >= 1 where H > 0, got %s strides %s'
                         % (who, tuple(hist_keys.shape), hist_keys.stride()))
    if hist_weight is not None:
        _mat(hist_weight, 'hist_weight')
        if hist_weight.shape != hist_keys.shape or not hist_weight.is_contiguous():
            raise ValueError('hist_weight must be contiguous and shaped like hist_keys %s, got %s' % (tuple(hist_keys.shape),
                                                                                                      tuple(hist_weight.shape)))
    for t, name in ((hist_keys, 'hist_keys'), (hist_weight, 'hist_weight')):
        if t is not None and t.device != device:
            raise ValueError('%s is on %s, the rows on %s' % (name, t.device, device))
    return rows, H


def calibrate_rows(scores, ids, keys, n_keys, hist_keys, hist_weight, lam, alpha, k):
    """``lime_calibrate_rows_f32``: calibrated greedy selection over a shortlist per row (``recommend.calibrated_select`` on the
    device).  scores fp32 [R, M] and ids int32 [R, M] (device, contiguous): a row's shortlist, best first, and the news id behind each
    entry (outside [0, n), or a score that is not finite: dead); keys int32 [n]: the group of every news, 0 <= key < ``n_keys`` <=
    8192; hist_keys int32 [hist_rows, H] (contiguous, H <= 128) and hist_weight fp32 like it or None: row r's target is history row
    r % hist_rows -> picks int32 [R, k], the shortlist ranks in the order taken, -1 behind the last.  1 <= k <= M <= 128,
    0 <= lam <= 1, 0 < alpha < 1."""
    _mat(scores, 'scores')
    R, M = scores.shape
    k, lam, alpha, n_keys = int(k), float(lam), float(alpha), int(n_keys)
    if not 1 <= k <= M or M > 128 or not 0.0 <= lam <= 1.0 or not 0.0 < alpha < 1.0 or not 1 <= n_keys <= 8192:
        raise ValueError('calibrate_rows needs 1 <= k <= M <= 128, 0 <= lam <= 1, 0 < alpha < 1 and 1 <= n_keys <= 8192, got k = %d, M = %d, '
                         'lam = %r, alpha = %r, n_keys = %d' % (k, M, lam, alpha, n_keys))
    if not scores.is_contiguous():
        raise ValueError('scores must be contiguous, got strides %s' % (scores.stride(),))
    _vec(ids, 'ids', R * M, dtype=torch.int32)
    n = _vec(keys, 'keys', dtype=torch.int32).numel()
    if n < 1:
        raise ValueError('keys must hold the group of at least one news')
    rows, H = _history(hist_keys, hist_weight, scores.device, 'calibrate_rows')
    for t, name in ((ids, 'ids'), (keys, 'keys')):
        if t.device != scores.device:
            raise ValueError('%s is on %s, scores on %s' % (name, t.device, scores.device))
    picks = torch.empty((R, k), dtype=torch.int32, device=scores.device)
    if R == 0:                                                    # (an empty tensor has no address to hand over)
        return picks
    lib = _lib.load()                                             # (H = 0: an empty tensor has no address; nothing is read through it)
    check(lib.lime_calibrate_rows_f32(_p(scores), _p(ids), R, M, _p(keys), n, n_keys, ctypes.c_void_p(hist_keys.data_ptr() or 16),
                                      _p(hist_weight) if H else None, rows, H, lam, alpha, k, _p(picks), _stream()), 'lime_calibrate_rows_f32')
    return picks


def row_scale(x, scale):
    lib = _lib.load()
    D = x.shape[-1]
    x = _vec(x.contiguous(), 'x')
    rows = x.numel() // D
    scale = _vec(scale.contiguous(), 'scale', rows)
    out = torch.empty_like(x)
    check(lib.lime_row_scale_f32(_p(x), _p(scale), _p(out), rows, D, _stream()), 'lime_row_scale_f32')
    return out


def inv_sqrt(x):
    return 1.0 / math.sqrt(float(x))


def multi_copy(pairs):
    """dst.copy_(src) for every (dst, src) pair in ONE launch per 32 pairs (same dtype / shape, both contiguous CUDA)."""
    lib = _lib.load()
    todo = []
    for dst, src in pairs:
        if dst.shape != src.shape or dst.dtype != src.dtype or not dst.is_cuda or not src.is_cuda:
            raise ValueError('multi_copy: shape / dtype / device mismatch (%s %s vs %s %s)' % (tuple(dst.shape), dst.dtype,
                                                                                              tuple(src.shape), src.dtype))
        if not dst.is_contiguous():
            raise ValueError('multi_copy: destinations must be contiguous')
        if not src.is_contiguous():
            src = src.contiguous()
        if dst.data_ptr() != src.data_ptr() and dst.numel():
            todo.append((dst, src))
    for i in range(0, len(todo), _lib.MAX_COPIES):
        part = todo[i:i + _lib.MAX_COPIES]
        table = (_lib.CopyDesc * len(part))()
        for d, (dst, src) in zip(table, part):
            d.src, d.dst, d.bytes = src.data_ptr(), dst.data_ptr(), dst.numel() * dst.element_size()
        check(lib.lime_multi_copy(table, len(part), _stream()), 'lime_multi_copy')
    return todo            # keeps the sources referenced until the caller drops the list (the copy is asynchronous)


# ---- bf16 matrix-core path (BASELINE config 3) ---------------------------------------------------------------------------
def to_bf16(src, rows_out=None, cols_out=None, out=None):
    """fp32 [rows, cols] (or a vector) -> bf16 [rows_out, cols_out], zero padded; cols_out a multiple of 4."""
    lib = _lib.load()
    vec = src.dim() == 1
    s2 = src.view(-1, 1) if vec else src
    _mat(s2, 'src')
    rows, cols = s2.shape
    if vec:                                       # a vector is padded along its only axis
        s2 = src.view(1, -1)
        rows, cols = 1, src.numel()
        rows_out = 1
    rows_out = rows if rows_out is None else rows_out
    cols_out = (cols + 7) // 8 * 8 if cols_out is None else cols_out
    if out is None:
        out = torch.empty((rows_out, cols_out), dtype=torch.bfloat16, device=src.device)
    _mat(out, 'out', dtype=torch.bfloat16)
    check(lib.lime_to_bf16(_p(s2), _ld(s2), rows, cols, _p(out), _ld(out), rows_out, cols_out, _stream()), 'lime_to_bf16')
    return out.view(-1) if vec else out


def linear_bf16(a, w, bias=None, act=None, out=None, a_ids=None, res=None, res_kind=0, res_mod=0, res_ids=None, res_pe=None,
                res_period=0, ln=None, ln_eps=1e-5, ln_count=None, pool32=False, n_alg=None, k_alg=None, m_dev=None, c_ids=None):
    """``lime_linear_bf16``: a / w / out (and residual kinds 2, 3) bfloat16, bias / LayerNorm / residual kind 1 fp32."""
    lib = _lib.load()
    _mat(a, 'a', dtype=torch.bfloat16)
    _mat(w, 'w', dtype=torch.bfloat16)
    N, K = w.shape
    if a.shape[1] != K:
        raise ValueError('a has %d columns, w has K=%d' % (a.shape[1], K))
    M = a_ids.numel() if a_ids is not None else a.shape[0]
    if pool32 and M % 32:
        raise ValueError('pool32 needs M %% 32 == 0 (M = %d)' % M)
    rows_out, odt = (M // 32, torch.float32) if pool32 else (M, torch.bfloat16)       # pool32: fp32 means over 32-row blocks
    if out is None:
        out = torch.empty((rows_out, N), dtype=odt, device=a.device)
    _mat(out, 'out', dtype=odt)
    if c_ids is not None:
        if out.shape[1] != N:
            raise ValueError('out must have N columns')
    elif tuple(out.shape) != (rows_out, N):
        raise ValueError('out must be [%d, %d], got %s' % (rows_out, N, tuple(out.shape)))
    args = _lib.LinearBf16Args()
    if c_ids is not None:
        args.c_ids = _vec(c_ids, 'c_ids', M, dtype=torch.int32).data_ptr()
    if m_dev is not None:
        args.m_dev = _vec(m_dev, 'm_dev', 1, dtype=torch.int32).data_ptr()
    args.pool32 = 1 if pool32 else 0
    args.a, args.lda = a.data_ptr(), _ld(a)
    args.a_ids = _vec(a_ids, 'a_ids', dtype=torch.int32).data_ptr() if a_ids is not None else None
    args.w, args.ldw = w.data_ptr(), _ld(w)
    args.bias = _vec(bias, 'bias', N).data_ptr() if bias is not None else None
    if res is not None:
        if res_kind not in (1, 2, 3):
            raise ValueError('res_kind must be 1 (fp32 rows), 2 (gathered bf16 rows) or 3 (bf16 rows)')
        _mat(res, 'res', dtype=torch.float32 if res_kind == 1 else torch.bfloat16)
        if res.shape[1] != N:
            raise ValueError('res must have N=%d columns' % N)
        args.res, args.ldr, args.res_kind, args.res_mod = res.data_ptr(), _ld(res), res_kind, res_mod
        if res_kind == 1 and res.shape[0] < (res_mod if res_mod > 0 else M):
            raise ValueError('res has too few rows')
        if res_kind == 3 and res.shape[0] < M:
            raise ValueError('res has too few rows')
        if res_kind == 2:
            args.res_ids = _vec(res_ids, 'res_ids', M, dtype=torch.int32).data_ptr()
            if res_pe is not None:
                _mat(res_pe, 'res_pe')
                if res_pe.shape[1] != N or res_pe.shape[0] < res_period or res_period <= 0:
                    raise ValueError('res_pe must be [>=res_period, N]')
                args.res_pe, args.ldr_pe, args.res_period = res_pe.data_ptr(), _ld(res_pe), res_period
    if ln is not None:
        args.ln_gamma = _vec(ln[0], 'ln gamma', N).data_ptr()
        args.ln_beta = _vec(ln[1], 'ln beta', N).data_ptr()
        args.ln_eps, args.ln_count = ln_eps, (N if ln_count is None else ln_count)
    args.c, args.ldc = out.data_ptr(), _ld(out)
    args.M, args.N, args.K = M, N, K
    args.act = LIME_ACT[act]
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib.lime_linear_bf16(ctypes.byref(args), _stream()), 'lime_linear_bf16')
        e1.record()
        m_run = M if m_dev is None else min(M, int(m_dev.item()))
        PROFILE.append((lib.lime_last_linear_kernel().decode(), m_run, N, k_alg or K, n_alg or N, e0, e1))
        return out
    check(lib.lime_linear_bf16(ctypes.byref(args), _stream()), 'lime_linear_bf16')
    return out


def ffn_model_columns():
    """The column count (304) ``encoder_ffn_bf16`` carries the model dimension in."""
    return int(_lib.load().lime_ffn_bf16_model_columns())


def ffn_pack_bf16(w1, b1, w2):
    """``lime_ffn_pack_bf16``: linear1 / linear2 weights (fp32 [F, E], [F], [E, F]) -> the bf16 operands of ``encoder_ffn_bf16``."""
    lib = _lib.load()
    _mat(w1, 'w1')
    _mat(w2, 'w2')
    F, E = w1.shape
    if tuple(w2.shape) != (E, F):
        raise ValueError('w2 must be [%d, %d]' % (E, F))
    _vec(b1, 'b1', F)
    w1p = torch.empty(int(lib.lime_ffn_pack_bf16_size(F, 0)), dtype=torch.bfloat16, device=w1.device)
    w2p = torch.empty(int(lib.lime_ffn_pack_bf16_size(F, 1)), dtype=torch.bfloat16, device=w1.device)
    check(lib.lime_ffn_pack_bf16(_p(w1), _ld(w1), _p(b1), _p(w2), _ld(w2), E, F, _p(w1p), _p(w2p), _stream()), 'lime_ffn_pack_bf16')
    return w1p, w2p


def ffn_pack_sp_sizes(F):
    """Elements of the bf16 buffers (w1p, w2p) that ``ffn_pack_sp`` fills for a feed-forward width F."""
    lib = _lib.load()
    return int(lib.lime_ffn_pack_sp_size(F, 0)), int(lib.lime_ffn_pack_sp_size(F, 1))


def ffn_pack_sp(w1, w2, out=None):
    """``lime_ffn_pack_sp``: linear1 / linear2 weights (fp32 [F, E], [E, F]) -> the split (three bf16 terms) operands of ``encoder_ffn_sp``.
    ``out``: a (w1p, w2p) pair of an earlier call for the same shapes, refilled in place."""
    lib = _lib.load()
    _mat(w1, 'w1')
    _mat(w2, 'w2')
    F, E = w1.shape
    if tuple(w2.shape) != (E, F):
        raise ValueError('w2 must be [%d, %d]' % (E, F))
    n1, n2 = ffn_pack_sp_sizes(F)
    if out is not None:
        w1p, w2p = _vec(out[0], 'w1p', n1, dtype=torch.bfloat16), _vec(out[1], 'w2p', n2, dtype=torch.bfloat16)
    else:
        w1p = torch.empty(n1, dtype=torch.bfloat16, device=w1.device)
        w2p = torch.empty(n2, dtype=torch.bfloat16, device=w1.device)
    check(lib.lime_ffn_pack_sp(_p(w1), _ld(w1), _p(w2), _ld(w2), E, F, _p(w1p), _p(w2p), _stream()), 'lime_ffn_pack_sp')
    return w1p, w2p


def encoder_ffn_sp(x, w1p, w2p, b1, b2, ln, ln_eps, pool32=False, m_dev=None, out=None):
    """``lime_encoder_ffn_sp``: LayerNorm(x + W2 relu(W1 x + b1) + b2) in one launch, fp32-level split products; x fp32 [M, E].
    pool32: [M / 32, E] means over 32-row blocks, else [M, E] rows (``out`` may be a strided view)."""
    lib = _lib.load()
    _mat(x, 'x')
    _vec(w1p, 'w1p', dtype=torch.bfloat16)
    _vec(w2p, 'w2p', dtype=torch.bfloat16)
    M, E = x.shape
    F = _vec(b1, 'b1').numel()
    if w1p.numel() != int(lib.lime_ffn_pack_sp_size(F, 0)) or w2p.numel() != int(lib.lime_ffn_pack_sp_size(F, 1)):
        raise ValueError('w1p / w2p must be the two buffers of ffn_pack_sp for F = %d' % F)
    if pool32 and M % 32:
        raise ValueError('pool32 needs M %% 32 == 0 (M = %d)' % M)
    rows_out = M // 32 if pool32 else M
    if out is None:
        out = torch.empty((rows_out, E), dtype=torch.float32, device=x.device)
    _mat(out, 'out')
    if tuple(out.shape) != (rows_out, E):
        raise ValueError('out must be [%d, %d]' % (rows_out, E))
    args = _lib.FfnSpArgs()
    args.x, args.ldx = x.data_ptr(), _ld(x)
    args.w1p, args.w2p = w1p.data_ptr(), w2p.data_ptr()
    args.b1 = b1.data_ptr()
    args.b2 = _vec(b2, 'b2', E).data_ptr()
    args.ln_gamma = _vec(ln[0], 'ln gamma', E).data_ptr()
    args.ln_beta = _vec(ln[1], 'ln beta', E).data_ptr()
    args.ln_eps = ln_eps
    args.pool32 = 1 if pool32 else 0
    args.out, args.ldo = out.data_ptr(), _ld(out)
    args.M, args.E, args.F = M, E, F
    if m_dev is not None:
        args.m_dev = _vec(m_dev, 'm_dev', 1, dtype=torch.int32).data_ptr()
    if PROFILE is not None:                        # bench.py: as ONE GEMM of the two layers' FLOPs: 2 M E (2 F)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib.lime_encoder_ffn_sp(ctypes.byref(args), _stream()), 'lime_encoder_ffn_sp')
        e1.record()
        m_run = M if m_dev is None else min(M, int(m_dev.item()))
        PROFILE.append(('ffn_sp_kernel<%s>' % ('true' if pool32 else 'false'), m_run, 2 * F, E, 2 * F, e0, e1))
        return out
    check(lib.lime_encoder_ffn_sp(ctypes.byref(args), _stream()), 'lime_encoder_ffn_sp')
    return out


def device_cus():
    """``lime_device_cus``: the CU count the library sizes its persistent grids by."""
    return int(_lib.load().lime_device_cus())


def oproj_pack_sp_size():
    """Elements of the bf16 buffer that ``oproj_pack_sp`` fills."""
    return int(_lib.load().lime_oproj_pack_sp_size())


def oproj_pack_sp(w, out=None):
    """``lime_oproj_pack_sp``: the out_proj weight (fp32 [E, E]) -> the split (three bf16 terms) operand of ``encoder_oproj_sp``.
    ``out``: the buffer of an earlier call, refilled in place."""
    lib = _lib.load()
    _mat(w, 'w')
    E = w.shape[0]
    if w.shape[1] != E:
        raise ValueError('w must be square, got %s' % (tuple(w.shape),))
    n = oproj_pack_sp_size()
    wp = _vec(out, 'wp', n, dtype=torch.bfloat16) if out is not None else torch.empty(n, dtype=torch.bfloat16, device=w.device)
    check(lib.lime_oproj_pack_sp(_p(w), _ld(w), E, _p(wp), _stream()), 'lime_oproj_pack_sp')
    return wp


def encoder_oproj_sp(attn, wp, bias, ln, ln_eps, res, res_ids=None, res_pe=None, res_period=0, m_dev=None, out=None):
    """``lime_encoder_oproj_sp``: LayerNorm(residual + attn Wo^T + bias) in one launch, fp32-level split products; attn fp32 [M, E].
    The residual of row r is ``res[r]`` or, with ``res_ids`` (int32 [M]), ``res[res_ids[r]] + res_pe[r % res_period]``."""
    lib = _lib.load()
    _mat(attn, 'attn')
    M, E = attn.shape
    _vec(wp, 'wp', int(lib.lime_oproj_pack_sp_size()), dtype=torch.bfloat16)
    _mat(res, 'res')
    if res.shape[1] != E:
        raise ValueError('res must have E=%d columns' % E)
    if out is None:
        out = torch.empty((M, E), dtype=torch.float32, device=attn.device)
    _mat(out, 'out')
    if tuple(out.shape) != (M, E):
        raise ValueError('out must be [%d, %d]' % (M, E))
    args = _lib.OprojSpArgs()
    args.attn, args.lda = attn.data_ptr(), _ld(attn)
    args.wp = wp.data_ptr()
    args.bias = _vec(bias, 'bias', E).data_ptr()
    args.res, args.ldr = res.data_ptr(), _ld(res)
    if res_ids is not None:
        args.res_ids = _vec(res_ids, 'res_ids', M, dtype=torch.int32).data_ptr()
        if res_pe is not None:
            _mat(res_pe, 'res_pe')
            if res_pe.shape[1] != E or res_pe.shape[0] < res_period or res_period <= 0:
                raise ValueError('res_pe must be [>=res_period, E]')
            args.res_pe, args.ldr_pe, args.res_period = res_pe.data_ptr(), _ld(res_pe), res_period
    elif res_pe is not None:
        raise ValueError('res_pe needs res_ids')
    elif res.shape[0] < M:
        raise ValueError('res has %d rows, needs >= %d' % (res.shape[0], M))
    args.ln_gamma = _vec(ln[0], 'ln gamma', E).data_ptr()
    args.ln_beta = _vec(ln[1], 'ln beta', E).data_ptr()
    args.ln_eps = ln_eps
    args.out, args.ldo = out.data_ptr(), _ld(out)
    args.M, args.E = M, E
    if m_dev is not None:
        args.m_dev = _vec(m_dev, 'm_dev', 1, dtype=torch.int32).data_ptr()
    if PROFILE is not None:                        # bench.py: as one GEMM of 2 M E E FLOPs
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib.lime_encoder_oproj_sp(ctypes.byref(args), _stream()), 'lime_encoder_oproj_sp')
        e1.record()
        m_run = M if m_dev is None else min(M, int(m_dev.item()))
        PROFILE.append(('oproj_sp_kernel', m_run, E, E, E, e0, e1))
        return out
    check(lib.lime_encoder_oproj_sp(ctypes.byref(args), _stream()), 'lime_encoder_oproj_sp')
    return out


def split_gemm_on():
    """True while lime_linear_f32 routes the big-M GEMMs through the split-product kernel (``set_split_gemm``)."""
    return bool(_lib.load().lime_set_split_gemm(-1) & 1)


def encoder_ffn_bf16(x, w1p, w2p, b2, ln, ln_eps, E, pool32=False, m_dev=None, out=None):
    """``lime_encoder_ffn_bf16``: LayerNorm(x + W2 relu(W1 x + b1) + b2) in one launch; x bf16 [M, 304] (E real columns).
    pool32: fp32 [M / 32, 304] means over 32-row blocks, else bf16 [M, 304]."""
    lib = _lib.load()
    _mat(x, 'x', dtype=torch.bfloat16)
    _vec(w1p, 'w1p', dtype=torch.bfloat16)
    _vec(w2p, 'w2p', dtype=torch.bfloat16)
    M, DP = x.shape
    F = w2p.numel() // ffn_model_columns()
    if DP != ffn_model_columns() or w1p.numel() != int(lib.lime_ffn_pack_bf16_size(F, 0)) or w2p.numel() != int(lib.lime_ffn_pack_bf16_size(F, 1)):
        raise ValueError('x [M, %d] and the two buffers of ffn_pack_bf16 expected' % ffn_model_columns())
    if pool32 and M % 32:
        raise ValueError('pool32 needs M %% 32 == 0 (M = %d)' % M)
    rows_out, odt = (M // 32, torch.float32) if pool32 else (M, torch.bfloat16)
    if out is None:
        out = torch.empty((rows_out, DP), dtype=odt, device=x.device)
    _mat(out, 'out', dtype=odt)
    if tuple(out.shape) != (rows_out, DP):
        raise ValueError('out must be [%d, %d]' % (rows_out, DP))
    args = _lib.FfnBf16Args()
    args.x, args.ldx = x.data_ptr(), _ld(x)
    args.w1p, args.w2p = w1p.data_ptr(), w2p.data_ptr()
    args.b2 = _vec(b2, 'b2', E).data_ptr()
    args.ln_gamma = _vec(ln[0], 'ln gamma', E).data_ptr()
    args.ln_beta = _vec(ln[1], 'ln beta', E).data_ptr()
    args.ln_eps = ln_eps
    args.pool32 = 1 if pool32 else 0
    args.out, args.ldo = out.data_ptr(), _ld(out)
    args.M, args.E, args.F = M, E, F
    if m_dev is not None:
        args.m_dev = _vec(m_dev, 'm_dev', 1, dtype=torch.int32).data_ptr()
    if PROFILE is not None:                        # bench.py: as ONE GEMM of the two layers' FLOPs: 2 M E (2 F)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib.lime_encoder_ffn_bf16(ctypes.byref(args), _stream()), 'lime_encoder_ffn_bf16')
        e1.record()
        m_run = M if m_dev is None else min(M, int(m_dev.item()))
        PROFILE.append(('ffn_bf16_kernel<%s, false>' % ('true' if pool32 else 'false'), m_run, 2 * F, E, 2 * F, e0, e1))
        return out
    check(lib.lime_encoder_ffn_bf16(ctypes.byref(args), _stream()), 'lime_encoder_ffn_bf16')
    return out


def inproj_pack_bf16(w, K):
    """``lime_inproj_pack_bf16``: in_proj weight (fp32 [N, E], heads padded to 32 columns: N % 320 == 0) -> the bf16 ring slots of
    ``inproj_bf16``; K: the column count of the bf16 operand rows (E rounded up to 8; the columns beyond E get zero weights)."""
    lib = _lib.load()
    _mat(w, 'w')
    N = w.shape[0]
    if w.shape[1] > K:
        raise ValueError('K must cover the weight columns')
    wp = torch.empty(int(lib.lime_inproj_pack_bf16_size(N)), dtype=torch.bfloat16, device=w.device)
    check(lib.lime_inproj_pack_bf16(_p(w), _ld(w), N, w.shape[1], _p(wp), _stream()), 'lime_inproj_pack_bf16')
    return wp


def inproj_bf16(a, wp, add_rows, N, out, a_ids=None, c_ids=None, m_dev=None):
    """``lime_inproj_bf16``: out[c_ids[r] or r] = bf16(a[a_ids[r] or r] . w^T + add_rows[(c_ids[r] or r) % period]); a bf16 [*, K]."""
    lib = _lib.load()
    _mat(a, 'a', dtype=torch.bfloat16)
    _mat(out, 'out', dtype=torch.bfloat16)
    _mat(add_rows, 'add_rows')
    K = a.shape[1]
    M = a_ids.numel() if a_ids is not None else a.shape[0]
    if out.shape[1] != N or add_rows.shape[1] < N or wp.numel() != int(lib.lime_inproj_pack_bf16_size(N)):
        raise ValueError('out must have N columns, add_rows >= N columns, wp must come from inproj_pack_bf16')
    args = _lib.InprojBf16Args()
    args.a, args.lda, args.a_rows = a.data_ptr(), _ld(a), a.shape[0]
    args.a_ids = _vec(a_ids, 'a_ids', dtype=torch.int32).data_ptr() if a_ids is not None else None
    args.wp = _vec(wp, 'wp', dtype=torch.bfloat16).data_ptr()
    args.add_rows, args.ld_add, args.add_period = add_rows.data_ptr(), _ld(add_rows), add_rows.shape[0]
    args.M, args.N, args.K = M, N, K
    args.c_ids = _vec(c_ids, 'c_ids', M, dtype=torch.int32).data_ptr() if c_ids is not None else None
    args.out, args.ldo, args.out_rows = out.data_ptr(), _ld(out), out.shape[0]
    if m_dev is not None:
        args.m_dev = _vec(m_dev, 'm_dev', 1, dtype=torch.int32).data_ptr()
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib.lime_inproj_bf16(ctypes.byref(args), _stream()), 'lime_inproj_bf16')
        e1.record()
        m_run = M if m_dev is None else min(M, int(m_dev.item()))
        PROFILE.append(('inproj_bf16_kernel', m_run, N, K // 8 * 8 - (4 if K == 304 else 0), N * 30 // 32, e0, e1))
        return out
    check(lib.lime_inproj_bf16(ctypes.byref(args), _stream()), 'lime_inproj_bf16')
    return out


def oproj_pack_bf16(w):
    """``lime_oproj_pack_bf16``: out_proj weight (fp32 [E, E]) -> the bf16 ring slots of ``encoder_block_bf16``."""
    lib = _lib.load()
    _mat(w, 'w')
    E = w.shape[0]
    if w.shape[1] != E:
        raise ValueError('w must be square')
    wp = torch.empty(int(lib.lime_oproj_pack_bf16_size()), dtype=torch.bfloat16, device=w.device)
    check(lib.lime_oproj_pack_bf16(_p(w), _ld(w), E, _p(wp), _stream()), 'lime_oproj_pack_bf16')
    return wp


def _aligned16(t):
    return t if t.data_ptr() % 16 == 0 else t.clone()


def encoder_block_bf16(attn, w0p, add_rows, ln1, ln1_eps, res, res_kind, w1p, w2p, b2, ln2, ln2_eps, E, res_ids=None, pool32=False, m_dev=None,
                       out=None):
    """``lime_encoder_block_bf16``: out_proj + residual + norm1 + linear1 + ReLU + linear2 + residual + norm2 (+ 32-row block means) in
    one launch.  attn bf16 [M, 304]; res_kind 2: res = bf16 table gathered by res_ids, 3: res = bf16 rows [M, 304]; add_rows fp32
    [period, >= E]: out_proj's bias (+ the positional rows), row r % period goes to token r."""
    lib = _lib.load()
    _mat(attn, 'attn', dtype=torch.bfloat16)
    _mat(res, 'res', dtype=torch.bfloat16)
    _mat(add_rows, 'add_rows')
    M, DP = attn.shape
    F = w2p.numel() // ffn_model_columns()
    if DP != ffn_model_columns() or res.shape[1] != DP:
        raise ValueError('attn and res must have %d columns' % ffn_model_columns())
    if add_rows.shape[1] < E:
        raise ValueError('add_rows must have >= E columns')
    if (w0p.numel() != int(lib.lime_oproj_pack_bf16_size()) or w1p.numel() != int(lib.lime_ffn_pack_bf16_size(F, 0)) or
            w2p.numel() != int(lib.lime_ffn_pack_bf16_size(F, 1))):
        raise ValueError('w0p / w1p / w2p must come from oproj_pack_bf16 / ffn_pack_bf16')
    if pool32 and M % 32:
        raise ValueError('pool32 needs M %% 32 == 0 (M = %d)' % M)
    rows_out, odt = (M // 32, torch.float32) if pool32 else (M, torch.bfloat16)
    if out is None:
        out = torch.empty((rows_out, DP), dtype=odt, device=attn.device)
    _mat(out, 'out', dtype=odt)
    if tuple(out.shape) != (rows_out, DP):
        raise ValueError('out must be [%d, %d]' % (rows_out, DP))
    keep = [_aligned16(_vec(ln1[0], 'ln1 gamma', E)), _aligned16(_vec(ln1[1], 'ln1 beta', E))]
    args = _lib.EncoderBlockBf16Args()
    args.attn, args.lda = attn.data_ptr(), _ld(attn)
    args.w0p = _vec(w0p, 'w0p', dtype=torch.bfloat16).data_ptr()
    args.add_rows, args.ld_add, args.add_period = add_rows.data_ptr(), _ld(add_rows), add_rows.shape[0]
    args.ln1_gamma, args.ln1_beta, args.ln1_eps = keep[0].data_ptr(), keep[1].data_ptr(), ln1_eps
    args.res_kind = res_kind
    args.res, args.ldr, args.res_rows = res.data_ptr(), _ld(res), res.shape[0]
    if res_kind == 2:
        args.res_ids = _vec(res_ids, 'res_ids', M, dtype=torch.int32).data_ptr()
    elif res_kind == 3:
        if res.shape[0] < M:
            raise ValueError('res has too few rows')
    else:
        raise ValueError('res_kind must be 2 or 3')
    args.pool32 = 1 if pool32 else 0
    args.w1p, args.w2p = _vec(w1p, 'w1p', dtype=torch.bfloat16).data_ptr(), _vec(w2p, 'w2p', dtype=torch.bfloat16).data_ptr()
    args.b2 = _vec(b2, 'b2', E).data_ptr()
    args.ln2_gamma, args.ln2_beta, args.ln2_eps = _vec(ln2[0], 'ln2 gamma', E).data_ptr(), _vec(ln2[1], 'ln2 beta', E).data_ptr(), ln2_eps
    args.M, args.E, args.F = M, E, F
    args.out, args.ldo = out.data_ptr(), _ld(out)
    if m_dev is not None:
        args.m_dev = _vec(m_dev, 'm_dev', 1, dtype=torch.int32).data_ptr()
    if PROFILE is not None:                        # bench.py: as ONE GEMM of the block's FLOPs: 2 M (E E + 2 E F) = 2 M E (E + 2 F)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib.lime_encoder_block_bf16(ctypes.byref(args), _stream()), 'lime_encoder_block_bf16')
        e1.record()
        m_run = M if m_dev is None else min(M, int(m_dev.item()))
        PROFILE.append(('ffn_bf16_kernel<%s, true>' % ('true' if pool32 else 'false'), m_run, DP + 2 * F, E, E + 2 * F, e0, e1))
        return out
    check(lib.lime_encoder_block_bf16(ctypes.byref(args), _stream()), 'lime_encoder_block_bf16')
    return out


def mean_pool_bf16(x, n_seq, S, dim, out=None):
    lib = _lib.load()
    _mat(x, 'x', dtype=torch.bfloat16)
    if x.shape[0] != n_seq * S:
        raise ValueError('x must have n_seq * S rows')
    if out is None:
        out = torch.empty((n_seq, dim), dtype=torch.float32, device=x.device)
    _mat(out, 'out')
    check(lib.lime_mean_pool_bf16(_p(x), _ld(x), _p(out), _ld(out), n_seq, S, dim, _stream()), 'lime_mean_pool_bf16')
    return out


def token_attention_rows_bf16(q, k, v, row_map, n_seq_dev, n_seq, S, n_head, head_dim, scale, out_cols=None, out=None):
    """``lime_token_attention_rows_bf16``: the bf16 attention over compacted sequences (see ``token_attention_rows``)."""
    lib = _lib.load()
    for t, n in ((q, 'q'), (k, 'k'), (v, 'v')):
        _mat(t, n, dtype=torch.bfloat16)
        if t.shape[1] != n_head * 32:
            raise ValueError('%s must have n_head * 32 columns' % n)
    if not (_ld(q) == _ld(k) == _ld(v)):
        raise ValueError('q, k and v must share one leading dimension')
    _vec(row_map, 'row_map', dtype=torch.int32)
    if row_map.numel() < n_seq * S:
        raise ValueError('row_map must cover n_seq * S tokens')
    if n_seq_dev is not None:
        _vec(n_seq_dev, 'n_seq_dev', 1, dtype=torch.int32)
    out_cols = n_head * head_dim if out_cols is None else out_cols
    if out is None:
        out = torch.empty((n_seq * S, out_cols), dtype=torch.bfloat16, device=q.device)
    _mat(out, 'out', dtype=torch.bfloat16)
    check(lib.lime_token_attention_rows_bf16(_p(q), _p(k), _p(v), _ld(q), _p(row_map), _p(n_seq_dev), _p(out), _ld(out), n_seq, S, n_head,
                                             head_dim, scale, out_cols, _stream()), 'lime_token_attention_rows_bf16')
    return out


def token_attention_bf16(q, k, v, n_seq, S, n_head, head_dim, scale, out_cols=None, out=None):
    """Unmasked encoder attention on bf16 storage: q / k / v [n_seq * S, n_head * 32] bf16 views of one qkv buffer."""
    lib = _lib.load()
    for t, name in ((q, 'q'), (k, 'k'), (v, 'v')):
        _mat(t, name, dtype=torch.bfloat16)
        if t.shape[0] != n_seq * S or t.shape[1] != n_head * 32:
            raise ValueError('%s must be [n_seq * S, n_head * 32]' % name)
    if not (_ld(q) == _ld(k) == _ld(v)):
        raise ValueError('q, k, v must share one leading dimension')
    out_cols = n_head * head_dim if out_cols is None else out_cols
    if out is None:
        out = torch.empty((n_seq * S, out_cols), dtype=torch.bfloat16, device=q.device)
    _mat(out, 'out', dtype=torch.bfloat16)
    check(lib.lime_token_attention_bf16(_p(q), _p(k), _p(v), _ld(q), _p(out), _ld(out), n_seq, S, n_head, head_dim, scale, out_cols,
                                        _stream()), 'lime_token_attention_bf16')
    return out


def gather_rows_multi_prepare(n_rows, pairs):
    """Validate (table, out) pairs once and build the descriptor tables: returns an opaque plan for gather_rows_multi_run.
    Tables / outputs: any dtype, row-major with contiguous rows ([n, ...] -> rows of prod(shape[1:]) elements); every
    out has n_rows rows.  The plan keeps the tensors alive."""
    todo = []
    for table, out in pairs:
        if table.dtype != out.dtype or not table.is_cuda or not out.is_cuda or table.shape[1:] != out.shape[1:] or out.shape[0] != n_rows:
            raise ValueError('gather_rows_multi: table %s %s vs out %s %s (rows %d)' % (tuple(table.shape), table.dtype,
                                                                                        tuple(out.shape), out.dtype, n_rows))
        if not table.is_contiguous() or not out.is_contiguous():
            raise ValueError('gather_rows_multi: tables and outputs must be contiguous')
        todo.append((table, out))
    tables = []
    for i in range(0, len(todo), _lib.MAX_GATHERS):
        part = todo[i:i + _lib.MAX_GATHERS]
        descs = (_lib.GatherDesc * len(part))()
        for d, (table, out) in zip(descs, part):
            rb = (table.numel() // max(1, table.shape[0])) * table.element_size()
            d.table, d.table_stride, d.out, d.out_stride, d.row_bytes = table.data_ptr(), rb, out.data_ptr(), rb, rb
        tables.append((descs, len(part)))
    return {'n_rows': n_rows, 'tables': tables, 'keep': todo}


def gather_rows_multi_run(idx, plan):
    lib = _lib.load()
    if idx.dtype != torch.int32 or not idx.is_cuda or not idx.is_contiguous() or idx.numel() != plan['n_rows']:
        raise ValueError('gather_rows_multi: idx must be a contiguous int32 CUDA vector of %d rows' % plan['n_rows'])
    stream = _stream()
    for descs, n in plan['tables']:
        check(lib.lime_gather_rows_multi(idx.data_ptr(), plan['n_rows'], descs, n, stream), 'lime_gather_rows_multi')


def gather_rows_multi(idx, pairs):
    """out[r] = table[idx[r]] for every (table, out) pair, one launch per 16 pairs."""
    _vec(idx, 'idx', dtype=torch.int32)
    gather_rows_multi_run(idx, gather_rows_multi_prepare(idx.numel(), pairs))


# ---- training step (include/lime_hip.h, "Training step") ------------------------------------------------------------------
_WS = {}


def _workspace(device, floats):
    """A per-device scratch buffer for the fixed-order reductions (grown on demand; launches on one stream are ordered, so
    consecutive kernels can share it)."""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < floats:
        ws = torch.empty(max(int(floats), 1 << 20), dtype=torch.float32, device=device)
        _WS[key] = ws
    return ws


def linear_wgrad(dy, x, out=None, accumulate=False, bias_out=None, want_bias=False):
    """dW [N, K] (+)= dy^T x  (dy [M, N], x [M, K]); with ``want_bias`` / ``bias_out`` also db [N] (+)= column sums of dy,
    returned as (dW, db)."""
    lib = _lib.load()
    _mat(dy, 'dy')
    _mat(x, 'x')
    M, N = dy.shape
    K = x.shape[1]
    if x.shape[0] != M:
        raise ValueError('dy has %d rows, x has %d' % (M, x.shape[0]))
    if out is None:
        if accumulate:
            raise ValueError('accumulate needs out')
        out = torch.empty((N, K), dtype=torch.float32, device=dy.device)
    _mat(out, 'out')
    if tuple(out.shape) != (N, K):
        raise ValueError('out must be [%d, %d]' % (N, K))
    if bias_out is None and want_bias:
        if accumulate:
            raise ValueError('accumulate needs bias_out')
        bias_out = torch.empty(N, dtype=torch.float32, device=dy.device)
    if bias_out is not None:
        _vec(bias_out, 'bias_out', N)
    if M == 0:
        if not accumulate:
            out.zero_()
            if bias_out is not None:
                bias_out.zero_()
    else:
        need = lib.lime_linear_wgrad_workspace(M, N, K)
        ws = _workspace(dy.device, need)
        if PROFILE is not None:                    # bench.py: HIP events around the launch pair (wgrad + partial-sum reduction)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        check(lib.lime_linear_wgrad_f32(_p(dy), _ld(dy), _p(x), _ld(x), _p(out), _ld(out), _p(bias_out), M, N, K,
                                        1 if accumulate else 0, _p(ws), ws.numel(), _stream()), 'lime_linear_wgrad_f32')
        if PROFILE is not None:
            e1.record()
            PROFILE.append(('wgrad_kernel + reduce_partials_kernel (dW = dY^T X)', M, N, K, N, e0, e1))
    return out if bias_out is None else (out, bias_out)


def colsum(x, out=None, accumulate=False):
    """out [N] (+)= column sums of x [M, N]."""
    lib = _lib.load()
    _mat(x, 'x')
    M, N = x.shape
    if out is None:
        if accumulate:
            raise ValueError('accumulate needs out')
        out = torch.empty(N, dtype=torch.float32, device=x.device)
    _vec(out, 'out', N)
    if M == 0:
        return out if accumulate else out.zero_()
    ws = _workspace(x.device, lib.lime_colsum_workspace(M, N))
    check(lib.lime_colsum_f32(_p(x), _ld(x), M, N, _p(out), 1 if accumulate else 0, _p(ws), ws.numel(), _stream()), 'lime_colsum_f32')
    return out


def layernorm_bwd(dy, y, gamma, beta, rstd, dy_div=1, dy_scale=1.0, want_dzsum=True, dropout=None):
    """Backward of y = LayerNorm(z): returns (dz [M, E], dgamma, dbeta, dzsum or None).  dy: [ceil(M / dy_div), E].
    ``dropout`` = (p, seed, site): a fifth result, dropout(dz) under that site's mask, written in the same pass; dzsum is then the
    column sums of THAT (the bias gradient of the linear in front of the dropout)."""
    lib = _lib.load()
    _mat(dy, 'dy')
    _mat(y, 'y')
    M, E = y.shape
    if dy.shape[1] != E or dy.shape[0] * dy_div < M:
        raise ValueError('dy must be [>= %d, %d]' % ((M + dy_div - 1) // dy_div, E))
    _vec(gamma, 'gamma', E)
    _vec(beta, 'beta', E)
    _vec(rstd, 'rstd', M)
    dev = y.device
    dz = torch.empty((M, E), dtype=torch.float32, device=dev)
    dgamma = torch.empty(E, dtype=torch.float32, device=dev)
    dbeta = torch.empty(E, dtype=torch.float32, device=dev)
    dzsum = torch.empty(E, dtype=torch.float32, device=dev) if want_dzsum else None
    ws = _workspace(dev, lib.lime_layernorm_bwd_workspace(M, E))
    if dropout is not None:
        if E % 4 or _ld(dy) % 4 or _ld(y) % 4:           # the fused copy needs 16-byte rows: otherwise a dropout pass of its own
            res = layernorm_bwd(dy, y, gamma, beta, rstd, dy_div, dy_scale, False)
            dt = globals()['dropout'](res[0], *dropout)
            return res[:3] + (colsum(dt) if want_dzsum else None, dt)
        dt = torch.empty((M, E), dtype=torch.float32, device=dev)
        check(lib.lime_layernorm_bwd_dropout_f32(_p(dy), _ld(dy), dy_div, dy_scale, _p(y), _ld(y), _p(gamma), _p(beta), _p(rstd), _p(dz),
                                                 _ld(dz), M, E, _p(dgamma), _p(dbeta), _p(dzsum), 0, _p(ws), ws.numel(), _p(dt), _ld(dt),
                                                 dropout[0], dropout[1], dropout[2], _stream()), 'lime_layernorm_bwd_dropout_f32')
        return dz, dgamma, dbeta, dzsum, dt
    check(lib.lime_layernorm_bwd_f32(_p(dy), _ld(dy), dy_div, dy_scale, _p(y), _ld(y), _p(gamma), _p(beta), _p(rstd), _p(dz), _ld(dz),
                                     M, E, _p(dgamma), _p(dbeta), _p(dzsum), 0, _p(ws), ws.numel(), _stream()),
          'lime_layernorm_bwd_f32')
    return dz, dgamma, dbeta, dzsum


def relu_bwd_(dh, h, scale=1.0):
    """dh = dh * scale where h > 0, else 0 -- in place."""
    lib = _lib.load()
    _mat(dh, 'dh')
    _mat(h, 'h')
    if dh.shape != h.shape:
        raise ValueError('dh and h differ in shape')
    check(lib.lime_relu_bwd_f32(_p(dh), _ld(dh), _p(h), _ld(h), dh.shape[0], dh.shape[1], scale, _stream()), 'lime_relu_bwd_f32')
    return dh


def _token_attention_bwd_block(q, k, v, dout, n_seq, S, n_head, head_dim, scale, head_stride, dqkv, out, dropout, key_mask, lse):
    """(lime_token_attention_bwd_args, dqkv, what the block points into and nobody else holds) for ``token_attention_bwd``'s arguments: the operand checks,
    the workspace and the choice between the entry's two forms, for the call and for its plan."""
    lib = _lib.load()
    hs = head_dim if head_stride is None else head_stride
    W = n_head * hs
    for t, name in ((q, 'q'), (k, 'k'), (v, 'v')):
        _mat(t, name)
        if t.shape[0] != n_seq * S or t.shape[1] != W:
            raise ValueError('%s must be [n_seq * S, n_head * head_stride]' % name)
    if not (_ld(q) == _ld(k) == _ld(v)):
        raise ValueError('q, k, v must share one leading dimension')
    _mat(dout, 'dout')
    if tuple(dout.shape) != (n_seq * S, n_head * head_dim):
        raise ValueError('dout must be [n_seq * S, n_head * head_dim]')
    if dqkv is None:
        dqkv = torch.empty((n_seq * S, 3 * W), dtype=torch.float32, device=q.device)
    _mat(dqkv, 'dqkv')
    dq, dk, dv = dqkv[:, :W], dqkv[:, W:2 * W], dqkv[:, 2 * W:]
    wide = head_dim > 32
    ws, need = None, lib.lime_token_attention_bwd_workspace_wide(n_seq, S, n_head, head_dim)
    if wide:
        ws = _workspace(q.device, need) if need else None
        if out is not None:
            _mat(out, 'out')
    elif need:
        if out is None:
            raise ValueError('S > 128 needs the forward output `out`')
        _mat(out, 'out')
        if tuple(out.shape) != tuple(dout.shape):
            raise ValueError('out must have the shape of dout')
        ws = _workspace(q.device, need)
    # The lse entry is used only where a workspace is needed (narrow heads: S > 128, where the forward's lse saves the statistics pass)
    # and, for wide heads (which need one at every S and read neither), only with S > 128 and `out` given -- the call a narrow head
    # would make.  Everywhere else lse is ignored and the plain entry speaks.
    use_lse = bool(lse is not None and need and (not wide or (S > 128 and out is not None)))
    a = _lib.TokenAttentionBwdArgs()
    ptr = lambda t: None if t is None else t.data_ptr()
    a.q, a.k, a.v, a.ld_qkv = ptr(q), ptr(k), ptr(v), _ld(q)
    a.dout, a.ldo, a.dq, a.dk, a.dv, a.ld_dqkv = ptr(dout), _ld(dout), ptr(dq), ptr(dk), ptr(dv), _ld(dqkv)
    a.n_seq, a.S, a.n_head, a.head_dim, a.head_stride, a.scale = n_seq, S, n_head, head_dim, hs, scale
    a.workspace, a.workspace_floats = ptr(ws), ws.numel() if ws is not None else 0
    if use_lse:
        if dropout or key_mask is not None:
            raise ValueError('lse goes with the plain (no dropout, no key mask) forward')
        _vec(lse, 'lse', n_seq * S * n_head)
        a.entry, a.out, a.ld_out, a.lse = _lib.BWD_ATTN_ENTRY['lse'], ptr(out), _ld(out), ptr(lse)
        return a, dqkv, ws
    key_mask = _mask_u8(key_mask, 'key_mask')
    a.entry, a.out, a.ld_out, a.key_mask = _lib.BWD_ATTN_ENTRY['plain'], ptr(out), _ld(out) if out is not None else 0, ptr(key_mask)
    a.dropout_p, a.dropout_seed, a.dropout_site = dropout or (0.0, 0, 0)
    return a, dqkv, (ws, key_mask)


def token_attention_bwd(q, k, v, dout, n_seq, S, n_head, head_dim, scale, head_stride=None, dqkv=None, out=None,
                        dropout=None, key_mask=None, lse=None):
    """Backward of the unmasked ``token_attention``: q / k / v column views of one packed qkv buffer [tokens, 3 * n_head *
    head_stride]; returns dqkv in the same layout.  ``out``: the forward's result (needed for S > 128).  ``dropout``:
    (p, seed, site) of the ``token_attention_dropout`` forward.  head_dim ranges as ``token_attention``; the wide heads
    (32 < head_dim <= 128) recompute their statistics at every S: ``out`` and ``lse`` are optional and unused there."""
    a, dqkv, _keep = _token_attention_bwd_block(q, k, v, dout, n_seq, S, n_head, head_dim, scale, head_stride, dqkv, out, dropout, key_mask, lse)
    check(_lib.load().lime_token_attention_bwd_f32(ctypes.byref(a), _stream()), 'lime_token_attention_bwd_f32')
    return dqkv


def token_attention_bwd_plan(q, k, v, dout, n_seq, S, n_head, head_dim, scale, head_stride=None, dqkv=None, out=None,
                             dropout=None, key_mask=None, lse=None):
    """What ``token_attention_bwd`` would run for the same arguments, without running it (``lime_token_attention_bwd_plan_f32``): a dict
    with ``family`` ('one_pass', 'sp', 'long', 'long_sp', 'wide'; None where nothing is launched), ``stats_pass`` (None / 'fp32' /
    'split' / 'delta') and ``kernels`` (the instantiations in launch order, as rocprofv3 prints them).  A call the wrapper or the entry
    would refuse raises the same error."""
    a, _dqkv, _keep = _token_attention_bwd_block(q, k, v, dout, n_seq, S, n_head, head_dim, scale, head_stride, dqkv, out, dropout, key_mask, lse)
    plan = _lib.TokenAttentionBwdPlan()
    check(_lib.load().lime_token_attention_bwd_plan_f32(ctypes.byref(a), ctypes.byref(plan)), 'lime_token_attention_bwd_plan_f32')
    return dict(family=_lib.BWD_ATTN_FAMILY[plan.family], stats_pass=_lib.BWD_ATTN_PASS[plan.stats_pass],
                kernels=[plan.name[i].value.decode() for i in range(plan.n_launches)])


def dropout2(src, p, seed, site1, site2, out=None):
    """dropout_site2(dropout_site1(src)) in one pass; ``out`` may be ``src``."""
    lib = _lib.load()
    _mat(src, 'src')
    if out is None:
        out = torch.empty(tuple(src.shape), dtype=torch.float32, device=src.device)
    _mat(out, 'out')
    if out.shape != src.shape:
        raise ValueError('out must have the shape of src')
    check(lib.lime_dropout2_f32(_p(src), _ld(src), _p(out), _ld(out), src.shape[0], src.shape[1], p, seed, site1, site2, _stream()),
          'lime_dropout2_f32')
    return out


def dropout(src, p, seed, site, out=None):
    """keep * src / (1 - p) with the counter-based mask of (seed, site); ``out`` may be ``src`` (in place)."""
    lib = _lib.load()
    _mat(src, 'src')
    if out is None:
        out = torch.empty(tuple(src.shape), dtype=torch.float32, device=src.device)
    _mat(out, 'out')
    if out.shape != src.shape:
        raise ValueError('out must have the shape of src')
    check(lib.lime_dropout_f32(_p(src), _ld(src), _p(out), _ld(out), src.shape[0], src.shape[1], p, seed, site, _stream()), 'lime_dropout_f32')
    return out


def embed_pe_dropout(ids, table, pe, period, p, seed, site_emb, site_pe):
    """drop(drop(table[ids]) + pe[r % period]) -> [len(ids), dim]; ``pe`` None: drop(drop(table[ids]))."""
    lib = _lib.load()
    _vec(ids, 'ids', dtype=torch.int32)
    _mat(table, 'table')
    if pe is not None:
        _mat(pe, 'pe')
        if pe.shape[1] != table.shape[1] or period <= 0 or pe.shape[0] < period:
            raise ValueError('pe must be [>= period, dim]')
    out = torch.empty((ids.numel(), table.shape[1]), dtype=torch.float32, device=table.device)
    check(lib.lime_embed_pe_dropout_f32(_p(ids), _p(table), _ld(table), _p(pe), _ld(pe) if pe is not None else 0, period, _p(out), _ld(out), ids.numel(),
                                        table.shape[1], p, seed, site_emb, site_pe, _stream()), 'lime_embed_pe_dropout_f32')
    return out


def dropout_add_layernorm(t, res, gamma, beta, eps, p, seed, site, want_rstd=True):
    """(LayerNorm(res + drop(t)), rstd)."""
    lib = _lib.load()
    _mat(t, 't')
    _mat(res, 'res')
    M, E = t.shape
    if res.shape != t.shape:
        raise ValueError('res must have the shape of t')
    _vec(gamma, 'gamma', E)
    _vec(beta, 'beta', E)
    y = torch.empty((M, E), dtype=torch.float32, device=t.device)
    rstd = torch.empty(M, dtype=torch.float32, device=t.device) if want_rstd else None
    check(lib.lime_dropout_add_layernorm_f32(_p(t), _ld(t), _p(res), _ld(res), _p(gamma), _p(beta), eps, _p(y), _ld(y), _p(rstd), M, E,
                                             p, seed, site, _stream()), 'lime_dropout_add_layernorm_f32')
    return y, rstd


def token_attention_dropout(q, k, v, n_seq, S, n_head, head_dim, scale, p, seed, site, head_stride=None):
    """Unmasked encoder attention with dropout on the probabilities (training mode); layouts and head_dim ranges (<= 32, or the
    wide heads up to 128) as ``token_attention``."""
    return _token_attention('dropout', q=q, k=k, v=v, n_seq=n_seq, S=S, n_head=n_head, head_dim=head_dim, scale=scale, p=p, seed=seed,
                            site=site, head_stride=head_stride)


DETERMINISTIC_EMBED_BWD = True      # word-table gradient by sort + segmented sum (no atomics); False: the float-atomic kernel


def embed_bwd(ids, dx, dtable, hot_id=0, accumulate=False):
    """dtable[ids[r]] = sum of dx[r] over the rows with that id, for a dtable the caller ZEROED (rows no id names are left alone).
    Tables of <= 32 rows: atomic-free LDS accumulation; larger tables with dim <= 320: stable sort of the positions by id +
    segmented sum in a fixed order (lime_embed_bwd_sorted_f32: bitwise reproducible) -- this back end STORES each touched row, the
    other two ADD into it, so a dtable that already holds a gradient needs ``accumulate=True`` (the sorted back end then sums into a
    zeroed scratch table and adds it: the same result on every back end); otherwise (or with DETERMINISTIC_EMBED_BWD off) float
    atomics."""
    lib = _lib.load()
    _vec(ids, 'ids', dtype=torch.int32)
    _mat(dx, 'dx')
    _mat(dtable, 'dtable')
    if dx.shape[0] != ids.numel() or dx.shape[1] != dtable.shape[1]:
        raise ValueError('dx must be [len(ids), dim]')
    if dtable.shape[0] <= 32:              # a handful of rows: per-column LDS accumulation instead of contended atomics
        check(lib.lime_embed_bwd_small_f32(_p(ids), _p(dx), _ld(dx), _p(dtable), _ld(dtable), ids.numel(), dx.shape[1],
                                           dtable.shape[0], _stream()), 'lime_embed_bwd_small_f32')
        return dtable
    if DETERMINISTIC_EMBED_BWD and dx.shape[1] <= 320 and ids.numel() > 0:
        if accumulate:
            return dtable.add_(embed_bwd(ids, dx, torch.zeros_like(dtable), hot_id))
        sorted_ids, order = torch.sort(ids, stable=True)
        order = order.to(torch.int32)
        need = int(lib.lime_embed_bwd_sorted_workspace(ids.numel(), dx.shape[1]))
        ws = torch.empty(need, dtype=torch.float32, device=dx.device)
        check(lib.lime_embed_bwd_sorted_f32(_p(order), _p(sorted_ids), _p(dx), _ld(dx), _p(dtable), _ld(dtable), ids.numel(), dx.shape[1],
                                            _p(ws), need, _stream()), 'lime_embed_bwd_sorted_f32')
        return dtable
    check(lib.lime_embed_bwd_f32(_p(ids), _p(dx), _ld(dx), _p(dtable), _ld(dtable), ids.numel(), dx.shape[1], hot_id, _stream()),
          'lime_embed_bwd_f32')
    return dtable


def grad_clip_coef(g, max_norm):
    """[norm, min(1, max_norm / (norm + 1e-6))] of the flat gradient buffer, as a 2-element device tensor."""
    lib = _lib.load()
    _vec(g, 'g')
    out = torch.empty(2, dtype=torch.float32, device=g.device)
    ws = _workspace(g.device, 1024)
    check(lib.lime_grad_clip_coef_f32(_p(g), g.numel(), float(max_norm), _p(out), _p(ws), ws.numel(), _stream()), 'lime_grad_clip_coef_f32')
    return out


def adam_step_(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=None):
    lib = _lib.load()
    note_param_write()                             # p is written through its address: no tensor's _version moves
    n = p.numel()
    for t, name in ((p, 'p'), (g, 'g'), (m, 'm'), (v, 'v')):
        _vec(t, name, n)
    check(lib.lime_adam_f32(_p(p), _p(g), _p(m), _p(v), n, lr, betas[0], betas[1], eps, weight_decay, step, _p(grad_scale), _stream()),
          'lime_adam_f32')
    return p


def nll_softmax(logits, want_grad=True):
    """(loss [1], dlogits [B, K] or None) of trainer.py:71-73."""
    lib = _lib.load()
    _mat(logits, 'logits')
    B, K = logits.shape
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    d = torch.empty((B, K), dtype=torch.float32, device=logits.device) if want_grad else None
    check(lib.lime_nll_softmax_f32(_p(logits), _ld(logits), B, K, _p(loss), _p(d), _ld(d) if d is not None else K, _stream()),
          'lime_nll_softmax_f32')
    return loss, d


def linear_xent(x, w, b, target, scale, want_grads=True):
    """The linear classifier z = x w^T + b and its cross-entropy against ``target`` in one launch (``lime_linear_xent_f32``): ->
    (loss [1], row_loss [M], dlogits [M, C] or None, dx [M, D] or None) with row_loss = scale (logsumexp(z) - z[target]), loss their
    fixed-order sum (the column-sum kernel), dlogits = scale (softmax(z) - onehot(target)) and dx = dlogits w.  x [M, D] may be a
    column slice of a wider tensor; w [C, D] with C <= 1024; b [C] or None; target int32 [M] -- a target outside [0, C) is the all-zero
    one-hot row (zero loss, zero gradients).  ``scale`` = weight / M gives the weighted mean over the rows."""
    # shapes first (they read no device memory), then dtype / device / layout
    for t, name in ((x, 'x'), (w, 'w')):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError('%s must be a 2-D tensor' % name)
    M, D = x.shape
    C = w.shape[0]
    if w.shape[1] != D:
        raise ValueError('x has %d columns, w has %d' % (D, w.shape[1]))
    if M < 1 or D < 1 or not 1 <= C <= 1024:
        raise ValueError('linear_xent needs M >= 1, D >= 1 and 1 <= C <= 1024, got M = %d, D = %d, C = %d' % (M, D, C))
    if not isinstance(target, torch.Tensor) or target.dtype != torch.int32:
        raise TypeError('target must be an int32 tensor')
    if target.numel() != M or (b is not None and b.numel() != C):
        raise ValueError('target must have M = %d elements and b C = %d' % (M, C))
    _mat(x, 'x')
    _mat(w, 'w')
    if not w.is_contiguous():
        raise ValueError('w must be contiguous')
    _vec(b, 'b', C)
    _vec(target, 'target', M, dtype=torch.int32)
    lib = _lib.load()
    row_loss = torch.empty(M, dtype=torch.float32, device=x.device)
    d = torch.empty((M, C), dtype=torch.float32, device=x.device) if want_grads else None
    dx = torch.empty((M, D), dtype=torch.float32, device=x.device) if want_grads else None
    check(lib.lime_linear_xent_f32(_p(x), _ld(x), _p(w), _p(b), _p(target), float(scale), _p(row_loss), _p(d), _p(dx), D, M, D, C,
                                   _stream()), 'lime_linear_xent_f32')
    return colsum(row_loss.view(M, 1)), row_loss, d, dx


# ---- backward of the fused tail kernels -----------------------------------------------------------------------------------
def intent_fuse_bwd(intents, att_hidden, affine2_t, affine2_b, dcontent, M, k, D, A):
    """-> (d_intents [2Mk, D], d_hidden [2Mk, A], d_affine2_title [A], d_affine2_body [A])."""
    lib = _lib.load()
    _mat(intents, 'intents')
    _mat(att_hidden, 'att_hidden')
    _mat(dcontent, 'dcontent')
    if not (intents.is_contiguous() and att_hidden.is_contiguous()) or tuple(intents.shape) != (2 * M * k, D) or \
            tuple(att_hidden.shape) != (2 * M * k, A) or dcontent.shape[0] != M or dcontent.shape[1] < 2 * D:
        raise ValueError('intent_fuse_bwd: operand shapes')
    dev = intents.device
    d_int, d_hid = torch.empty_like(intents), torch.empty_like(att_hidden)
    da_t, da_b = torch.empty(A, dtype=torch.float32, device=dev), torch.empty(A, dtype=torch.float32, device=dev)
    ws = _workspace(dev, lib.lime_intent_fuse_bwd_workspace(M, A))
    check(lib.lime_intent_fuse_bwd_f32(_p(intents), _p(att_hidden), _p(_vec(affine2_t, 'affine2_t', A)), _p(_vec(affine2_b, 'affine2_b', A)),
                                       _p(dcontent), _ld(dcontent), _p(d_int), _p(d_hid), _p(da_t), _p(da_b), M, k, D, A, _p(ws),
                                       ws.numel(), _stream()), 'lime_intent_fuse_bwd_f32')
    return d_int, d_hid, da_t, da_b


def gate_ln_bwd(y, x, scale, bias, gamma, beta, eps, dout):
    """-> (dy, dx, dscale [rows], dbias, dgamma, dbeta) of ``gate_ln``; y / x / dout: contiguous [rows, D]."""
    lib = _lib.load()
    D = x.shape[-1]
    x = _vec(x.contiguous(), 'x')
    rows = x.numel() // D
    y = _vec(y.contiguous(), 'y', x.numel())
    dout = _vec(dout.contiguous(), 'dout', x.numel())
    dev = x.device
    dy, dx = torch.empty_like(x), torch.empty_like(x)
    dscale = torch.empty(rows, dtype=torch.float32, device=dev)
    dbias, dgamma, dbeta = (torch.empty(D, dtype=torch.float32, device=dev) for _ in range(3))
    ws = _workspace(dev, lib.lime_gate_ln_bwd_workspace(rows, D))
    check(lib.lime_gate_ln_bwd_f32(_p(y), _p(x), _p(_vec(scale.contiguous(), 'scale', rows)), _p(_vec(bias, 'bias', D)),
                                   _p(_vec(gamma, 'gamma', D)), _p(_vec(beta, 'beta', D)), eps, _p(dout), _p(dy), _p(dx), _p(dscale),
                                   _p(dbias), _p(dgamma), _p(dbeta), rows, D, _p(ws), ws.numel(), _stream()), 'lime_gate_ln_bwd_f32')
    return dy, dx, dscale, dbias, dgamma, dbeta


def interest_match_bwd(kp, qp, g, cand, remaining, dlogits, B, N, H, A, D, scale, alpha, beta, use_weight, use_penalty):
    """-> (dkp [B*H, A], dqp [B*N, A], dg [B*H, D], dcand [B*N, D])."""
    lib = _lib.load()
    _vec(kp, 'kp', B * H * A)
    _vec(qp, 'qp', B * N * A)
    _vec(g, 'g', B * H * D)
    _vec(cand, 'cand', B * N * D)
    dlogits = _vec(dlogits.contiguous(), 'dlogits', B * N)
    if use_weight:
        remaining = _vec(remaining.contiguous(), 'remaining', B * N)
    dev = kp.device
    dkp = torch.empty((B * H, A), dtype=torch.float32, device=dev)
    dqp = torch.empty((B * N, A), dtype=torch.float32, device=dev)
    dg = torch.empty((B * H, D), dtype=torch.float32, device=dev)
    dcand = torch.empty((B * N, D), dtype=torch.float32, device=dev)
    ws = _workspace(dev, lib.lime_interest_match_bwd_workspace(B, N, H, A, D))
    check(lib.lime_interest_match_bwd_f32(_p(kp), _p(qp), _p(g), _p(cand), _p(remaining) if use_weight else None, _p(dlogits), _p(dkp),
                                          _p(dqp), _p(dg), _p(dcand), B, N, H, A, D, scale, alpha, beta, int(use_weight),
                                          int(use_penalty), _p(ws), ws.numel(), _stream()), 'lime_interest_match_bwd_f32')
    return dkp, dqp, dg, dcand


def cand_attn_weights_train(qp, kp, mask, B, N, H, D, n_head, p=0.0, seed=0, site=0):
    """agg [B, H] of layers.py:66-81 with the training-mode dropout on the per-head probabilities."""
    lib = _lib.load()
    _vec(qp, 'qp', B * N * D)
    _vec(kp, 'kp', B * H * D)
    m = _mask_u8(mask, 'mask')
    if m.numel() != B * H:
        raise ValueError('mask must be [B, H]')
    agg = torch.empty((B, H), dtype=torch.float32, device=qp.device)
    check(lib.lime_cand_attn_weights_train_f32(_p(qp), _p(kp), _p(m), _p(agg), B, N, H, D, n_head, p, seed, site, _stream()),
          'lime_cand_attn_weights_train_f32')
    return agg


def cand_attn_weights_bwd(qp, kp, mask, dagg, B, N, H, D, n_head, p=0.0, seed=0, site=0):
    """-> (dqp [B*N, D], dkp [B*H, D])."""
    lib = _lib.load()
    _vec(qp, 'qp', B * N * D)
    _vec(kp, 'kp', B * H * D)
    m = _mask_u8(mask, 'mask')
    dagg = _vec(dagg.contiguous(), 'dagg', B * H)
    dqp = torch.empty((B * N, D), dtype=torch.float32, device=qp.device)
    dkp = torch.empty((B * H, D), dtype=torch.float32, device=qp.device)
    check(lib.lime_cand_attn_weights_bwd_f32(_p(qp), _p(kp), _p(m), _p(dagg), _p(dqp), _p(dkp), B, N, H, D, n_head, p, seed, site, _stream()),
          'lime_cand_attn_weights_bwd_f32')
    return dqp, dkp


def conv1d_pack(weight):
    """nn.Conv1d weight [O, C, window] -> the [O, window * C] operand of ``conv1d_window`` (row o = taps j, each C wide)."""
    O, C, win = weight.shape
    return weight.permute(0, 2, 1).reshape(O, win * C).contiguous()


def conv1d_pack_dgrad(weight):
    """nn.Conv1d weight [O, C, window] -> the [C, window * O] operand of the data gradient (taps reversed):
    wd[c, j * O + o] = weight[o, c, window - 1 - j]."""
    O, C, win = weight.shape
    return weight.flip(2).permute(1, 2, 0).reshape(C, win * O).contiguous()


def conv1d_window(a, w, window, T, ids=None, bias=None, act=None, out=None, accumulate=False, m_dev=None):
    """out[r, o] (+)= act(bias[o] + sum_j A(r, j) . w[o, j C : (j + 1) C]) -- see ``lime_conv1d_window_f32``.

    a: [rows, C] dense source rows (ids None, rows = M) or the [V, C] table the int32 ``ids`` [M] gather from; w: [N, window * C]
    (``conv1d_pack``); M = sequences x T; out: [M, N] (may be a column slice of a wider output).  Out-of-sequence taps read zeros.
    m_dev: int32 device tensor (1 element): rows >= min(m_dev, M) are neither computed nor written."""
    lib = _lib.load()
    _mat(a, 'a')
    _mat(w, 'w')
    C = a.shape[1]
    N = w.shape[0]
    if window <= 0 or window % 2 == 0:
        raise ValueError('conv1d_window: window must be odd and positive (got %d)' % window)
    if w.shape[1] != window * C:
        raise ValueError('w must be [N, window * C] = [%d, %d], got %s' % (N, window * C, tuple(w.shape)))
    if ids is not None:
        _vec(ids, 'ids', dtype=torch.int32)
        M = ids.numel()
    else:
        M = a.shape[0]
    if T <= 0 or M % T:
        raise ValueError('conv1d_window: M = %d rows is not a whole number of sequences of T = %d' % (M, T))
    if out is None:
        if accumulate:
            raise ValueError('accumulate needs out')
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _mat(out, 'out')
    if tuple(out.shape) != (M, N):
        raise ValueError('out must be [%d, %d], got %s' % (M, N, tuple(out.shape)))
    if C % 4 or _ld(a) % 4 or _ld(w) % 4 or a.data_ptr() % 16 or w.data_ptr() % 16:
        raise ValueError('conv1d_window: the source width, the leading dimensions of a and w must be multiples of 4 and a, w 16-byte '
                         'aligned (C = %d)' % C)
    if act not in (None, 'none', 'relu'):
        raise ValueError('conv1d_window: act must be None or relu')
    if m_dev is not None:
        _vec(m_dev, 'm_dev', 1, dtype=torch.int32)
    if M == 0:
        return out
    check(lib.lime_conv1d_window_f32(_p(a), _ld(a), _p(ids), _p(w), _ld(w), _p(_vec(bias, 'bias', N)), _p(out), _ld(out), M, N, C, T,
                                     window, LIME_ACT[act], 1 if accumulate else 0, _p(m_dev), _stream()), 'lime_conv1d_window_f32')
    return out


def conv1d_window_wgrad(dy, a, window, T, ids=None, out=None, accumulate=False):
    """dW [N, window * C] (+)= sum_r dy[r, :]^T A(r, j) -- the weight gradient of ``conv1d_window`` in its packed layout
    (``lime_conv1d_wgrad_f32``: fixed-order partial sums, bitwise reproducible).  dy [M, N]; a / ids as in conv1d_window."""
    lib = _lib.load()
    _mat(dy, 'dy')
    _mat(a, 'a')
    M, N = dy.shape
    C = a.shape[1]
    if window <= 0 or window % 2 == 0:
        raise ValueError('conv1d_window_wgrad: window must be odd and positive (got %d)' % window)
    if ids is not None:
        _vec(ids, 'ids', M, dtype=torch.int32)
    elif a.shape[0] != M:
        raise ValueError('dy has %d rows, a has %d' % (M, a.shape[0]))
    if T <= 0 or M % T:
        raise ValueError('conv1d_window_wgrad: M = %d rows is not a whole number of sequences of T = %d' % (M, T))
    if out is None:
        if accumulate:
            raise ValueError('accumulate needs out')
        out = torch.empty((N, window * C), dtype=torch.float32, device=dy.device)
    _mat(out, 'out')
    if tuple(out.shape) != (N, window * C):
        raise ValueError('out must be [%d, %d]' % (N, window * C))
    if N % 4 or C % 4 or _ld(dy) % 4 or _ld(a) % 4 or dy.data_ptr() % 16 or a.data_ptr() % 16:
        raise ValueError('conv1d_window_wgrad: N, C and the leading dimensions must be multiples of 4, dy and a 16-byte aligned')
    if M == 0:
        return out if accumulate else out.zero_()
    ws = _workspace(dy.device, lib.lime_conv1d_wgrad_workspace(M, N, C, window))
    check(lib.lime_conv1d_wgrad_f32(_p(dy), _ld(dy), _p(a), _ld(a), _p(ids), _p(out), _ld(out), M, N, C, T, window,
                                    1 if accumulate else 0, _p(ws), ws.numel(), _stream()), 'lime_conv1d_wgrad_f32')
    return out


CONV_POOL_T_MAX = 128            # the fused conv + pool kernel's limit: a 128-row tile holds whole sequences (csrc/conv_pool_sp_f32.hip)
# Measured on MI355X (tools/bench_kcnn.py --part kernel, DESIGN.md "KCNN content encoder"; interleaved, medians of 15 rounds): three
# sources of 300 columns -> 400, window 3, at 1760 x 32 tokens the fused launch takes 0.971 ms against 1.053 ms for conv1d_window per
# source + relu_maxpool, at 8192 x 32 (one pass of the content cache) 4.325 against 4.774 ms.  So ``conv_pool`` takes the fused kernel
# wherever it applies (T <= 128) unless asked for the other form (fused=False, or LIME_FUSED_CONV_POOL=0 for the whole process).
FUSED_CONV_POOL = os.environ.get('LIME_FUSED_CONV_POOL', '1') == '1'


def conv_pool_pack(weight):
    """nn.Conv2d weight [O, C, window, n_src] -> the [O, n_src * window * C] operand of ``conv_pool``: column (src * window + j) * C + c."""
    O, C, win, n_src = weight.shape
    return weight.permute(0, 3, 2, 1).reshape(O, n_src * win * C).contiguous()


def _pool_outputs(n_seq, N, device, out, arg, want_arg):
    if out is None:
        out = torch.empty((n_seq, N), dtype=torch.float32, device=device)
    _mat(out, 'out')
    if tuple(out.shape) != (n_seq, N):
        raise ValueError('out must be [%d, %d], got %s' % (n_seq, N, tuple(out.shape)))
    if arg is None and want_arg:
        arg = torch.empty((n_seq, N), dtype=torch.int32, device=device)
    if arg is not None:
        _mat(arg, 'arg', dtype=torch.int32)
        if tuple(arg.shape) != (n_seq, N):
            raise ValueError('arg must be [%d, %d], got %s' % (n_seq, N, tuple(arg.shape)))
    return out, arg


def relu_maxpool(pre, n_seq, T, P, bias=None, out=None, arg=None, want_arg=False, n_seq_dev=None):
    """pooled[s, o] = max(0, max_{t < P} pre[s T + t, o] + bias[o]) and (``want_arg`` / ``arg``) the smallest t attaining it, -1 where
    the pooled value is 0 -- ``lime_relu_maxpool_f32``.  pre [n_seq * T, N] (may be a column slice).  -> out, or (out, arg)."""
    lib = _lib.load()
    _mat(pre, 'pre')
    N = pre.shape[1]
    if pre.shape[0] != n_seq * T:
        raise ValueError('pre has %d rows, expected n_seq * T = %d' % (pre.shape[0], n_seq * T))
    if not 1 <= P <= T:
        raise ValueError('relu_maxpool: P = %d outside 1 .. T = %d' % (P, T))
    out, arg = _pool_outputs(n_seq, N, pre.device, out, arg, want_arg)
    if N % 4 or _ld(pre) % 4 or _ld(out) % 4 or pre.data_ptr() % 16 or out.data_ptr() % 16:
        raise ValueError('relu_maxpool: N and the leading dimensions must be multiples of 4, pre and out 16-byte aligned')
    if n_seq_dev is not None:
        _vec(n_seq_dev, 'n_seq_dev', 1, dtype=torch.int32)
    if n_seq > 0:
        check(lib.lime_relu_maxpool_f32(_p(pre), _ld(pre), _p(_vec(bias, 'bias', N)), _p(out), _ld(out), _p(arg), 0 if arg is None else _ld(arg),
                                        n_seq, T, P, N, _p(n_seq_dev), _stream()), 'lime_relu_maxpool_f32')
    return out if arg is None else (out, arg)


def relu_maxpool_bwd(dpooled, arg, T, out=None):
    """dpre [n_seq * T, N]: dpooled[s, o] at row s T + arg[s, o] where arg >= 0, zeros everywhere else; every element is written
    (``lime_relu_maxpool_bwd_f32``: no atomics, no pre-zeroing)."""
    lib = _lib.load()
    _mat(dpooled, 'dpooled')
    _mat(arg, 'arg', dtype=torch.int32)
    n_seq, N = dpooled.shape
    if tuple(arg.shape) != (n_seq, N):
        raise ValueError('arg must be [%d, %d], got %s' % (n_seq, N, tuple(arg.shape)))
    if T <= 0:
        raise ValueError('relu_maxpool_bwd: T must be positive')
    if out is None:
        out = torch.empty((n_seq * T, N), dtype=torch.float32, device=dpooled.device)
    _mat(out, 'out')
    if tuple(out.shape) != (n_seq * T, N):
        raise ValueError('out must be [%d, %d], got %s' % (n_seq * T, N, tuple(out.shape)))
    if N % 4 or _ld(dpooled) % 4 or _ld(out) % 4 or dpooled.data_ptr() % 16 or out.data_ptr() % 16:
        raise ValueError('relu_maxpool_bwd: N and the leading dimensions must be multiples of 4, dpooled and out 16-byte aligned')
    if n_seq > 0:
        check(lib.lime_relu_maxpool_bwd_f32(_p(dpooled), _ld(dpooled), _p(arg), _ld(arg), _p(out), _ld(out), n_seq, T, N, _stream()),
              'lime_relu_maxpool_bwd_f32')
    return out


def conv_pool_odd_window(window, pad):
    """(window', shift): the odd window with pad' = (window' - 1) / 2 that holds the taps of (window, pad) behind ``shift`` zero taps --
    how ``conv1d_window`` and its gradients express the even windows (2, 0) and (4, 1) of Conv2D_Pool."""
    shift = max(0, window - 1 - 2 * pad)                  # zero taps in front: pad' - pad with window' = window + shift
    wodd = window + shift
    if wodd % 2 == 0 or (wodd - 1) // 2 != pad + shift:
        raise ValueError('conv_pool: (window, pad) = (%d, %d) is not an odd centred window behind zero first taps' % (window, pad))
    return wodd, shift


def conv_pool_unfused_weights(w, n_src, window, pad, C):
    """The packed [N, n_src * window * C] weight of ``conv_pool`` -> per source the [N, window' * C] operand of ``conv1d_window``
    (``conv_pool_odd_window``: zero first taps for an even window)."""
    wodd, shift = conv_pool_odd_window(window, pad)
    N = w.shape[0]
    w4 = w.view(N, n_src, window, C)
    if shift == 0:
        return [w4[:, s].reshape(N, window * C) for s in range(n_src)], wodd
    out = w.new_zeros((n_src, N, wodd, C))
    out[:, :, shift:] = w4.permute(1, 0, 2, 3)
    return [out[s].view(N, wodd * C) for s in range(n_src)], wodd


def conv_pool(sources, w, window, pad, P, T, bias=None, out=None, arg=None, want_arg=False, n_seq_dev=None, fused=None):
    """pooled[s, o] = max(0, max_{t < P} (bias[o] + sum_src sum_{j < window} X_src(s T + t + j - pad) . w[o, (src window + j) C : + C])),
    optionally with the position ``arg`` [n_seq, N] int32 of the maximum (-1 where pooled is 0): the KCNN convolution + ReLU + max pool.

    sources: 1 to 3 pairs (a, ids): a [rows, C] dense rows (ids None) or the [V, C] table that the int32 ``ids`` [n_seq * T] gather from.
    w: [N, n_src * window * C] (``conv_pool_pack``).  out may be a column slice of a wider output.  n_seq_dev: int32 device tensor (1
    element): sequences >= min(n_seq_dev, n_seq) are neither computed nor written.
    fused True: ``lime_conv_pool_f32``, one launch, T <= 128.  False: per source ``conv1d_window`` (accumulate) into a dense
    [n_seq * T, N] pre-activation, then ``relu_maxpool`` -- the fallback for longer sequences and the A/B partner.  None: FUSED_CONV_POOL
    where the fused kernel applies."""
    lib = _lib.load()
    if not 1 <= len(sources) <= 3:
        raise ValueError('conv_pool takes 1 to 3 sources, got %d' % len(sources))
    _mat(w, 'w')
    N = w.shape[0]
    C = sources[0][0].shape[1] if isinstance(sources[0][0], torch.Tensor) and sources[0][0].dim() == 2 else 0
    M = None
    for a, ids in sources:
        _mat(a, 'a')
        if a.shape[1] != C:
            raise ValueError('conv_pool: every source must be %d wide, got %d' % (C, a.shape[1]))
        if ids is not None:
            _vec(ids, 'ids', dtype=torch.int32)
        m = a.shape[0] if ids is None else ids.numel()
        if M is not None and m != M:
            raise ValueError('conv_pool: the sources have %d and %d rows' % (M, m))
        M = m
        if C % 4 or _ld(a) % 4 or a.data_ptr() % 16:
            raise ValueError('conv_pool: the source width and leading dimensions must be multiples of 4 and the sources 16-byte aligned')
    n_src = len(sources)
    if T <= 0 or M % T:
        raise ValueError('conv_pool: %d rows is not a whole number of sequences of T = %d' % (M, T))
    n_seq = M // T
    if not (1 <= window <= T and 0 <= pad < window and 1 <= P <= T):
        raise ValueError('conv_pool: window %d, pad %d, P %d outside what T = %d allows' % (window, pad, P, T))
    if w.shape[1] != n_src * window * C:
        raise ValueError('w must be [N, n_src * window * C] = [%d, %d], got %s' % (N, n_src * window * C, tuple(w.shape)))
    if N % 4 or _ld(w) % 4 or w.data_ptr() % 16:
        raise ValueError('conv_pool: N and the leading dimension of w must be multiples of 4 and w 16-byte aligned')
    out, arg = _pool_outputs(n_seq, N, w.device, out, arg, want_arg)
    bias = _vec(bias, 'bias', N)
    if n_seq_dev is not None:
        _vec(n_seq_dev, 'n_seq_dev', 1, dtype=torch.int32)
    if fused is None:
        fused = FUSED_CONV_POOL and T <= CONV_POOL_T_MAX
    if n_seq == 0:
        return out if arg is None else (out, arg)
    if fused:
        if T > CONV_POOL_T_MAX:
            raise ValueError('conv_pool: the fused kernel holds whole sequences in a tile, T = %d > %d (use fused=False)' % (T, CONV_POOL_T_MAX))
        a = _lib.ConvPoolArgs()
        for s, (src, ids) in enumerate(sources):
            a.a[s], a.lda[s], a.ids[s] = src.data_ptr(), _ld(src), (None if ids is None else ids.data_ptr())
        a.w, a.ldw, a.bias = w.data_ptr(), _ld(w), (None if bias is None else bias.data_ptr())
        a.pooled, a.ldp = out.data_ptr(), _ld(out)
        a.arg, a.ldarg = (None, 0) if arg is None else (arg.data_ptr(), _ld(arg))
        a.n_seq_dev = None if n_seq_dev is None else n_seq_dev.data_ptr()
        a.n_seq, a.T, a.N, a.C, a.n_src, a.window, a.pad, a.P = n_seq, T, N, C, n_src, window, pad, P
        check(lib.lime_conv_pool_f32(ctypes.byref(a), _stream()), 'lime_conv_pool_f32')
        return out if arg is None else (out, arg)
    ws, wodd = conv_pool_unfused_weights(w, n_src, window, pad, C)
    pre = torch.empty((M, N), dtype=torch.float32, device=w.device)
    m_dev = None if n_seq_dev is None else n_seq_dev * T
    for s, (src, ids) in enumerate(sources):
        conv1d_window(src, ws[s], wodd, T, ids=ids, out=pre, accumulate=s > 0, m_dev=m_dev)
    relu_maxpool(pre, n_seq, T, P, bias=bias, out=out, arg=arg, n_seq_dev=n_seq_dev)
    return out if arg is None else (out, arg)


ATTN_POOL_T_MAX, ATTN_POOL_A_MAX = 128, 512       # the fused attention pool's limits (csrc/attn_pool_sp_f32.hip)
# Measured on MI355X (tools/bench_naml.py --part pool, DESIGN.md "NAML content encoder"): at 1760 x 32, 1760 x 128 and 1760 x 4 rows
# (D = A = 400) the fused launch takes 1.38x, 1.37x and 2.2x the time of linear(tanh) + additive_pool, so ``attn_pool`` keeps the two
# launches unless asked for the fused one (fused=True, or LIME_FUSED_ATTN_POOL=1 for the whole process).
FUSED_ATTN_POOL = os.environ.get('LIME_FUSED_ATTN_POOL', '0') == '1'


def attn_pool_pack(w1):
    """``lime_attn_pool_pack_sp``: Attention.affine1's weight (fp32 [A, D]) -> the split (three bf16 terms) operand of ``attn_pool``.
    Runs on the stream like any launch: called inside a forward, a captured graph repacks on every replay."""
    lib = _lib.load()
    _mat(w1, 'w1')
    A, D = w1.shape
    n = int(lib.lime_attn_pool_pack_sp_size(D, A))
    if n <= 0:
        raise ValueError('attn_pool_pack: built for D %% 4 == 0 and A <= %d (w1 is %s)' % (ATTN_POOL_A_MAX, tuple(w1.shape)))
    w1p = torch.empty(n, dtype=torch.bfloat16, device=w1.device)
    check(lib.lime_attn_pool_pack_sp(_p(w1), _ld(w1), D, A, _p(w1p), _stream()), 'lime_attn_pool_pack_sp')
    return w1p


def attn_pool_fused(D, A, T, fused=None):
    """True when ``attn_pool(..., fused=fused)`` runs the one-launch kernel for these dimensions (else linear(tanh) + additive_pool).
    Depends on the dimensions and the switch only, never on the sequence count."""
    want = FUSED_ATTN_POOL if fused is None else fused
    return bool(want) and 0 < T <= ATTN_POOL_T_MAX and D % 4 == 0 and 0 < A <= ATTN_POOL_A_MAX


def attn_pool(x, w1, b1, w2, n_seq, T, mask=None, out=None, n_seq_dev=None, w1p=None, fused=None, m_dev=None):
    """layers.Attention (layers.py:285-300) over n_seq sequences of T rows of x [n_seq * T, D]:
    out[s] = sum_t softmax_t(w2 . tanh(w1 x[s T + t] + b1)) x[s T + t] -> [n_seq, D] (``out`` may be a row-strided view, e.g. one slot
    of a [M, 4, D] stack).  mask: optional bool / uint8 [n_seq * T] (0: the key scores -1e9).  n_seq_dev: int32 device tensor
    (1 element): only that many sequences are read and written.

    One launch (``lime_attn_pool_sp_f32``, the hidden state stays in registers) when ``attn_pool_fused(D, A, T, fused)``; w1p is the
    packed w1 (``attn_pool_pack``; packed here when not given).  Otherwise ``linear(act='tanh')`` + ``additive_pool``; m_dev (int32
    device tensor, 1 element, = n_seq_dev * T) then bounds the rows of the linear launch."""
    lib = _lib.load()
    _mat(x, 'x')
    _mat(w1, 'w1')
    D = x.shape[1]
    A = w1.shape[0]
    if w1.shape[1] != D:
        raise ValueError('w1 must be [A, %d], got %s' % (D, tuple(w1.shape)))
    if T <= 0 or n_seq < 0 or x.shape[0] != n_seq * T:
        raise ValueError('x must have n_seq * T rows (n_seq = %d, T = %d, x has %d)' % (n_seq, T, x.shape[0]))
    _vec(w2, 'w2', A)
    _vec(b1, 'b1', A)
    if out is None:
        out = torch.empty((n_seq, D), dtype=torch.float32, device=x.device)
    _mat(out, 'out')
    if tuple(out.shape) != (n_seq, D):
        raise ValueError('out must be [%d, %d], got %s' % (n_seq, D, tuple(out.shape)))
    m = _mask_u8(mask, 'mask')
    if m is not None and m.numel() != n_seq * T:
        raise ValueError('mask must have n_seq * T elements')
    if n_seq_dev is not None:
        _vec(n_seq_dev, 'n_seq_dev', 1, dtype=torch.int32)
    if not attn_pool_fused(D, A, T, fused):
        hidden = linear(x, w1, b1, act='tanh', m_dev=m_dev)
        return additive_pool(hidden, w2, x, n_seq, T, mask=m, out=out, n_seq_dev=n_seq_dev)
    if _ld(x) % 4 or x.data_ptr() % 16 or _ld(out) % 4 or out.data_ptr() % 16:
        raise ValueError('attn_pool: x and out must be 16-byte aligned with leading dimensions that are multiples of 4')
    if w1p is None:
        w1p = attn_pool_pack(w1)
    elif w1p.dtype != torch.bfloat16 or not w1p.is_contiguous() or w1p.numel() != int(lib.lime_attn_pool_pack_sp_size(D, A)):
        raise ValueError('w1p must be the buffer of attn_pool_pack for w1 [%d, %d]' % (A, D))
    if n_seq == 0:
        return out
    check(lib.lime_attn_pool_sp_f32(_p(x), _ld(x), D, _p(w1p), _p(b1), _p(w2), A, _p(m), _p(out), _ld(out), n_seq, T, _p(n_seq_dev),
                                    _stream()), 'lime_attn_pool_sp_f32')
    return out


# ---- device-side dev / test pass: ranks + AUC / MRR / nDCG per impression (csrc/rank_metrics.hip) -----------------------------------
class RankMetrics:
    """Result of ``rank_metrics``: ``ranks`` int32 [R] (1-based inside the impression), ``per_impression`` fp64 [n_imp, 4] (AUC, MRR,
    nDCG@5, nDCG@10; zeros unless status is 0), ``status`` int32 [n_imp] (0 counted, 1 skipped or no rows, 2 one class only, 3 a label
    outside {0, 1} or a NaN score), ``sums`` fp64 [4] and ``count`` int64 [1] over the status == 0 impressions -- all device tensors."""
    __slots__ = ('ranks', 'per_impression', 'status', 'sums', 'count')

    def __init__(self, ranks, per_impression, status, sums, count):
        self.ranks, self.per_impression, self.status, self.sums, self.count = ranks, per_impression, status, sums, count

    def means(self):
        """(AUC, MRR, nDCG@5, nDCG@10) over the counted impressions as Python floats (one device -> host copy)."""
        s, c = self.sums.cpu().numpy(), int(self.count.cpu()[0])
        return tuple(float(v) for v in (s / c if c else s * float('nan')))


_DISC = {}


def _ndcg_discounts(device):
    """1 / log2(p + 2), p = 0..9, with numpy's bits (evaluate.dcg_score divides by np.log2)."""
    key = str(device)
    if key not in _DISC:
        import numpy as np
        _DISC[key] = torch.from_numpy(1.0 / np.log2(np.arange(10) + 2.0)).to(device)
    return _DISC[key]


def check_offsets(offsets, R):
    """``offsets`` of ``rank_metrics`` as a host int32 array after the checks a launch relies on: 1-D, at least one entry, starts at
    0, non-decreasing, ends at R.  Raises ValueError; no device work."""
    import numpy as np
    o = np.asarray(offsets.cpu() if isinstance(offsets, torch.Tensor) else offsets)
    if o.ndim != 1 or o.size < 1 or o.dtype.kind not in 'iu':
        raise ValueError('offsets must be a 1-D integer array of n_imp + 1 entries')
    o = o.astype(np.int64)
    if o[0] != 0 or o[-1] != R:
        raise ValueError('offsets must start at 0 and end at the row count %d, got %d .. %d' % (R, o[0], o[-1]))
    if o.size > 1 and (np.diff(o) < 0).any():
        raise ValueError('offsets must be non-decreasing (the rows of an impression are contiguous): first decrease at entry %d'
                         % (int(np.argmax(np.diff(o) < 0)) + 1))
    if R > 2 ** 31 - 1:
        raise ValueError('rank_metrics takes up to 2^31 - 1 rows')
    return o.astype(np.int32)


def rank_metrics(scores, labels, offsets, skip=None, rank_blocks=0, reduce_blocks=0):
    """``lime_rank_metrics``: the dev / test pass behind the scores in one call.  scores fp32 [R], labels uint8 [R] (0 / 1) and the
    optional skip uint8 / bool [n_imp] are CUDA tensors; ``offsets`` (n_imp + 1 entries, rows offsets[i] .. offsets[i + 1] - 1 are
    impression i) is a host array / list / CPU tensor, checked on the host and copied, or an int32 CUDA tensor, whose check costs one
    device -> host copy.  Returns a ``RankMetrics``.  ``rank_blocks`` / ``reduce_blocks``: workgroup counts of the rank launch and of
    the first reduction level (0: default); the result does not depend on them."""
    if not isinstance(scores, torch.Tensor) or not isinstance(labels, torch.Tensor):
        raise TypeError('scores and labels must be CUDA tensors (the HIP path has no CPU fallback)')
    R = scores.numel()
    off_host = check_offsets(offsets, R)                    # ValueError before anything touches the device
    n_imp = off_host.size - 1
    if not scores.is_cuda or not labels.is_cuda or (isinstance(skip, torch.Tensor) and not skip.is_cuda):
        raise TypeError('scores, labels and skip must be CUDA tensors (the HIP path has no CPU fallback)')
    _vec(scores, 'scores')
    _vec(labels, 'labels', R, dtype=torch.uint8)
    if scores.dim() != 1:
        raise ValueError('scores must be 1-D')
    if isinstance(offsets, torch.Tensor) and offsets.is_cuda:
        if offsets.dtype != torch.int32 or not offsets.is_contiguous():
            raise TypeError('a CUDA offsets tensor must be contiguous int32')
        off = offsets
    else:
        off = torch.from_numpy(off_host).to(scores.device)
    sk = None
    if skip is not None:
        if not isinstance(skip, torch.Tensor):
            raise TypeError('skip must be a CUDA uint8 / bool tensor')
        sk = _mask_u8(skip, 'skip')
        if sk.numel() != n_imp:
            raise ValueError('skip must have one entry per impression (%d), got %d' % (n_imp, sk.numel()))
    if rank_blocks < 0 or reduce_blocks < 0:
        raise ValueError('rank_blocks and reduce_blocks must be >= 0')
    lib = _lib.load()
    dev = scores.device
    ranks = torch.empty(R, dtype=torch.int32, device=dev)
    per_imp = torch.empty((n_imp, 4), dtype=torch.float64, device=dev)
    status = torch.empty(n_imp, dtype=torch.int32, device=dev)
    sums = torch.empty(4, dtype=torch.float64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ws_bytes = int(lib.lime_rank_metrics_workspace(n_imp))
    ws = torch.empty(max(1, (ws_bytes + 7) // 8), dtype=torch.float64, device=dev)
    disc = _ndcg_discounts(dev)
    a = _lib.RankMetricsArgs()
    a.scores, a.labels, a.offsets, a.skip, a.disc = scores.data_ptr(), labels.data_ptr(), off.data_ptr(), (sk.data_ptr() if sk is not None else None), disc.data_ptr()
    a.ranks, a.per_imp, a.status, a.sums, a.count = ranks.data_ptr(), per_imp.data_ptr(), status.data_ptr(), sums.data_ptr(), count.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 8
    a.R, a.n_imp, a.rank_blocks, a.reduce_blocks, a.reserved = R, n_imp, int(rank_blocks), int(reduce_blocks), 0
    check(lib.lime_rank_metrics(ctypes.byref(a), _stream()), 'lime_rank_metrics')
    return RankMetrics(ranks, per_imp, status, sums, count)


class SlateMetrics:
    """Result of ``slate_metrics``: ``per_slate`` fp64 [R, 8] (nDCG@k, RR@k, hit@k, recall@k, ILD, distinct keys, filled slots, mean
    value), ``status`` int32 [R] (0 counted, 1 skipped / no labels / no rows, 2 one class only, 3 a label outside {0, 1}), ``sums``
    fp64 [8] and ``counts`` int64 [3] (the slates behind the sums of columns 0-3, of column 4, of columns 5-7) -- all device tensors."""
    __slots__ = ('per_slate', 'status', 'sums', 'counts')

    def __init__(self, per_slate, status, sums, counts):
        self.per_slate, self.status, self.sums, self.counts = per_slate, status, sums, counts


_SLATE_DISC = {}


def _slate_discounts(device, k):
    """1 / log2(p + 2), p = 0 .. k - 1, with numpy's bits: the first k of one table of 128 per device."""
    key = str(device)
    if key not in _SLATE_DISC:
        import numpy as np
        _SLATE_DISC[key] = torch.from_numpy(1.0 / np.log2(np.arange(128) + 2.0)).to(device)
    return _SLATE_DISC[key][:k]


def slate_metrics(positions, k, offsets, news, labels=None, skip=None, value=None, table=None, keys=None, n=None, n_keys=None,
                  reduce_blocks=0):
    """``lime_slate_metrics_f32``: what the slates ``positions`` int32 [R, ldp] (device; unit column stride, a row-strided view is
    fine; the first k <= ldp slots count) are worth (``recommend.slate_metrics`` on the device).  ``offsets`` int64 [R + 1] (device):
    a position counts inside the slate's own list, rows offsets[r] .. offsets[r + 1] - 1 of news int32 [P] / labels uint8 [P] /
    value fp32 [P]; None: inside one pool of P rows.  skip uint8 / bool [R]; table fp32 [n, E] (a row-strided view is fine, E a
    multiple of 4); keys int32 [n] with 0 <= key < n_keys.  ``n`` defaults to the rows of table / keys.  Every check is made on the
    host before the launch (the offsets' VALUES are not read: the kernel clamps them into [0, P]).  Returns a ``SlateMetrics``.
    ``reduce_blocks``: workgroups of the sums' launch (0: default); no bit of the result depends on it."""
    if isinstance(positions, torch.Tensor) and positions.dim() == 2 and positions.shape[0] == 0:
        positions = positions.new_empty(positions.shape)           # (no slates: whatever strides the empty tensor carries)
    _mat(positions, 'positions', dtype=torch.int32)
    R, ldp = positions.shape
    k = int(k)
    if not 1 <= k <= min(ldp, 128):
        raise ValueError('slate_metrics needs 1 <= k <= min(ldp, 128) = %d, got k = %d' % (min(ldp, 128), k))
    P = _vec(news, 'news', dtype=torch.int32).numel()
    if offsets is None:
        if labels is not None:
            raise ValueError('labels need offsets: a pool has no impression to count the positives of')
    else:
        _vec(offsets, 'offsets', R + 1, dtype=torch.int64)
    _vec(labels, 'labels', P, dtype=torch.uint8)
    _vec(value, 'value', P)
    sk = None
    if skip is not None:
        sk = _vec(_mask_u8(skip, 'skip'), 'skip', R, dtype=torch.uint8)
    E = ld = 0
    if table is not None:
        _mat(table, 'table')
        E, ld = table.shape[1], _ld(table)
        if table.shape[0] < 1 or E < 1 or E % 4:
            raise ValueError('table must be [n, E] with n >= 1 and E a positive multiple of 4, got %s' % (tuple(table.shape),))
    if keys is not None:
        _vec(keys, 'keys', dtype=torch.int32)
        n_keys = 8192 if n_keys is None else int(n_keys)
        if n_keys < 1:
            raise ValueError('n_keys must be >= 1, got %d' % n_keys)
    rows = {t.shape[0] for t in (table, keys) if t is not None}
    if len(rows) > 1:
        raise ValueError('table and keys must have one row per news alike, got %d and %d' % (table.shape[0], keys.numel()))
    n = int(n) if n is not None else (rows.pop() if rows else 2 ** 31 - 1)
    if n < 1 or (rows and n > min(rows)):
        raise ValueError('n = %d must be in [1, the rows of table / keys]' % n)
    if reduce_blocks < 0:
        raise ValueError('reduce_blocks must be >= 0')
    for t, name in ((news, 'news'), (offsets, 'offsets'), (labels, 'labels'), (sk, 'skip'), (value, 'value'), (table, 'table'),
                    (keys, 'keys')):
        if t is not None and t.device != positions.device:
            raise ValueError('%s is on %s, positions on %s' % (name, t.device, positions.device))
    lib = _lib.load()
    dev = positions.device
    per_slate = torch.empty((R, 8), dtype=torch.float64, device=dev)
    status = torch.empty(R, dtype=torch.int32, device=dev)
    if R == 0:                                                    # (an empty tensor has no address to hand over)
        return SlateMetrics(per_slate, status, torch.zeros(8, dtype=torch.float64, device=dev), torch.zeros(3, dtype=torch.int64, device=dev))
    sums = torch.empty(8, dtype=torch.float64, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    disc = _slate_discounts(dev, k)
    ptr = lambda t: None if t is None else t.data_ptr()
    a = _lib.SlateMetricsArgs()
    a.positions, a.offsets, a.news, a.labels, a.skip = ptr(positions), ptr(offsets), ptr(news), ptr(labels), ptr(sk)
    a.value, a.table, a.keys, a.disc = ptr(value), ptr(table), ptr(keys), ptr(disc)
    a.per_slate, a.status, a.sums, a.counts = ptr(per_slate), ptr(status), ptr(sums), ptr(counts)
    a.R, a.P, a.ldp, a.ld, a.n = R, P, _ld(positions), ld, n
    a.k, a.E, a.n_keys, a.reduce_blocks, a.reserved = k, E, (n_keys if keys is not None else 0), int(reduce_blocks), 0
    check(lib.lime_slate_metrics_f32(ctypes.byref(a), _stream()), 'lime_slate_metrics_f32')
    return SlateMetrics(per_slate, status, sums, counts)


def slate_miscalibration(positions, k, offsets, news, keys, n_keys, hist_keys, hist_weight=None, alpha=0.01):
    """``lime_slate_miscalibration``: how far the topic mix of the slates ``positions`` int32 [R, ldp] (the first k <= ldp slots) is
    from their readers' (``recommend.slate_miscalibration`` on the device) -> (value fp64 [R], status int32 [R]: 0 defined, 1 no
    target, 2 no filled slot).  ``positions`` / ``offsets`` / ``news`` as in ``slate_metrics``; keys int32 [n] (n bounds the news ids
    too) with 0 <= key < ``n_keys`` <= 8192; hist_keys / hist_weight as in ``calibrate_rows``, slate r reading history row
    r % hist_rows.  ``alpha`` is read as the fp32 number ``calibrate_rows`` reads.  k <= 128, H <= 128."""
    if isinstance(positions, torch.Tensor) and positions.dim() == 2 and positions.shape[0] == 0:
        positions = positions.new_empty(positions.shape)           # (no slates: whatever strides the empty tensor carries)
    _mat(positions, 'positions', dtype=torch.int32)
    R, ldp = positions.shape
    k, alpha, n_keys = int(k), float(alpha), int(n_keys)
    if not 1 <= k <= min(ldp, 128) or not 0.0 < alpha < 1.0 or not 1 <= n_keys <= 8192:
        raise ValueError('slate_miscalibration needs 1 <= k <= min(ldp, 128) = %d, 0 < alpha < 1 and 1 <= n_keys <= 8192, got k = %d, '
                         'alpha = %r, n_keys = %d' % (min(ldp, 128), k, alpha, n_keys))
    P = _vec(news, 'news', dtype=torch.int32).numel()
    _vec(offsets, 'offsets', R + 1, dtype=torch.int64)
    n = _vec(keys, 'keys', dtype=torch.int32).numel()
    if n < 1:
        raise ValueError('keys must hold the group of at least one news')
    rows, H = _history(hist_keys, hist_weight, positions.device, 'slate_miscalibration')
    for t, name in ((news, 'news'), (offsets, 'offsets'), (keys, 'keys')):
        if t is not None and t.device != positions.device:
            raise ValueError('%s is on %s, positions on %s' % (name, t.device, positions.device))
    value = torch.empty(R, dtype=torch.float64, device=positions.device)
    status = torch.empty(R, dtype=torch.int32, device=positions.device)
    if R == 0:                                                    # (an empty tensor has no address to hand over)
        return value, status
    lib = _lib.load()                                             # (P = 0 or H = 0: an empty tensor has no address; nothing is read through it)
    check(lib.lime_slate_miscalibration(_p(positions), R, _ld(positions), k, _p(offsets), ctypes.c_void_p(news.data_ptr() or 16), P, _p(keys),
                                        n, n_keys, ctypes.c_void_p(hist_keys.data_ptr() or 16), _p(hist_weight) if H else None, rows, H,
                                        alpha, _p(value), _p(status), _stream()), 'lime_slate_miscalibration')
    return value, status


# ---- the epoch's negative sampling from the resident train tables (csrc/negative_sample.hip) --------------------------------------------
def negative_sample(offsets, neg_index, neg_lifetime, pos_index, pos_lifetime, freshness, K, seed, epoch, inclusive=False,
                    cand_index=None, cand_freshness=None, cand_lifetime=None):
    """``lime_negative_sample``: the candidate tables [N, 1 + K] (news index int32, freshness fp32, lifetime fp32) of one epoch from the
    CSR of every train record's non-clicked news -- offsets int64 [N + 1], neg_index int32 [nnz], neg_lifetime fp32 [nnz] -- and the
    per-record pos_index int32 [N], pos_lifetime fp32 [N], freshness fp32 [N]; all CUDA tensors.  Row i is a function of
    (seed, epoch, i) and the record (device_data.counter_negative_sampling is the same rule in NumPy).  The offsets are not checked (a
    check would cost a host synchronise; the kernel clamps them into [0, nnz]): DeviceBehaviors.train_resident checks them on the
    host, where it also refuses a record without non-clicked news.  With the three outputs given nothing is allocated.  Returns
    (cand_index, cand_freshness, cand_lifetime)."""
    lib = _lib.load()
    K, seed, epoch = int(K), int(seed), int(epoch)
    if not 1 <= K <= _lib.NEG_MAX_K:
        raise ValueError('negative_sample: K must be in [1, %d], got %d' % (_lib.NEG_MAX_K, K))
    if not 0 <= epoch < 2 ** 32 - 1 or not 0 <= seed < 2 ** 64:
        raise ValueError('negative_sample: seed must be in [0, 2^64) and epoch in [0, 2^32 - 1), got %d, %d' % (seed, epoch))
    N = _vec(pos_index, 'pos_index', dtype=torch.int32).numel()
    _vec(offsets, 'offsets', N + 1, dtype=torch.int64)
    nnz = _vec(neg_index, 'neg_index', dtype=torch.int32).numel()
    _vec(neg_lifetime, 'neg_lifetime', nnz)
    _vec(pos_lifetime, 'pos_lifetime', N)
    _vec(freshness, 'freshness', N)
    if nnz >= 2 ** 31:
        raise ValueError('negative_sample takes up to 2^31 - 1 non-clicked news in all')
    dev = pos_index.device
    if cand_index is None:
        cand_index = torch.empty((N, 1 + K), dtype=torch.int32, device=dev)
    if cand_freshness is None:
        cand_freshness = torch.empty((N, 1 + K), dtype=torch.float32, device=dev)
    if cand_lifetime is None:
        cand_lifetime = torch.empty((N, 1 + K), dtype=torch.float32, device=dev)
    for t, name, dt in ((cand_index, 'cand_index', torch.int32), (cand_freshness, 'cand_freshness', torch.float32),
                        (cand_lifetime, 'cand_lifetime', torch.float32)):
        _vec(t, name, N * (1 + K), dtype=dt)
        if tuple(t.shape) != (N, 1 + K):
            raise ValueError('negative_sample: %s must be [%d, %d], got %s' % (name, N, 1 + K, tuple(t.shape)))
    check(lib.lime_negative_sample(_p(offsets), _p(neg_index), _p(neg_lifetime), nnz, _p(pos_index), _p(pos_lifetime), _p(freshness),
                                   _p(cand_index), _p(cand_freshness), _p(cand_lifetime), N, K, seed, epoch, 1 if inclusive else 0,
                                   _stream()), 'lime_negative_sample')
    return cand_index, cand_freshness, cand_lifetime


# ---- CNE content encoder: bidirectional LSTM (csrc/lstm_f32.hip) ------------------------------------------------------------------

LSTM_UNIT_TILE = 16          # hidden sizes the step kernel is built for: multiples of this (a workgroup owns 16 units with their four gates)


def mask_lengths(mask, min_len=0, out=None):
    """``lime_mask_lengths``: int32 [R] = max(number of set entries of mask[r], min_len); mask bool / uint8 [R, T]."""
    lib = _lib.load()
    R, T = mask.shape
    m = _mask_u8(mask, 'mask')
    if out is None:
        out = torch.empty(R, dtype=torch.int32, device=mask.device)
    _vec(out, 'out', R, dtype=torch.int32)
    check(lib.lime_mask_lengths(_p(m), R, T, min_len, _p(out), _stream()), 'lime_mask_lengths')
    return out


def _lstm_dims(whh, lengths, T):
    _vec(whh, 'whh')
    if whh.dim() != 3 or whh.shape[0] != 2 or whh.shape[1] != 4 * whh.shape[2]:
        raise ValueError('whh must be [2, 4h, h] (weight_hh_l0 and weight_hh_l0_reverse stacked), got %s' % (tuple(whh.shape),))
    h = whh.shape[2]
    if h % LSTM_UNIT_TILE:
        raise ValueError('the LSTM step kernel needs a hidden size that is a multiple of %d, got %d' % (LSTM_UNIT_TILE, h))
    _vec(lengths, 'lengths', dtype=torch.int32)
    if T < 1:
        raise ValueError('T must be >= 1')
    return lengths.numel(), h


def lstm_step(gi, whh, lengths, hout, c, step, T, n_rows_dev=None, saved=None):
    """One time step of the bidirectional LSTM, both directions in one launch -- see ``lime_lstm_step_f32`` in include/lime_hip.h.
    gi [R T, 8h]; whh [2, 4h, h]; lengths int32 [R]; hout [R T, 2h] (zeroed once by the caller) and c [2, R, h] are updated in place.
    saved: (gates [R T, 8h], c_seq [R T, 2h], h_prev [R T, 2h]) to keep what the backward step needs."""
    lib = _lib.load()
    R, h = _lstm_dims(whh, lengths, T)
    _mat(gi, 'gi')
    _mat(hout, 'hout')
    if gi.shape[0] != R * T or gi.shape[1] != 8 * h or tuple(hout.shape) != (R * T, 2 * h) or not hout.is_contiguous():
        raise ValueError('gi must be [R T, 8h] and hout a contiguous [R T, 2h] (R = %d, T = %d, h = %d)' % (R, T, h))
    _vec(c, 'c', 2 * R * h)
    g = cs = hp = None
    if saved is not None:
        g, cs, hp = saved
        _vec(g, 'gates', R * T * 8 * h)
        _vec(cs, 'c_seq', R * T * 2 * h)
        _vec(hp, 'h_prev', R * T * 2 * h)
    if n_rows_dev is not None:
        _vec(n_rows_dev, 'n_rows_dev', 1, dtype=torch.int32)
    check(lib.lime_lstm_step_f32(_p(gi), _ld(gi), _p(whh), _p(lengths), _p(hout), _p(c), _p(g), _p(cs), _p(hp), R, T, h, step,
                                 _p(n_rows_dev), _stream()), 'lime_lstm_step_f32')


def lstm(gi, whh, lengths, T, n_rows_dev=None, save=False, hout=None, c=None):
    """The whole recurrence: T ``lstm_step`` launches in order (the time loop is on the host; a captured graph records them like any other
    launch).  Returns (hout [R T, 2h] with zeros behind every length, c [2, R, h] = c_n of both directions) and, with ``save``, the
    (gates, c_seq, h_prev) triple of ``lstm_bwd``.  hout / c may be passed in (hout zeroed by the caller)."""
    R, h = _lstm_dims(whh, lengths, T)
    if hout is None:
        hout = torch.zeros((R * T, 2 * h), dtype=torch.float32, device=gi.device)
    if c is None:
        c = torch.zeros((2, R, h), dtype=torch.float32, device=gi.device)
    saved = None
    if save:
        saved = (torch.zeros((R * T, 8 * h), dtype=torch.float32, device=gi.device),
                 torch.zeros((R * T, 2 * h), dtype=torch.float32, device=gi.device),
                 torch.zeros((R * T, 2 * h), dtype=torch.float32, device=gi.device))
    for s in range(T):
        lstm_step(gi, whh, lengths, hout, c, s, T, n_rows_dev=n_rows_dev, saved=saved)
    return (hout, c, saved) if save else (hout, c)


def lstm_bwd(dhout, dc_n, whh, lengths, T, saved, whh_t=None):
    """Backward of ``lstm``: steps T - 1 .. 0, each one gate-gradient launch (``lime_lstm_step_bwd_f32``) and -- but for step 0 -- one
    grouped GEMM of both directions carrying dh through W_hh.  dhout [R T, 2h] or None, dc_n [2, R, h] or None.  Returns
    dgi [R T, 8h] (zeros at padding tokens): the gradient of ``lstm``'s gi, from which the caller takes dW_ih, the bias gradients and
    the input rows with the existing GEMM nodes, and dW_hh = dgi[:, direction]^T h_prev[:, direction].  whh_t: [2, h, 4h], W_hh transposed."""
    lib = _lib.load()
    R, h = _lstm_dims(whh, lengths, T)
    gates, c_seq, _ = saved
    dev = whh.device
    if whh_t is None:
        whh_t = whh.transpose(1, 2).contiguous()
    dgi = torch.zeros((R * T, 8 * h), dtype=torch.float32, device=dev)
    dgs = torch.empty((2, R, 4 * h), dtype=torch.float32, device=dev)
    dh = torch.zeros((2, R, h), dtype=torch.float32, device=dev)
    dc = torch.zeros((2, R, h), dtype=torch.float32, device=dev) if dc_n is None else dc_n.contiguous().clone()
    lddh = 0
    if dhout is not None:
        _mat(dhout, 'dhout')
        if tuple(dhout.shape) != (R * T, 2 * h):
            raise ValueError('dhout must be [R T, 2h]')
        lddh = _ld(dhout)
    if R == 0:
        return dgi
    for s in range(T - 1, -1, -1):
        check(lib.lime_lstm_step_bwd_f32(_p(dhout), lddh, _p(gates), _p(c_seq), _p(lengths), _p(dh), _p(dc), _p(dgi), _p(dgs), R, T, h, s,
                                         _stream()), 'lime_lstm_step_bwd_f32')
        if s > 0:
            linear_group([dict(a=dgs[d], w=whh_t[d], out=dh[d]) for d in (0, 1)])
    return dgi


def gate_mul(x, g, div=1, scale=1.0, sigmoid=True, out=None, n_rows_dev=None):
    """``lime_gate_mul_f32`` on contiguous [rows, cols] operands: x * sigmoid(g) (g [rows, cols]), or with ``sigmoid`` off
    x[r] * g[r // div] * scale (g [rows / div, cols])."""
    lib = _lib.load()
    _mat(x, 'x')
    _mat(g, 'g')
    rows, cols = x.shape
    if not x.is_contiguous() or not g.is_contiguous() or g.shape[1] != cols or g.shape[0] * (1 if sigmoid else div) < rows or (sigmoid and div != 1):
        raise ValueError('gate_mul: x [rows, cols] and g [rows / div, cols] must be contiguous and agree')
    if out is None:
        out = torch.empty_like(x)
    if tuple(out.shape) != (rows, cols) or not out.is_contiguous():
        raise ValueError('gate_mul: out must be a contiguous [rows, cols]')
    if n_rows_dev is not None:
        _vec(n_rows_dev, 'n_rows_dev', 1, dtype=torch.int32)
    check(lib.lime_gate_mul_f32(_p(x), _p(g), _p(out), rows, cols, div, 0 if sigmoid else 1, scale, _p(n_rows_dev), _stream()), 'lime_gate_mul_f32')
    return out



# ---- CNE's per-news recurrence cache (csrc/seq_cache_f32.hip) -----------------------------------------------------------------------

def _packed_rows(lens, offsets, n):
    _vec(lens, 'lens', n, dtype=torch.int32)
    _vec(offsets, 'offsets', dtype=torch.int64)
    if offsets.numel() < (n if n is not None else lens.numel()):
        raise ValueError('offsets must hold a destination row for every entry of lens')


def seq_pack(src, lens, offsets, dst, S):
    """``lime_seq_pack_f32``: dst[offsets[i] + t] = src[i S + t] for t < lens[i].  src [n S, C] contiguous, lens int32 [n], offsets
    int64 [>= n] (destination rows), dst [rows, C] contiguous: the caller sizes it so that every offsets[i] + lens[i] fits."""
    lib = _lib.load()
    _mat(src, 'src')
    _mat(dst, 'dst')
    if S < 1:
        raise ValueError('S must be >= 1')
    n, C = lens.numel(), src.shape[1]
    _packed_rows(lens, offsets, n)
    if C % 4 or dst.shape[1] != C or src.shape[0] != n * S or not src.is_contiguous() or not dst.is_contiguous():
        raise ValueError('seq_pack: src must be a contiguous [n S, C] (n = %d, S = %d), dst a contiguous [rows, C], C a multiple of 4; got %s, %s'
                         % (n, S, tuple(src.shape), tuple(dst.shape)))
    check(lib.lime_seq_pack_f32(_p(src), _p(lens), _p(offsets), _p(dst), n, S, C, _stream()), 'lime_seq_pack_f32')
    return dst


def cne_gate_cached(h, hh, offsets, lens, idx, tm, S, out=None, n_rows_dev=None):
    """``lime_cne_gate_cached_f32``: out[r S + t] = h[offsets[j] + t] * sigmoid(hh[offsets[j] + t] + tm[r]) for t < lens[j], j = idx[r],
    zeros behind the length -- CNE's gated LSTM output of a batch from the packed per-news cache, one launch.  h, hh [rows, C]
    contiguous, offsets int64 [n + 1], lens int32 [n], idx int32 [cap] (news indices in [0, n): unchecked), tm [cap, C] contiguous
    -> out [cap S, C].  n_rows_dev (int32 device tensor, 1 element): only the first min(n_rows_dev, cap) slots are written."""
    lib = _lib.load()
    _mat(h, 'h')
    _mat(hh, 'hh')
    _mat(tm, 'tm')
    if S < 1:
        raise ValueError('S must be >= 1')
    _vec(idx, 'idx', dtype=torch.int32)
    cap, C = idx.numel(), h.shape[1]
    _packed_rows(lens, offsets, None)
    if C % 4 or tuple(hh.shape) != tuple(h.shape) or tuple(tm.shape) != (cap, C) or not (h.is_contiguous() and hh.is_contiguous() and tm.is_contiguous()):
        raise ValueError('cne_gate_cached: h and hh must be contiguous [rows, C] of one shape, tm a contiguous [cap, C] (cap = %d), C a multiple '
                         'of 4; got %s, %s, %s' % (cap, tuple(h.shape), tuple(hh.shape), tuple(tm.shape)))
    if out is None:
        out = torch.empty((cap * S, C), dtype=torch.float32, device=h.device)
    _mat(out, 'out')
    if tuple(out.shape) != (cap * S, C) or not out.is_contiguous():
        raise ValueError('cne_gate_cached: out must be a contiguous [cap S, C]')
    if n_rows_dev is not None:
        _vec(n_rows_dev, 'n_rows_dev', 1, dtype=torch.int32)
    check(lib.lime_cne_gate_cached_f32(_p(h), _p(hh), _p(offsets), _p(lens), _p(idx), _p(tm), _p(out), cap, S, C, _p(n_rows_dev), _stream()),
          'lime_cne_gate_cached_f32')
    return out
