"""The workspace contract of every entry of include/lime_hip.h that takes a caller-provided scratch buffer, on the MI355X.

The header promises that ``lime_*_workspace(...)`` floats (bytes for ``lime_rank_metrics``) are enough and that what the buffer holds
on entry does not matter; ``ops._workspace`` never hands a kernel fewer than 1 << 20 floats of finite leftovers, so neither promise is
visible from the other GPU tests.  Here every entry gets a buffer of EXACTLY the size its size function returns, 16-byte aligned,
inside a larger device allocation with a guard band of 1 << 18 floats (1 MiB, more than the largest partial tile any of these
kernels writes) on each side, and each case asserts:

1. exact size is enough and the result is right: the outputs match the fp64 statement and the tolerance of the operation's own test
   (test_backward_gpu.py, test_wide_heads_gpu.py, test_cnn_gpu.py, test_kernels_gpu.py, test_rank_metrics_gpu.py);
2. nothing is written outside: both guard bands still hold the sentinel, compared as int32;
3. stale contents do not matter: the scratch buffer is poisoned with all-zero bits, 0x7FC00000 (a quiet NaN as a float, a large
   positive flag word) and 0xFFFFFFFF, and the three results are bitwise equal;
4. outputs are fully written: where the call does not accumulate, the outputs start as NaN (the ones ``ops`` allocates with
   ``torch.empty`` / ``torch.empty_like`` too: both hand out NaN-filled memory for the duration of a call) and come out finite
   wherever the operation defines them;
5. a short buffer is refused, not used: with one element less the call fails with LimeHipError and the outputs, the guard bands and
   the poisoned scratch buffer are bit for bit what they were -- the pointer still lies inside the guarded allocation.

Entries that reach their scratch through ``ops._workspace`` get it replaced (pytest's monkeypatch) by a function that returns the
exact-size view and asserts that the size asked for is what the matching size function returns; the entries for which ``ops``
allocates with ``torch.empty`` itself are called through ``_lib.load()`` the way ``ops`` calls them."""
import ctypes
import functools
import math
from contextlib import contextmanager

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import rel_err

pytestmark = pytest.mark.gpu

TIGHT = 5e-5                    # test_backward_gpu.py: exact-fp32 kernels against fp64
BWD = 2e-4                      # test_backward_gpu.py / test_wide_heads_gpu.py: gradients against fp64 autograd
KTOL = 2e-5                     # test_cnn_gpu.py (conv weight gradient), test_kernels_gpu.py's TIGHT (candidate attention weights)
ATOL = 1e-12                    # test_rank_metrics_gpu.py: the ranking metrics

GUARD = 1 << 18                 # words of each guard band
SENTINEL = 0x5A5AA5A5
POISONS = (0, 0x7FC00000, -1)   # -1: 0xFFFFFFFF as int32
SPLITS = pytest.mark.parametrize('split', [True, False], ids=['split_product', 'fp32_mfma'])

_EMPTY, _EMPTY_LIKE = torch.empty, torch.empty_like


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from lime_cikm25_amd import ops as _ops
    from lime_cikm25_amd import _lib
    _lib.load()
    return _ops


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=dtype) * 2 - 1) * scale


def close(got, want, tol, what='', strict=False):
    got = got.detach().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), '%s: not finite everywhere (an output the kernel did not write?)' % what
    e = rel_err(got.numpy(), want.detach().numpy())
    print('%s: rel err %.3e (bound %.1e)' % (what, e, tol))
    assert (e < tol) if strict else (e <= tol), '%s: rel err %.3e > %.1e' % (what, e, tol)


def bits(t):
    """The tensor as integers of its element size: comparisons that see NaN payloads and signed zeros."""
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@contextmanager
def split_mode(ops, split):
    prev = ops.set_split_gemm(split)
    try:
        yield
    finally:
        ops.set_split_gemm(prev)


# ---------------------------------------------------------------------------------------------------------------------
# the harness
# ---------------------------------------------------------------------------------------------------------------------
class Scratch:
    """`words` 4-byte words of poisoned scratch between two guard bands of GUARD sentinel words, in one device allocation."""

    def __init__(self, words, poison):
        self.words, self.poison = words, poison
        self.raw = _EMPTY(2 * GUARD + words, dtype=torch.int32, device='cuda')
        self.raw[:GUARD] = SENTINEL
        self.raw[GUARD:GUARD + words] = poison
        self.raw[GUARD + words:] = SENTINEL
        self.ptr = self.raw.data_ptr() + 4 * GUARD
        assert self.ptr % 16 == 0                   # as torch's own allocations: lime_conv1d_wgrad_f32 requires it

    def floats(self):
        return self.raw[GUARD:GUARD + self.words].view(torch.float32)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == SENTINEL).all()) and bool((self.raw[GUARD + self.words:] == SENTINEL).all())

    def still_poisoned(self):
        return bool((self.raw[GUARD:GUARD + self.words] == self.poison).all())


class Harness:
    """One call's scratch buffers (each of exactly the size asked for, or one element less with `short`) and the outputs whose bits
    must survive a refused call."""

    def __init__(self, poison, sizes, short=False):
        self.poison, self.sizes, self.short = poison, sorted(int(s) for s in sizes), short
        self.scratch, self.owned = [], []

    def workspace(self, device, floats):
        """Stands in for ops._workspace(device, floats)."""
        floats = int(floats)
        assert floats in self.sizes, 'the call asks for %d floats of workspace, the size functions return %s' % (floats, self.sizes)
        assert floats > 1
        s = Scratch(floats - (1 if self.short else 0), self.poison)
        self.scratch.append(s)
        return s.floats()

    def workspace_bytes(self, n_bytes):
        """-> (pointer, byte count to pass) of a scratch buffer sized in bytes (lime_rank_metrics)."""
        assert n_bytes in self.sizes and n_bytes % 4 == 0 and n_bytes > 1
        s = Scratch(n_bytes // 4, self.poison)          # short: the same words, one byte less on offer
        self.scratch.append(s)
        return s.ptr, n_bytes - (1 if self.short else 0)

    def own(self, t):
        self.owned.append((t, t.clone()))
        return t

    def nan(self, *shape, dtype=torch.float32):
        return self.own(_EMPTY(shape, dtype=dtype, device='cuda').fill_(float('nan')))

    def _empty(self, *args, **kw):
        t = _EMPTY(*args, **kw)
        return self.own(t.fill_(float('nan'))) if t.is_cuda and t.is_floating_point() else t

    def _empty_like(self, *args, **kw):
        t = _EMPTY_LIKE(*args, **kw)
        return self.own(t.fill_(float('nan'))) if t.is_cuda and t.is_floating_point() else t

    def install(self, m, ops):
        m.setattr(ops, '_workspace', self.workspace)
        m.setattr(torch, 'empty', self._empty)
        m.setattr(torch, 'empty_like', self._empty_like)

    def guards_intact(self):
        return all(s.guards_intact() for s in self.scratch)

    def untouched(self):
        return all(s.still_poisoned() for s in self.scratch) and all(same_bits(t, was) for t, was in self.owned)


def contract(monkeypatch, ops, sizes, call, verify):
    """`call(h)` runs the entry on fresh outputs (taking its scratch from the harness `h`) and returns them; `verify(*outputs)`
    compares them with the reference.  `sizes`: what the matching lime_*_workspace() functions return for this call."""
    from lime_cikm25_amd._lib import LimeHipError
    runs = []
    for poison in POISONS:
        h = Harness(poison, sizes)
        with monkeypatch.context() as m:
            h.install(m, ops)
            outs = call(h)
            torch.cuda.synchronize()
        assert h.scratch, 'the call took no workspace'
        assert h.guards_intact(), 'scratch poisoned with %#x: the call wrote outside its %s floats' % (poison & 0xFFFFFFFF, h.sizes)
        runs.append([o.clone() for o in outs])
    for poison, run in zip(POISONS[1:], runs[1:]):
        for i, (a, b) in enumerate(zip(runs[0], run)):
            assert same_bits(a, b), 'output %d depends on what the workspace held on entry (zeros against %#x)' % (i, poison & 0xFFFFFFFF)
    verify(*runs[0])
    h = Harness(POISONS[1], sizes, short=True)
    with monkeypatch.context() as m:
        h.install(m, ops)
        with pytest.raises(LimeHipError):
            call(h)
        torch.cuda.synchronize()
    assert h.scratch, 'the short call took no workspace'
    assert h.guards_intact(), 'the refused call wrote outside its buffer'
    assert h.untouched(), 'the refused call wrote to its outputs or to the short buffer'


def c_args(ops):
    from lime_cikm25_amd import _lib
    return _lib.load(), _lib.check, ops._p, ops._stream


# ---------------------------------------------------------------------------------------------------------------------
# lime_linear_wgrad_f32, lime_colsum_f32
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wgrad_data(M, N, K):
    dy, x = rnd(M, N, seed=1), rnd(M, K, seed=2)
    return dy, x, (dy.double().t() @ x.double()).float(), dy.double().sum(0).float()


@SPLITS
@pytest.mark.parametrize('variant', ['dw', 'dw_db', 'accumulate_strided'])
@pytest.mark.parametrize('M,N,K', [(333, 50, 100), (1000, 900, 300), (500, 64, 192), (600, 128, 320), (4096, 300, 304), (5000, 300, 512),
                                   (4127, 300, 300)])
def test_linear_wgrad(ops, monkeypatch, M, N, K, variant, split):
    """(333, 50, 100): the scalar kernel with the ones column; (1000, 900, 300): the vector / DMA kernel, five 64-column k tiles, ones
    column; (500, 64, 192) and (600, 128, 320): K fills its tiles, so db comes from the column-sum pass that lives behind the partial
    tiles; (4096, 300, 304): split product with the ones column in a tile of its own; (5000, 300, 512): split product, transposed
    reduction, then the column sums behind the used part; (4127, 300, 300): ragged tail."""
    lib = c_args(ops)[0]
    dy, x, want, want_b = wgrad_data(M, N, K)
    dyg, xg = dy.cuda(), x.cuda()
    base, base_b = rnd(N, K + 8, seed=5), rnd(N, seed=6)

    def call(h):
        if variant == 'dw':
            return (ops.linear_wgrad(dyg, xg, out=h.nan(N, K)),)
        if variant == 'dw_db':
            return ops.linear_wgrad(dyg, xg, out=h.nan(N, K), bias_out=h.nan(N))
        wide, b = h.own(base.cuda()), h.own(base_b.cuda())
        ops.linear_wgrad(dyg, xg, out=wide[:, 4:K + 4], accumulate=True, bias_out=b)
        return wide, b

    def verify(dw, db=None):
        if variant == 'accumulate_strided':
            assert torch.equal(dw[:, :4].cpu(), base[:, :4]) and torch.equal(dw[:, K + 4:].cpu(), base[:, K + 4:])
            close(dw[:, 4:K + 4], base[:, 4:K + 4] + want, TIGHT, 'wgrad accumulate')
            close(db, base_b + want_b, TIGHT, 'bias accumulate')
        else:
            close(dw, want, TIGHT, 'wgrad %s' % ((M, N, K),))
            if db is not None:
                close(db, want_b, TIGHT, 'bias gradient %s' % ((M, N, K),))

    with split_mode(ops, split):
        contract(monkeypatch, ops, [lib.lime_linear_wgrad_workspace(M, N, K)], call, verify)


@pytest.mark.parametrize('M,N', [(1, 7), (1000, 300), (66000, 8)])
def test_colsum(ops, monkeypatch, M, N):
    """(66000, 8) reaches the cap of 256 row blocks."""
    lib = c_args(ops)[0]
    x = rnd(M, N, seed=6)
    xg = x.cuda()
    contract(monkeypatch, ops, [lib.lime_colsum_workspace(M, N)], lambda h: (ops.colsum(xg, out=h.nan(N)),),
             lambda out: close(out, x.double().sum(0).float(), TIGHT, 'colsum'))


# ---------------------------------------------------------------------------------------------------------------------
# lime_layernorm_bwd_f32, lime_layernorm_bwd_dropout_f32
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layernorm_data(M, E, div):
    """test_backward_gpu.py::test_layernorm_bwd_and_rstd's statement, with y and rstd taken from the reference itself."""
    a, w, b = rnd(M, 64, seed=1), rnd(E, 64, seed=2, scale=0.3), rnd(E, seed=3)
    res = rnd(M, E, seed=4)
    gamma, beta = rnd(E, seed=5) * 0.5 + 1.0, rnd(E, seed=6)
    dy = rnd((M + div - 1) // div, E, seed=7)
    z = (a @ w.t() + b + res).double().requires_grad_()
    gd, bd = gamma.double().requires_grad_(), beta.double().requires_grad_()
    y = F.layer_norm(z, (E,), gd, bd, 1e-5)
    y.backward(dy.double().repeat_interleave(div, dim=0)[:M] / div)
    rstd = (1.0 / torch.sqrt(z.detach().var(dim=1, unbiased=False) + 1e-5)).float()
    return dy, y.detach().float(), gamma, beta, rstd, z.grad, gd.grad.float(), bd.grad.float()


@pytest.mark.parametrize('with_dropout', [False, True], ids=['plain', 'dropout'])
@pytest.mark.parametrize('M,E,div', [(96, 300, 1), (300, 400, 1), (64, 50, 16)])
def test_layernorm_bwd(ops, monkeypatch, M, E, div, with_dropout):
    """With dropout: the mask is read back through ops.dropout on ones; dzsum is then the column sums of the dropped gradient.  E = 50
    has no 16-byte rows: lime_layernorm_bwd_dropout_f32 takes 16-byte friendly operands only, so ops.layernorm_bwd goes through
    lime_layernorm_bwd_f32, lime_dropout_f32 and lime_colsum_f32 there -- each with a workspace of exactly its own size."""
    lib = c_args(ops)[0]
    dy, y, gamma, beta, rstd, dz64, dgamma, dbeta = layernorm_data(M, E, div)
    dev = [t.cuda() for t in (dy, y, gamma, beta, rstd)]
    drop = (0.2, 1234567, 5) if with_dropout else None
    sizes = [lib.lime_layernorm_bwd_workspace(M, E)]
    if with_dropout:
        keep = ops.dropout(torch.ones(M, E, device='cuda'), *drop).cpu().double()
        if E % 4:
            sizes.append(lib.lime_colsum_workspace(M, E))

    def verify(dz, dg, db, dzs, dt=None):
        close(dz, dz64.float(), BWD, 'dz')
        close(dg, dgamma, BWD, 'dgamma')
        close(db, dbeta, BWD, 'dbeta')
        if with_dropout:
            close(dt, (dz64 * keep).float(), BWD, 'dropped dz')
            close(dzs, (dz64 * keep).sum(0).float(), BWD, 'dzsum of the dropped dz')
        else:
            close(dzs, dz64.sum(0).float(), BWD, 'dzsum')

    contract(monkeypatch, ops, sizes, lambda h: ops.layernorm_bwd(*dev, dy_div=div, dy_scale=1.0 / div, dropout=drop), verify)


# ---------------------------------------------------------------------------------------------------------------------
# token attention: the blocked backward (S > 128), the forward with dropout, the wide heads
# ---------------------------------------------------------------------------------------------------------------------
def attention_ref(vals, dout, n_seq, S, nh, hd, keep=None, mask=None):
    """vals [tok, 3, nh, hd] -> (out [tok, nh * hd], d vals) of softmax(q k^T / sqrt(hd)) (* keep) v in fp64."""
    x = vals.double().requires_grad_()
    q, k, v = (x[:, i].reshape(n_seq, S, nh, hd).permute(0, 2, 1, 3) for i in range(3))
    a = q @ k.transpose(-1, -2) / math.sqrt(hd)
    if mask is not None:
        a = a.masked_fill(mask.view(n_seq, 1, 1, S) == 0, -1e9)
    p = torch.softmax(a, dim=-1)
    if keep is not None:
        p = p * keep
    o = (p @ v).permute(0, 2, 1, 3).reshape(n_seq * S, nh * hd)
    o.backward(dout.double())
    return o.detach().float(), x.grad.float()


@functools.lru_cache(maxsize=None)
def attention_data(n_seq, S, nh, hd, hs):
    tok = n_seq * S
    vals, dout = rnd(tok, 3, nh, hd, seed=1), rnd(tok, nh * hd, seed=2)
    qkv = torch.zeros(tok, 3, nh, hs)
    qkv[..., :hd] = vals
    o, dvals = attention_ref(vals, dout, n_seq, S, nh, hd)
    want = torch.zeros(tok, 3, nh, hs)
    want[..., :hd] = dvals
    return vals, qkv.view(tok, 3 * nh * hs), dout, o, want.view(tok, 3 * nh * hs)


def attention_keep(ops, n_seq, S, nh, drop):
    return ops.dropout(torch.ones(n_seq * nh * S, S, device='cuda'), *drop).cpu().double().view(n_seq, nh, S, S)


# two key blocks of 128 (one dQ slab behind the row statistics) at S = 129, 200 and 256; S = 385: four key blocks, three slabs
BLOCKED = [(1, 129, 2, 20, 20), (2, 256, 4, 32, 32), (1, 200, 3, 30, 32), (1, 385, 2, 20, 20)]


def blocked_sizes(lib, n_seq, S, nh, hd):
    need = lib.lime_token_attention_bwd_workspace(n_seq, S, nh)
    n_blk = (S + 127) // 128
    assert need == lib.lime_token_attention_bwd_workspace_wide(n_seq, S, nh, hd)
    assert need == lib.lime_token_attention_stats_workspace(n_seq, S, nh) + (n_blk - 1) * n_seq * S * nh * 32
    return [need]


@SPLITS
@pytest.mark.parametrize('stats', ['recomputed', 'lse'])
@pytest.mark.parametrize('n_seq,S,nh,hd,hs', BLOCKED)
def test_token_attention_bwd_blocked(ops, monkeypatch, n_seq, S, nh, hd, hs, stats, split):
    """lime_token_attention_bwd_f32 and _bwd_lse_f32 for S > 128: one and three dQ slabs behind the row statistics, heads 20 and 32
    columns apart, and both split modes (the split-product and the fp32-MFMA blocked kernels with their own slab stores)."""
    lib = c_args(ops)[0]
    tok, W, scale = n_seq * S, nh * hs, 1.0 / math.sqrt(hd)
    _, qkv, dout, o, want = attention_data(n_seq, S, nh, hd, hs)
    g, dg = qkv.cuda(), dout.cuda()
    q, k, v = g[:, :W], g[:, W:2 * W], g[:, 2 * W:]
    with split_mode(ops, split):
        lse = torch.empty(tok * nh, device='cuda') if stats == 'lse' else None
        out = ops.token_attention(q, k, v, n_seq, S, nh, hd, scale, head_stride=hs, lse=lse)
        close(out, o, TIGHT, 'attention forward')

        def verify(dqkv):
            close(dqkv, want, BWD, 'dqkv')
            if hs > hd:
                assert (dqkv.view(tok, 3, nh, hs)[..., hd:] == 0).all(), 'pad columns must be exact zeros'

        contract(monkeypatch, ops, blocked_sizes(lib, n_seq, S, nh, hd),
                 lambda h: (ops.token_attention_bwd(q, k, v, dg, n_seq, S, nh, hd, scale, head_stride=hs, dqkv=h.nan(tok, 3 * W), out=out,
                                                    lse=lse),), verify)


@SPLITS
def test_token_attention_bwd_blocked_with_dropout(ops, monkeypatch, split):
    lib = c_args(ops)[0]
    n_seq, S, nh, hd, hs = 1, 200, 3, 30, 32
    tok, W, scale, drop = n_seq * S, nh * hs, 1.0 / math.sqrt(hd), (0.2, 424242, 2)
    vals, qkv, dout, _, _ = attention_data(n_seq, S, nh, hd, hs)
    o, dvals = attention_ref(vals, dout, n_seq, S, nh, hd, keep=attention_keep(ops, n_seq, S, nh, drop))
    want = torch.zeros(tok, 3, nh, hs)
    want[..., :hd] = dvals
    g, dg = qkv.cuda(), dout.cuda()
    q, k, v = g[:, :W], g[:, W:2 * W], g[:, 2 * W:]
    with split_mode(ops, split):
        out = ops.token_attention_dropout(q, k, v, n_seq, S, nh, hd, scale, *drop, head_stride=hs)
        close(out, o, TIGHT, 'attention forward with dropout')
        contract(monkeypatch, ops, blocked_sizes(lib, n_seq, S, nh, hd),
                 lambda h: (ops.token_attention_bwd(q, k, v, dg, n_seq, S, nh, hd, scale, head_stride=hs, dqkv=h.nan(tok, 3 * W), out=out,
                                                    dropout=drop),),
                 lambda dqkv: close(dqkv, want.view(tok, 3 * W), BWD, 'dqkv with dropout'))


@SPLITS
@pytest.mark.parametrize('n_seq,S,nh,hd,hs', BLOCKED)
def test_token_attention_dropout_forward(ops, monkeypatch, n_seq, S, nh, hd, hs, split):
    """lime_token_attention_dropout_f32 for S > 128 with exactly lime_token_attention_stats_workspace() floats: all it requires."""
    lib = c_args(ops)[0]
    W, scale, drop = nh * hs, 1.0 / math.sqrt(hd), (0.2, 987654321, 3)
    vals, qkv, dout, _, _ = attention_data(n_seq, S, nh, hd, hs)
    o, _ = attention_ref(vals, dout, n_seq, S, nh, hd, keep=attention_keep(ops, n_seq, S, nh, drop))
    g = qkv.cuda()
    need = lib.lime_token_attention_stats_workspace(n_seq, S, nh)
    assert need == 2 * n_seq * S * nh < lib.lime_token_attention_bwd_workspace(n_seq, S, nh)
    with split_mode(ops, split):
        contract(monkeypatch, ops, [need],
                 lambda h: (ops.token_attention_dropout(g[:, :W], g[:, W:2 * W], g[:, 2 * W:], n_seq, S, nh, hd, scale, *drop, head_stride=hs),),
                 lambda out: close(out, o, TIGHT, 'attention forward with dropout'))


def test_token_attention_dropout_names_the_size_function_it_checks(ops, monkeypatch):
    from lime_cikm25_amd._lib import LimeHipError
    g = torch.zeros(130, 3 * 32, device='cuda')
    monkeypatch.setattr(ops, '_workspace', lambda device, floats: Scratch(int(floats) - 1, 0).floats())
    with pytest.raises(LimeHipError, match=r'lime_token_attention_stats_workspace\(\)'):
        ops.token_attention_dropout(g[:, :32], g[:, 32:64], g[:, 64:], 1, 130, 1, 32, 1.0, 0.1, 1, 2)


@pytest.mark.parametrize('masked', [False, True], ids=['no_mask', 'key_mask'])
@pytest.mark.parametrize('n_seq,S,nh,hd', [(2, 40, 3, 100), (1, 130, 3, 100)])
def test_token_attention_bwd_wide(ops, monkeypatch, n_seq, S, nh, hd, masked):
    """Heads of 100 columns: one and three 64-row blocks; 3 floats of statistics a (token, head) at every S."""
    lib = c_args(ops)[0]
    tok, W, scale = n_seq * S, nh * hd, 1.0 / math.sqrt(hd)
    vals, dout = rnd(tok, 3, nh, hd, seed=1), rnd(tok, W, seed=2)
    mask = (torch.arange(S)[None, :] < torch.tensor([17, S][:n_seq] if n_seq > 1 else [S - 30])[:, None]) if masked else None
    _, dvals = attention_ref(vals, dout, n_seq, S, nh, hd, mask=mask)
    g, dg = vals.reshape(tok, 3 * W).cuda(), dout.cuda()
    q, k, v = g[:, :W], g[:, W:2 * W], g[:, 2 * W:]
    need = lib.lime_token_attention_bwd_workspace_wide(n_seq, S, nh, hd)
    assert need == 3 * tok * nh
    contract(monkeypatch, ops, [need],
             lambda h: (ops.token_attention_bwd(q, k, v, dg, n_seq, S, nh, hd, scale, dqkv=h.nan(tok, 3 * W),
                                                key_mask=mask.cuda() if masked else None),),
             lambda dqkv: close(dqkv, dvals.reshape(tok, 3 * W), BWD, 'wide dqkv'))


# ---------------------------------------------------------------------------------------------------------------------
# lime_embed_bwd_sorted_f32, lime_grad_clip_coef_f32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [300, 302])
@pytest.mark.parametrize('rows,share,hot', [(9000, 0.4, False), (20000, 0.4, False), (20000, 0.45, True)])
def test_embed_bwd_sorted(ops, monkeypatch, rows, share, hot, D):
    """`share` of the positions carry id 0.  The kernel sums the first run of the sorted order in a pass of its own (256 partial rows
    behind the chunks' partials and flag words) from 8192 positions on: 40 % of 20000 stays below that, 45 % reaches it.  D = 302:
    the scratch rows are padded to 304 floats.  The table starts as NaN: rows that receive a contribution are stored, the others
    (ids 497 .. 499 never occur) keep their bits."""
    lib, check, _p, _stream = c_args(ops)
    V = 500
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1, V - 3, (rows,), generator=g, dtype=torch.int32)
    ids[torch.rand(rows, generator=g) < share] = 0
    assert (int((ids == 0).sum()) >= 8192) == hot
    dx = rnd(rows, D, seed=4)
    want = torch.zeros(V, D, dtype=torch.float64).index_add_(0, ids.long(), dx.double()).float()
    touched = torch.bincount(ids.long(), minlength=V) > 0
    assert touched[:V - 3].all() and not touched[V - 3:].any()
    sorted_ids, order = torch.sort(ids.cuda(), stable=True)
    order, dxg = order.to(torch.int32), dx.cuda()
    need = int(lib.lime_embed_bwd_sorted_workspace(rows, D))

    def call(h):
        ws, table = h.workspace(dxg.device, need), h.nan(V, D)
        check(lib.lime_embed_bwd_sorted_f32(_p(order), _p(sorted_ids), _p(dxg), D, _p(table), D, rows, D, _p(ws), ws.numel(), _stream()),
              'lime_embed_bwd_sorted_f32')
        return (table,)

    def verify(table):
        close(table[:V - 3], want[:V - 3], BWD, 'embedding gradient')
        assert same_bits(table[V - 3:], torch.full((3, D), float('nan'), device='cuda')), 'a row without a contribution was written'

    contract(monkeypatch, ops, [need], call, verify)


@pytest.mark.parametrize('n', [100003, 300000])
def test_grad_clip_coef(ops, monkeypatch, n):
    """Exactly the 1024 floats the header asks for; n = 300000 reaches the cap of 1024 blocks."""
    g = rnd(n, seed=10, scale=0.05)
    gg = g.cuda()
    norm = float(g.double().norm())
    want = torch.tensor([norm, min(1.0, 4.0 / (norm + 1e-6))], dtype=torch.float64).float()
    assert want[1] < 1
    contract(monkeypatch, ops, [1024], lambda h: (ops.grad_clip_coef(gg, 4.0),), lambda out: close(out, want, TIGHT, 'norm and coefficient'))


# ---------------------------------------------------------------------------------------------------------------------
# backward of the fused tail kernels: the statements of test_backward_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,k,D,A', [(7, 3, 400, 400), (300, 3, 400, 400)])
def test_intent_fuse_bwd(ops, monkeypatch, M, k, D, A):
    lib = c_args(ops)[0]
    iv, hid = rnd(2 * M * k, D, seed=1), torch.tanh(rnd(2 * M * k, A, seed=2))
    a2t, a2b = rnd(A, seed=3, scale=0.2), rnd(A, seed=4, scale=0.2)
    dcontent = rnd(M, 2 * D, seed=5)
    x, h64, wt, wb = (t.double().requires_grad_() for t in (iv, hid, a2t, a2b))

    def pool(xx, hh, w):
        alpha = torch.softmax((hh.view(M, k, A) * w).sum(-1), dim=1)
        return (alpha.unsqueeze(-1) * xx.view(M, k, D)).sum(1)
    t, b = pool(x[:M * k], h64[:M * k], wt), pool(x[M * k:], h64[M * k:], wb)
    sim = (F.cosine_similarity(t, b, dim=1) + 1) / 2
    torch.cat([t, sim.unsqueeze(1) * b], dim=1).backward(dcontent.double())
    dev = [v.cuda() for v in (iv, hid, a2t, a2b, dcontent)]

    def verify(*got):
        for name, a, ref in zip(('d intents', 'd hidden', 'd affine2 title', 'd affine2 body'), got, (x, h64, wt, wb)):
            close(a, ref.grad.float(), BWD, name)

    contract(monkeypatch, ops, [lib.lime_intent_fuse_bwd_workspace(M, A)], lambda h: ops.intent_fuse_bwd(*dev, M, k, D, A), verify)


@pytest.mark.parametrize('rows,D', [(13, 400), (1600, 400)])
def test_gate_ln_bwd(ops, monkeypatch, rows, D):
    lib = c_args(ops)[0]
    y, x = rnd(rows, D, seed=1), rnd(rows, D, seed=2)
    s = torch.softmax(rnd(rows, seed=3), dim=0) * 5
    bias, gamma, beta = rnd(D, seed=4, scale=0.3), rnd(D, seed=5, scale=0.3) + 1, rnd(D, seed=6, scale=0.3)
    dout = rnd(rows, D, seed=7)
    refs = yd, xd, sd, bd, gd, ed = [t.double().requires_grad_() for t in (y, x, s, bias, gamma, beta)]
    gate = torch.sigmoid(sd.unsqueeze(1) * yd + bd)
    F.layer_norm(gate * (sd.unsqueeze(1) * xd) + (1 - gate) * xd, (D,), gd, ed, 1e-5).backward(dout.double())
    dev = [t.cuda() for t in (y, x, s, bias, gamma, beta)]

    def verify(*got):
        for name, a, ref in zip(('dy', 'dx', 'dscale', 'dbias', 'dgamma', 'dbeta'), got, refs):
            close(a.view(ref.shape), ref.grad.float(), BWD, name)

    contract(monkeypatch, ops, [lib.lime_gate_ln_bwd_workspace(rows, D)], lambda h: ops.gate_ln_bwd(*dev, 1e-5, dout.cuda()), verify)


@pytest.mark.parametrize('B,N,H,A,D,penalty', [(3, 5, 50, 400, 400, True), (2, 1, 7, 64, 48, False)])
def test_interest_match_bwd(ops, monkeypatch, B, N, H, A, D, penalty):
    lib = c_args(ops)[0]
    kp, qp = rnd(B * H, A, seed=1, scale=0.3), rnd(B * N, A, seed=2, scale=0.3)
    g, cand = rnd(B * H, D, seed=3), rnd(B * N, D, seed=4)
    remaining = rnd(B, N, seed=5, scale=8.0)
    special = torch.tensor([0.0, -0.0, 1e5, -1e5, 40.0, -40.0])[:B * N]
    remaining.view(-1)[:special.numel()] = special
    if B * N > 2 * special.numel():
        remaining.view(-1)[-special.numel():] = special.flip(0)
    dlogits = rnd(B, N, seed=6)
    alpha, beta, scale = 0.3, 0.3, 1.0 / math.sqrt(A)
    refs = kd, qd, gd, cd = [t.double().requires_grad_() for t in (kp, qp, g, cand)]
    a = torch.einsum('bha,bna->bnh', kd.view(B, H, A), qd.view(B, N, A)) * scale
    base = ((torch.softmax(a, dim=-1) @ gd.view(B, H, D)) * cd.view(B, N, D)).sum(-1)
    r = remaining.double()
    w = torch.sigmoid(alpha * r)
    w = torch.where(r >= 0, w, beta * w) if penalty else torch.sigmoid(alpha * r.abs())
    (base * w).backward(dlogits.double())
    dev = [t.cuda().view(-1) for t in (kp, qp, g, cand)]

    def verify(*got):
        for name, x, ref in zip(('dkp', 'dqp', 'dg', 'dcand'), got, refs):
            close(x, ref.grad.float(), BWD, name)

    contract(monkeypatch, ops, [lib.lime_interest_match_bwd_workspace(B, N, H, A, D)],
             lambda h: ops.interest_match_bwd(*dev, remaining.cuda(), dlogits.cuda(), B, N, H, A, D, scale, alpha, beta, True, penalty), verify)


# ---------------------------------------------------------------------------------------------------------------------
# lime_conv1d_wgrad_f32
# ---------------------------------------------------------------------------------------------------------------------
@SPLITS
@pytest.mark.parametrize('C,O,T,win,n,gather', [(120, 36, 1, 3, 29, True), (48, 64, 32, 3, 16, False), (48, 64, 32, 5, 16, False)])
def test_conv1d_wgrad(ops, monkeypatch, C, O, T, win, n, gather, split):
    """The smallest weight-gradient case of test_cnn_gpu.py (29 rows, gathered from a table), and 512 rows (16 sequences of 32
    tokens), which split over several workgroups' partial tiles."""
    lib = c_args(ops)[0]
    V, M = 61, n * T
    table = rnd(V, C, seed=21, dtype=torch.float64)
    table[0] = 1.5
    w = rnd(O, C, win, seed=22, scale=0.2, dtype=torch.float64).requires_grad_(True)
    gen = torch.Generator().manual_seed(23)
    ids = torch.randint(1, V, (n, T), generator=gen, dtype=torch.int32)
    for s, ln in enumerate(torch.randint(1, T + 1, (n,), generator=gen)):
        ids[s, ln:] = 0
    ids[0] = 0
    ids = ids.reshape(-1)
    x = table[ids.long()]
    dy = rnd(M, O, seed=24, dtype=torch.float64)
    y = F.conv1d(x.view(n, T, C).permute(0, 2, 1), w, None, padding=(win - 1) // 2).permute(0, 2, 1).reshape(M, O)
    (y * dy).sum().backward()
    need = lib.lime_conv1d_wgrad_workspace(M, O, C, win)
    assert need % (O * win * C) == 0 and (need > O * win * C) == (M >= 512)        # several row splits from 512 rows on
    dyg, src, idg = dy.float().cuda(), (table if gather else x).float().cuda(), ids.cuda() if gather else None
    with split_mode(ops, split):
        contract(monkeypatch, ops, [need], lambda h: (ops.conv1d_window_wgrad(dyg, src, win, T, ids=idg),),
                 lambda dw: close(dw.view(O, win, C).permute(0, 2, 1), w.grad.float(), KTOL, 'conv weight gradient', strict=True))


# ---------------------------------------------------------------------------------------------------------------------
# lime_cand_attn_weights_ws_f32 / _shared_f32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry', ['ws', 'shared'])
@pytest.mark.parametrize('B,N,H,n_head,D', [(4, 5, 50, 10, 400), (3, 1, 7, 2, 16)])
def test_cand_attn_weights(ops, monkeypatch, B, N, H, n_head, D, entry):
    """test_kernels_gpu.py::test_cand_attn_weights' statement in fp64; `shared`: one history for all B rows (hist_div = B)."""
    lib, check, _p, _stream = c_args(ops)
    div = B if entry == 'shared' else 1
    Bh = B // div
    qp, kp = rnd(B * N, D, seed=1, scale=3), rnd(Bh * H, D, seed=2, scale=3)
    lens = torch.randint(1, H + 1, (Bh,), generator=torch.Generator().manual_seed(3))
    if Bh > 1:
        lens[0] = 0                                               # an empty history
    mask = torch.arange(H)[None, :] < lens[:, None]
    Q = qp.double().view(B, N, n_head, D // n_head).transpose(1, 2)
    K = kp.double().view(Bh, H, n_head, D // n_head).transpose(1, 2).repeat_interleave(div, dim=0)
    s = (Q @ K.transpose(-2, -1) / D ** 0.5).masked_fill(mask.repeat_interleave(div, dim=0).view(B, 1, 1, H) == 0, -1e9)
    qw = torch.softmax(torch.norm(qp.double().view(B, N, D), dim=-1), dim=1)
    want = torch.softmax((torch.softmax(s, dim=-1).sum(dim=1) * qw.unsqueeze(-1)).sum(dim=1), dim=-1).float()
    qg, kg, mg = qp.cuda(), kp.cuda(), mask.cuda().view(torch.uint8)
    need = int(lib.lime_cand_attn_weights_workspace(B, N, H, n_head))

    def call(h):
        ws, agg = h.workspace(qg.device, need), h.nan(B, H)
        if entry == 'ws':
            st = lib.lime_cand_attn_weights_ws_f32(_p(qg), _p(kg), _p(mg), _p(agg), B, N, H, D, n_head, _p(ws), ws.numel(), _stream())
        else:
            st = lib.lime_cand_attn_weights_shared_f32(_p(qg), _p(kg), _p(mg), _p(agg), B, N, H, D, n_head, div, _p(ws), ws.numel(), _stream())
        check(st, 'lime_cand_attn_weights_%s_f32' % entry)
        return (agg,)

    contract(monkeypatch, ops, [need], call, lambda agg: close(agg, want, KTOL, 'candidate attention weights', strict=True))


# ---------------------------------------------------------------------------------------------------------------------
# lime_rank_metrics (bytes)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_imp', [1, 1024, 1025])
def test_rank_metrics(ops, monkeypatch, n_imp):
    """The four impressions of test_rank_metrics_gpu.py's smallest case (ten scores; the second has no labels and is skipped), repeated
    n_imp times over: one chunk of 1024 impressions, exactly one, and two."""
    from lime_cikm25_amd import _lib, evaluate as E, util as U
    lib, check, _p, _stream = c_args(ops)
    imps = [([0.3, 0.1, 0.2], [1, 0, 0]), ([0.9, 0.8], []), ([0.5, 0.4], [0, 1]), ([0.7, 0.6, 0.2], [0, 1, 0])]
    scores, indices, labels = [], [], []
    for i in range(n_imp):
        s, y = imps[i % 4]
        scores += s
        indices += [i] * len(s)
        labels.append(y)
    off, lab, skip = E.impression_layout(indices, labels)
    want_ranks = U.rank_impressions(scores, indices)
    want_per, want_status = E.metrics_from_ranks(want_ranks, labels, per_impression=True)
    counted = want_status == 0
    R = len(scores)
    dev = dict(scores=torch.tensor(scores, dtype=torch.float32).cuda(), labels=torch.from_numpy(lab).cuda(),
               offsets=torch.from_numpy(np.asarray(off, dtype=np.int32)).cuda(), skip=torch.from_numpy(skip).cuda(), disc=ops._ndcg_discounts(torch.device('cuda', 0)))
    need = int(lib.lime_rank_metrics_workspace(n_imp))
    assert need == (n_imp + 1023) // 1024 * 40

    def call(h):
        ptr, n_bytes = h.workspace_bytes(need)
        outs = dict(ranks=h.own(torch.full((R,), -1, dtype=torch.int32, device='cuda')), per_imp=h.nan(n_imp, 4, dtype=torch.float64),
                    status=h.own(torch.full((n_imp,), -1, dtype=torch.int32, device='cuda')), sums=h.nan(4, dtype=torch.float64),
                    count=h.own(torch.full((1,), -1, dtype=torch.int64, device='cuda')))
        a = _lib.RankMetricsArgs()
        for name, t in list(dev.items()) + list(outs.items()):
            setattr(a, name, t.data_ptr())
        a.workspace, a.workspace_bytes = ptr, n_bytes
        a.R, a.n_imp, a.rank_blocks, a.reduce_blocks, a.reserved = R, n_imp, 0, 0, 0
        check(lib.lime_rank_metrics(ctypes.byref(a), _stream()), 'lime_rank_metrics')
        return tuple(outs.values())

    def verify(ranks, per_imp, status, sums, count):
        assert U.ranks_to_lists(ranks, indices) == want_ranks
        assert status.cpu().numpy().tolist() == want_status.tolist()
        per = per_imp.cpu().numpy()
        assert np.isfinite(per).all() and np.allclose(per, want_per, rtol=0, atol=ATOL)
        assert int(count.cpu()[0]) == int(counted.sum())
        means = sums.cpu().numpy() / max(1, int(counted.sum()))
        assert np.isfinite(means).all() and np.allclose(means, want_per[counted].mean(axis=0) if counted.any() else 0.0, rtol=0, atol=ATOL)

    contract(monkeypatch, ops, [need], call, verify)
