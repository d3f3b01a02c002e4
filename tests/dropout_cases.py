"""The dropout mask of csrc/dropout.h and the operations that draw it, stated on the host -- shared by tests/test_dropout_reference_cpu.py
(which pins this model without a GPU) and tests/test_dropout_kernels_gpu.py (which holds every mask-drawing kernel to it).

The mask: "keep element e of site s under seed" is a pure function of the three (lime_make_dropout / lime_hash4 / lime_keep):
    key    = seed * 0x9E3779B97F4A7C15 + ((s + 1) mod 2^32) * 0xD1B54A32D192ED03             (uint64, wrapping)
    z      = splitmix64's mixer of (e >> 2) + key                                           (one value per four consecutive elements)
    keep   = ((z >> 16 (e & 3)) & 0xFFFF) >= thresh,   thresh = 0 for p <= 0, else min(floor(p * 65536 + 0.5), 0xFFFF)
    scale  = the fp32 value 1.0f / (1.0f - p)
so p is realised in steps of 2^-16 while kept values are scaled by the exact 1 / (1 - p).

The statements are torch fp64 (autograd gives the backward) and take the mask as an explicit multiplier tensor ``m`` = keep * scale
-- the form tests/test_dropout_gpu.py, test_backward_gpu.py and test_wide_heads_gpu.py already use; the statements those files
contained live here now and are imported from here."""
import math

import numpy as np
import torch
import torch.nn.functional as F

_U = np.uint64
GOLDEN, SITE_MUL = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
MIX1, MIX2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB

# the project's own bounds for the same kernels without dropout
TIGHT = 5e-5            # forward results and rstd against fp64 (test_backward_gpu.py)
GEMM_TIGHT = 2e-5       # the GEMM epilogue (test_split_gemm_gpu.py)
BWD = 2e-4              # gradients against fp64 autograd

P = 0.2
# (seed, site): one seed at or above 2^32
SEED_SITES = ((987654321, 2), ((1 << 32) + 12345, 5), (4242, 0))


def _u64(x):
    return np.array([int(x) & 0xFFFFFFFFFFFFFFFF], dtype=_U)


def mixer(z):
    """splitmix64's three-step output function on a uint64 array (wrapping)."""
    z = np.asarray(z, dtype=_U).copy()
    with np.errstate(over='ignore'):
        z ^= z >> _U(30)
        z *= _U(MIX1)
        z ^= z >> _U(27)
        z *= _U(MIX2)
        z ^= z >> _U(31)
    return z


def make_key(seed, site):
    """lime_make_dropout's key: seed and site mixed in wrapping uint64 arithmetic; site + 1 wraps in 32 bits first."""
    with np.errstate(over='ignore'):
        return (_u64(seed) * _U(GOLDEN) + _u64((int(site) + 1) & 0xFFFFFFFF) * _U(SITE_MUL))[0]


def thresh(p):
    """lime_make_dropout's threshold: p is a float (fp32) argument, the product is taken in double."""
    p32 = np.float32(p)
    if p32 <= 0:
        return 0
    t = float(p32) * 65536.0 + 0.5
    return 0xFFFF if t >= 65535.0 else int(t)


def scale(p):
    """The fp32 value 1.0f / (1.0f - p) (1 for p <= 0)."""
    p32 = np.float32(p)
    return np.float32(1.0) if p32 <= 0 else np.float32(1.0) / (np.float32(1.0) - p32)


def keep_mask(p, seed, site, n, start=0):
    """bool [n]: keep elements start .. start + n - 1 of site `site` under `seed`."""
    th = thresh(p)
    if n == 0:
        return np.zeros(0, dtype=bool)
    first, last = start >> 2, (start + n - 1) >> 2
    with np.errstate(over='ignore'):
        z = mixer(np.arange(first, last + 1, dtype=_U) + make_key(seed, site))
    lanes = np.empty((z.size, 4), dtype=np.uint32)
    for e in range(4):
        lanes[:, e] = ((z >> _U(16 * e)) & _U(0xFFFF)).astype(np.uint32)
    lo = start - 4 * first
    return lanes.reshape(-1)[lo:lo + n] >= np.uint32(th)


def multiplier(p, seed, site, shape, start=0):
    """keep * scale as a torch fp64 tensor of `shape` (elements in row-major order from `start`)."""
    n = int(np.prod(shape))
    k = keep_mask(p, seed, site, n, start).reshape(shape)
    return torch.from_numpy(k.astype(np.float64) * float(scale(p)))


def dropped_f32(x, keep, p, times=1):
    """The bitwise statement where an output is one multiplication of an input: where(keep, fl32(x * scale), 0), numpy fp32;
    ``times`` = 2: the two roundings (x * s) * s of the double dropout."""
    y = np.asarray(x, dtype=np.float32)
    for _ in range(times):
        y = y * scale(p)
    return np.where(keep, y, np.float32(0.0)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------
# fp64 statements; m = keep * scale
# ---------------------------------------------------------------------------------------------------
def dropout_ref(x, m):
    return x.double() * m


def dropout2_ref(x, m1, m2):
    return (x.double() * m1) * m2


def embed_pe_dropout_ref(table, ids, pe, period, m_emb, m_pe):
    """drop_pe(drop_emb(table[ids]) + pe[r % period])."""
    x = m_emb * table.double()[ids.long().reshape(-1)]
    if pe is not None:
        rows = torch.arange(ids.numel()) % period
        x = x + pe.double()[rows]
    return m_pe * x


def dropout_add_ln_ref(t, res, gamma, beta, eps, m):
    """(LayerNorm(res + drop(t)), rstd)."""
    z = res.double() + m * t.double()
    y = F.layer_norm(z, (z.shape[1],), gamma.double(), beta.double(), eps)
    return y, 1.0 / torch.sqrt(z.var(dim=1, unbiased=False) + eps)


def layernorm_bwd_ref(z, gamma, beta, dy, div=1, eps=1e-5, m=None):
    """y = LayerNorm(z) and its backward under dy (one dy row per `div` rows, spread as dy / div):
    -> (y, rstd, dz, dgamma, dbeta, dzsum) in fp64; with ``m`` also the dropped copy dz * m as a seventh result, and dzsum is then ITS
    column sums (the bias gradient of the linear in front of that dropout)."""
    M, E = z.shape
    z = z.detach().double().requires_grad_()
    gd, bd = gamma.detach().double().requires_grad_(), beta.detach().double().requires_grad_()
    y = F.layer_norm(z, (E,), gd, bd, eps)
    dy_full = dy.double().repeat_interleave(div, dim=0)[:M] / div
    y.backward(dy_full)
    rstd = 1.0 / torch.sqrt(z.detach().var(dim=1, unbiased=False) + eps)
    if m is None:
        return y.detach(), rstd, z.grad, gd.grad, bd.grad, z.grad.sum(0)
    dt = z.grad * m
    return y.detach(), rstd, z.grad, gd.grad, bd.grad, dt.sum(0), dt


def linear_dropout_ref(a, w, b, act, m):
    """drop(act(A W^T + b)), act 'relu' or None."""
    y = a.double() @ w.double().t() + b.double()
    if act == 'relu':
        y = torch.relu(y)
    return y * m


def attn_ref(vals, n_seq, S, h, hd, scale, mask=None, m=None):
    """vals [tok, 3, h, hd] -> (out [tok, h * hd], log2-domain lse [n_seq, h, S]) in vals' dtype; ``mask`` [n_seq, S]: the key mask
    (-1e9 fill), ``m`` [n_seq, h, S, S]: dropout on the probabilities."""
    q, k, v = (vals[:, i].reshape(n_seq, S, h, hd).transpose(1, 2) for i in range(3))
    a = (q * scale) @ k.transpose(-2, -1)
    if mask is not None:
        a = a.masked_fill(mask.view(n_seq, 1, 1, S) == 0, -1e9)
    p = torch.softmax(a, dim=-1)
    if m is not None:
        p = p * m
    return (p @ v).transpose(1, 2).reshape(n_seq * S, h * hd), torch.logsumexp(a, dim=-1) / math.log(2.0)


def attn_bwd_ref(vals, dout, n_seq, S, h, hd, scale, mask=None, m=None):
    """fp64 autograd of attn_ref -> (out, dqkv [tok, 3, h, hd]) in fp64."""
    x = vals.double().requires_grad_()
    o, _ = attn_ref(x, n_seq, S, h, hd, scale, mask, m)
    o.backward(dout.double())
    return o.detach(), x.grad


def cand_attn_ref(qd, kd, mask, m, B, N, H, nh, hd):
    """The candidate-attention weights of layers.py:66-81: agg [B, H] from qd [B * N, D], kd [B * H, D], the history mask [B, H] and the
    dropout multiplier m [B, nh, N, H] on the per-head probabilities."""
    D = nh * hd
    Q = qd.view(B, N, nh, hd).transpose(1, 2)
    K = kd.view(B, H, nh, hd).transpose(1, 2)
    sc = (Q @ K.transpose(-2, -1)) / (D ** 0.5)
    sc = sc.masked_fill(mask.view(B, 1, 1, H) == 0, -1e9)
    a = torch.softmax(sc, dim=-1) * m
    qw = torch.softmax(torch.norm(Q.transpose(1, 2).reshape(B, N, -1), dim=-1), dim=1)
    return torch.softmax((a.sum(dim=1) * qw.unsqueeze(-1)).sum(dim=1), dim=-1)


# ---------------------------------------------------------------------------------------------------
# the case lists of tests/test_dropout_kernels_gpu.py
# ---------------------------------------------------------------------------------------------------
N_SEQ, N_HEAD = 3, 2
HEADS_NARROW = ((30, 32), (32, 32), (20, 20))          # (head_dim, head_stride): padded, full, packed
HEADS_WIDE = ((36, 36), (100, 100))


def _fwd_cases():
    """(route, S, hd, hs, split): split None = the route does not depend on lime_set_split_gemm."""
    c = []
    for S in (32, 64, 128):                              # split-product forward: heads 32 columns apart
        for hd in (30, 32):
            c.append(('sp', S, hd, 32, True))
    for name, sizes, cap in (('one32', (7, 31), 32), ('one64', (33, 50), 64), ('one128', (65, 100, 127), 128)):
        for hd, hs in ((30, 32), (20, 20)):
            for S in sizes:
                c.append((name, S, hd, hs, None))
            # S at the kernel's capacity: with heads 32 apart the one-pass fp32 kernel runs only with split products off; packed
            # heads never take the split-product kernel
            c.append((name, cap, hd, hs, False if hs == 32 else None))
    for S in (129, 131, 256, 300):                       # blocked: two and three key blocks; its statistics run under both settings
        for hd, hs in ((30, 32), (20, 20)):
            for split in (True, False):
                c.append(('blocked', S, hd, hs, split))
    for S in (33, 64, 65, 130):
        for hd, hs in HEADS_WIDE:
            c.append(('wide', S, hd, hs, None))
    return c


def _bwd_cases():
    c = []
    for S in (31, 33, 65, 127):                          # one-pass fp32: split off, or packed heads
        c.append(('one', S, 30, 32, False))
        c.append(('one', S, 20, 20, None))
    for S in (68, 100, 128):                             # split-product one-pass (phase A, and phase B's quad exchange)
        c.append(('sp', S, 30, 32, True))
    for S in (129, 131, 300):                            # blocked fp32 and split-product
        for split in (True, False):
            c.append(('blocked', S, 30, 32, split))
    for S in (33, 130):
        for hd, hs in HEADS_WIDE:
            c.append(('wide', S, hd, hs, None))
    return c


ATTN_FWD_CASES = _fwd_cases()
ATTN_BWD_CASES = _bwd_cases()
ATTN_S = sorted({c[1] for c in ATTN_FWD_CASES} | {c[1] for c in ATTN_BWD_CASES})


def row_residues(S, n_prob=N_SEQ * N_HEAD):
    """The residues mod 4 of the mask row bases ((prob * S + i) * S) that a call with n_prob (sequence, head) pairs reaches."""
    return {((prob * S + i) * S) % 4 for prob in range(n_prob) for i in range(S)}


def attn_case_id(c):
    route, S, hd, hs, split = c
    return '%s-S%d-hd%d-hs%d-%s' % (route, S, hd, hs, {True: 'split', False: 'fp32', None: 'any'}[split])


# (B, N, H, n_head, head_dim, p): the three dropout shapes of test_backward_gpu.py's test_cand_attn_weights_train_and_bwd, an odd H
# (mask rows off the hash groups) and the limit shape N = 16, H = 256
CAND_CASES = ((4, 5, 50, 10, 40, 0.2), (3, 1, 7, 2, 8, 0.5), (2, 3, 70, 10, 40, 0.2), (2, 3, 33, 2, 8, 0.2), (1, 16, 256, 2, 8, 0.2))
