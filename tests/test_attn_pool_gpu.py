"""The fused additive attention pool (csrc/attn_pool_sp_f32.hip, ops.attn_pool) on the MI355X: against fp64 torch, the device sequence
count and strided output slots, the same bits for a sequence in any tile slot, graph replay after an in-place change of W1, the
two-launch fallback beyond its limits, and argument checks before any launch."""
import pytest
import torch

from helpers import rel_err
from lime_cikm25_amd import ops
from lime_cikm25_amd._lib import LimeHipError

pytestmark = pytest.mark.gpu
KTOL = 2e-5                     # kernel level: fp32-level products against fp64


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale


def ref_pool(x, w1, b1, w2, n, T, mask=None):
    """fp64 layers.Attention (layers.py:285-300) over n sequences of T rows of x."""
    s = (torch.tanh(x @ w1.t() + b1) @ w2).view(n, T)
    if mask is not None:
        s = s.masked_fill(~mask.view(n, T).bool(), -1e9)
    return (torch.softmax(s, dim=1).unsqueeze(2) * x.view(n, T, -1)).sum(dim=1)


def _problem(n, T, D, A, seed):
    x = rnd(n * T, D, seed=seed)
    w1 = rnd(A, D, seed=seed + 1, scale=2.0 / D ** 0.5)
    b1, w2 = rnd(A, seed=seed + 2, scale=0.1), rnd(A, seed=seed + 3, scale=4.0 / A ** 0.5)
    return x, w1, b1, w2


def pool(*args, **kw):
    """ops.attn_pool on the fused launch (the dispatcher's default is the two launches: ops.FUSED_ATTN_POOL)."""
    return ops.attn_pool(*args, fused=True, **kw)


def _cuda(*ts):
    return [t.float().cuda().contiguous() for t in ts]


@pytest.mark.parametrize('T', [1, 4, 7, 32, 128])
@pytest.mark.parametrize('D,A', [(400, 400), (84, 64), (400, 64), (84, 400)])
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('split', [True, False])
def test_against_fp64(T, D, A, masked, split):
    n = 300 // T + 3
    x, w1, b1, w2 = _problem(n, T, D, A, seed=T + D + A)
    mask = None
    if masked:
        g = torch.Generator().manual_seed(T)
        mask = torch.rand(n * T, generator=g) < 0.7
        mask.view(n, T)[:, 0] = True
        if T > 1:
            mask.view(n, T)[1] = False                        # a fully masked sequence: the uniform softmax of additive_pool
    want = ref_pool(x, w1, b1, w2, n, T, mask)
    prev = ops.set_split_gemm(split)
    try:
        got = pool(*_cuda(x, w1, b1, w2), n, T, mask=None if mask is None else mask.cuda())
    finally:
        ops.set_split_gemm(prev)
    assert ops.attn_pool_fused(D, A, T, fused=True)
    e = rel_err(got.cpu().numpy(), want.numpy())
    assert e < KTOL, e


def test_device_count_and_strided_slot():
    """n_seq_dev below n_seq: sequences beyond it are left untouched; the output is one slot of a [n, 4, D] stack (ldo = 4 D)."""
    n, T, D, A = 40, 7, 400, 400
    x, w1, b1, w2 = _problem(n, T, D, A, seed=11)
    want = ref_pool(x, w1, b1, w2, n, T)
    stack = torch.full((n, 4, D), 7.0, device='cuda')
    live = 23
    pool(*_cuda(x, w1, b1, w2), n, T, out=stack[:, 1], n_seq_dev=torch.tensor([live], dtype=torch.int32, device='cuda'))
    got = stack.cpu()
    assert rel_err(got[:live, 1].numpy(), want[:live].numpy()) < KTOL
    assert torch.all(got[live:] == 7.0) and torch.all(got[:, 0] == 7.0) and torch.all(got[:, 2:] == 7.0)


@pytest.mark.parametrize('T', [1, 7, 32, 128])
def test_a_sequence_has_the_same_bits_in_any_tile_slot(T):
    """Sequence s computed among others (in some tile slot) and alone (slot 0 of a one-sequence launch): the same bits; a repeat run
    too."""
    n, D, A = 2 * (128 // T) + 5, 400, 400
    x, w1, b1, w2 = _cuda(*_problem(n, T, D, A, seed=21))
    w1p = ops.attn_pool_pack(w1)
    full = pool(x, w1, b1, w2, n, T, w1p=w1p)
    assert torch.equal(full, pool(x, w1, b1, w2, n, T, w1p=w1p))
    for s in (0, 1, n // 2, n - 1):
        one = pool(x[s * T:(s + 1) * T].contiguous(), w1, b1, w2, 1, T, w1p=w1p)
        assert torch.equal(one[0], full[s]), s


def test_graph_replay_sees_an_in_place_change_of_w1():
    n, T, D, A = 64, 32, 400, 400
    x, w1, b1, w2 = _cuda(*_problem(n, T, D, A, seed=31))
    out = torch.empty((n, D), device='cuda')
    pool(x, w1, b1, w2, n, T, out=out)                # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pool(x, w1, b1, w2, n, T, out=out)            # packs w1 inside the captured forward
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, pool(x, w1, b1, w2, n, T))
    w1.mul_(-0.5)
    g.replay()
    torch.cuda.synchronize()
    want = pool(x, w1, b1, w2, n, T)
    assert torch.equal(out, want)
    assert rel_err(out.cpu().numpy(), ref_pool(*[t.cpu().double() for t in (x, w1, b1, w2)], n, T).numpy()) < KTOL


def test_beyond_the_limits_is_the_two_launch_path():
    """T = 256 (and A > 512): linear(tanh) + additive_pool, bit for bit."""
    for n, T, D, A in ((6, 256, 400, 400), (20, 8, 84, 640)):
        assert not ops.attn_pool_fused(D, A, T, fused=True)
        x, w1, b1, w2 = _cuda(*_problem(n, T, D, A, seed=41))
        got = pool(x, w1, b1, w2, n, T)
        want = ops.additive_pool(ops.linear(x, w1, b1, act='tanh'), w2, x, n, T)
        assert torch.equal(got, want)
        assert rel_err(got.cpu().numpy(), ref_pool(*[t.cpu().double() for t in (x, w1, b1, w2)], n, T).numpy()) < KTOL


def test_the_default_dispatch_is_the_two_launch_path(monkeypatch):
    n, T, D, A = 50, 32, 400, 400
    x, w1, b1, w2 = _cuda(*_problem(n, T, D, A, seed=45))
    monkeypatch.setattr(ops, 'FUSED_ATTN_POOL', False)
    assert not ops.attn_pool_fused(D, A, T)
    want = ops.additive_pool(ops.linear(x, w1, b1, act='tanh'), w2, x, n, T)
    assert torch.equal(ops.attn_pool(x, w1, b1, w2, n, T), want)
    monkeypatch.setattr(ops, 'FUSED_ATTN_POOL', True)
    assert ops.attn_pool_fused(D, A, T)
    assert torch.equal(ops.attn_pool(x, w1, b1, w2, n, T), pool(x, w1, b1, w2, n, T))


def test_bad_arguments_are_refused_before_any_launch():
    n, T, D, A = 8, 4, 400, 64
    x, w1, b1, w2 = _cuda(*_problem(n, T, D, A, seed=51))
    with pytest.raises(ValueError):
        pool(x, w1, b1, w2, n + 1, T)                               # rows != n_seq T
    with pytest.raises(ValueError):
        pool(x, w1[:, :D - 4].contiguous(), b1, w2, n, T)           # W1 of another width
    with pytest.raises(ValueError):
        pool(x, w1, b1, w2, n, T, out=torch.empty((n, D + 1), device='cuda')[:, 1:])      # misaligned out
    with pytest.raises(ValueError):
        pool(x, w1, b1, w2, n, T, w1p=ops.attn_pool_pack(w1)[:-8])  # a packed buffer of another size
    with pytest.raises(ValueError):
        pool(x, w1, b1, w2, n, T, mask=torch.ones(n * T + 1, dtype=torch.bool, device='cuda'))
    with pytest.raises(TypeError):
        pool(x.cpu(), w1, b1, w2, n, T)
    lib = ops._lib.load()
    out = torch.empty((n, D), device='cuda')
    w1p = ops.attn_pool_pack(w1)
    # the C entry point itself: T > 128, A > 512, D % 4, a NULL operand
    for T_, D_, A_, xp in ((256, D, A, x), (T, D, 1024, x), (T, D - 2, A, x), (T, D, A, None)):
        rc = lib.lime_attn_pool_sp_f32(ops._p(xp), D, D_, ops._p(w1p), ops._p(b1), ops._p(w2), A_, None, ops._p(out), D, n, T_, None,
                                       ops._stream())
        assert rc != 0
    assert lib.lime_attn_pool_pack_sp_size(D, 1024) == 0
    with pytest.raises((ValueError, LimeHipError)):
        ops.attn_pool_pack(torch.zeros((A, D - 2), device='cuda'))
