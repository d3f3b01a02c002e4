"""The KCNN kernels on the MI355X (csrc/conv_pool_sp_f32.hip): lime_conv_pool_f32 (convolution over up to three sources + ReLU + max
pool in one launch), lime_relu_maxpool_f32 (the same pooling from dense pre-activations) and lime_relu_maxpool_bwd_f32, against a torch
fp64 statement of the formula on the CPU (F.conv2d on the stacked sources, ReLU, sliced max).

Bounds: the forward against fp64 at KTOL = 2e-5 by ``rel_err``, what tests/test_cnn_gpu.py asks of conv1d_window (the same arithmetic);
fused against unfused at the same KTOL (the same sums in another order, tests/test_user_encoders_gpu.py); the whole backward at
TOL = 1e-3.  The weights are scaled so that the pre-activations have unit variance: a position ``arg`` is compared wherever the two
largest pre-activations of the sequence (and the largest and zero) are more than KTOL apart."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import rel_err
from lime_cikm25_amd import _lib, ops
from lime_cikm25_amd import training as TR

pytestmark = pytest.mark.gpu
TOL = 1e-3
KTOL = 2e-5


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale


def ref_pre(xs, w, b, T, p):
    """fp64 pre-activations [n, O, T]: nn.Conv2d(C, O, [win, n_src]) over the [n, C, T, n_src] stack of the sources, p zero rows in front
    and win - 1 - p behind (the reference's padding plus the zero row it appends for the even windows)."""
    n = xs[0].shape[0] // T
    win = w.shape[2]
    feat = torch.stack(xs, dim=2).view(n, T, -1, len(xs)).permute(0, 2, 1, 3)
    feat = F.pad(feat, (0, 0, p, win - 1 - p))
    return F.conv2d(feat, w, b)[..., 0]


def ref_pool(pre, P):
    """-> pooled [n, O], arg [n, O] (first position of the maximum, -1 where pooled is 0), sure [n, O] (the position is decided by more
    than KTOL: against the runner-up and against zero)."""
    act = pre[:, :, :P]
    best, at = act.max(dim=2)
    first = (act == best.unsqueeze(2)).double().argmax(dim=2)           # the smallest t attaining the maximum
    pooled = best.clamp(min=0)
    arg = torch.where(best > 0, first, torch.full_like(first, -1))
    if P > 1:
        top2 = act.topk(2, dim=2).values
        gap = top2[..., 0] - top2[..., 1]
    else:
        gap = torch.full_like(best, float('inf'))
    sure = (best.abs() > KTOL) & ((gap > KTOL) | (best <= 0))
    return pooled, arg, sure


def make_problem(n_seq, T, N, C, n_src, win, gathered, seed, V=53):
    """-> (xs fp64 dense sources, device sources [(a, ids)], w fp64 [N, C, win, n_src], b fp64).  Row 0 of every table is NOT zero:
    out-of-range taps must read zeros, not row 0."""
    M = n_seq * T
    xs, src = [], []
    g = torch.Generator().manual_seed(seed)
    for s in range(n_src):
        if gathered[s]:
            table = rnd(V, C, seed=seed + 10 + s)
            ids = torch.randint(0, V, (M,), generator=g, dtype=torch.int32)
            ids[::3] = 0
            xs.append(table[ids.long()])
            src.append((table.float().cuda(), ids.cuda()))
        else:
            x = rnd(M, C, seed=seed + 20 + s)
            xs.append(x)
            src.append((x.float().cuda(), None))
    w = rnd(N, C, win, n_src, seed=seed + 1, scale=3.0 / math.sqrt(n_src * win * C))
    b = rnd(N, seed=seed + 2, scale=0.5)
    return xs, src, w, b


def check_pool(got, got_arg, pre, P, what):
    pooled, arg, sure = ref_pool(pre, P)
    e = rel_err(got.cpu().numpy(), pooled.numpy())
    print('%s: pooled vs fp64 %.2e' % (what, e))
    assert e < KTOL, (what, e)
    if got_arg is not None:
        ga = got_arg.cpu().long()
        assert int(ga.min()) >= -1 and int(ga.max()) < P
        assert torch.equal(ga[sure], arg[sure]), what
    return pooled, arg, sure


# (n_seq, T, N, C, n_src, win, pad, P, gathered): the five (win, pad) pairs of Conv2D_Pool with their P, T in {1, 8, 30, 32, 128}, n_seq in
# {1, 5, 37} (37 sequences of 8 tokens cross the 16-sequence tile), N in {4, 100, 132, 400} (132 crosses the column tile), C in {20, 300}
# (300 is no whole number of 32-deep chunks), 1 and 3 sources, gathered and dense mixed
CASES = [
    (5, 1, 4, 20, 1, 1, 0, 1, (True,)),
    (37, 8, 132, 300, 3, 3, 1, 6, (True, True, True)),
    (37, 8, 100, 20, 3, 2, 0, 7, (True, False, True)),
    (5, 30, 100, 300, 3, 4, 1, 27, (True, True, False)),
    (5, 30, 132, 20, 1, 5, 2, 26, (False,)),
    (37, 32, 400, 300, 3, 3, 1, 30, (True, True, True)),
    (5, 32, 100, 300, 3, 1, 0, 32, (False, True, True)),
    (1, 32, 4, 300, 3, 2, 0, 31, (True, True, True)),
    (1, 128, 132, 20, 3, 5, 2, 124, (True, False, False)),
    (5, 128, 100, 300, 1, 3, 1, 126, (True,)),
    (37, 30, 400, 20, 3, 4, 1, 27, (False, False, False)),
]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'n%d_T%d_N%d_C%d_s%d_w%d' % c[:6])
def test_fused_and_unfused_against_fp64(case):
    n_seq, T, N, C, n_src, win, pad, P, gathered = case
    xs, src, w, b = make_problem(n_seq, T, N, C, n_src, win, gathered, seed=100 + T + N)
    pre = ref_pre(xs, w, b, T, pad)
    wp, bc = ops.conv_pool_pack(w.float().cuda()), b.float().cuda()
    fused, farg = ops.conv_pool(src, wp, win, pad, P, T, bias=bc, want_arg=True, fused=True)
    pooled, arg, sure = check_pool(fused, farg, pre, P, 'fused')
    plain, parg = ops.conv_pool(src, wp, win, pad, P, T, bias=bc, want_arg=True, fused=False)
    check_pool(plain, parg, pre, P, 'unfused')
    e = rel_err(fused.cpu().numpy(), plain.cpu().numpy())
    print('fused vs unfused %.2e' % e)
    assert e < KTOL, e
    assert torch.equal(farg.cpu()[sure], parg.cpu()[sure])
    # without the positions, and once more: the same bits
    again = ops.conv_pool(src, wp, win, pad, P, T, bias=bc, fused=True)
    assert torch.equal(again, fused)
    again2, aarg2 = ops.conv_pool(src, wp, win, pad, P, T, bias=bc, want_arg=True, fused=True)
    assert torch.equal(again2, fused) and torch.equal(aarg2, farg)


def test_exact_fp32_mfma_form():
    """lime_set_split_gemm(0): the same kernel on the fp32 matrix cores."""
    n_seq, T, N, C, n_src, win, pad, P = 9, 30, 132, 300, 3, 3, 1, 28
    xs, src, w, b = make_problem(n_seq, T, N, C, n_src, win, (True, False, True), seed=7)
    pre = ref_pre(xs, w, b, T, pad)
    prev = ops.set_split_gemm(False)
    try:
        got, arg = ops.conv_pool(src, ops.conv_pool_pack(w.float().cuda()), win, pad, P, T, bias=b.float().cuda(), want_arg=True, fused=True)
    finally:
        ops.set_split_gemm(prev)
    check_pool(got, arg, pre, P, 'fp32 mfma')


def test_negative_columns_pool_to_zero_without_a_position():
    n_seq, T, N, C, n_src, win, pad, P = 5, 8, 100, 20, 3, 3, 1, 6
    xs, src, w, b = make_problem(n_seq, T, N, C, n_src, win, (True, True, True), seed=11)
    b[::7] = -1000.0                                                   # every pre-activation of these columns is negative
    wp, bc = ops.conv_pool_pack(w.float().cuda()), b.float().cuda()
    for fused in (True, False):
        got, arg = ops.conv_pool(src, wp, win, pad, P, T, bias=bc, want_arg=True, fused=fused)
        assert torch.all(got[:, ::7] == 0) and torch.all(arg[:, ::7] == -1)
        assert torch.all((arg >= 0) == (got > 0))


def test_exact_ties_take_the_smallest_position():
    """Identical rows under a window of one give identical pre-activations at every position: the position is 0 wherever the pooled value
    is positive; with positions 0 and 1 pushed below the rest, it is 2."""
    n_seq, T, N, C = 6, 8, 100, 20
    row = rnd(n_seq, 1, C, seed=21)
    x = row.expand(n_seq, T, C).reshape(n_seq * T, C).contiguous()
    w, b = rnd(N, C, 1, 1, seed=22, scale=0.5), rnd(N, seed=23, scale=0.2)
    wp, bc = ops.conv_pool_pack(w.float().cuda()), b.float().cuda()
    low = x.view(n_seq, T, C).clone()
    low[:, :2] = 0.0                                                   # positions 0 and 1: the bias alone
    for fused in (True, False):
        got, arg = ops.conv_pool([(x.float().cuda(), None)], wp, 1, 0, T, T, bias=bc, want_arg=True, fused=fused)
        assert bool((got > 0).any()) and bool((got == 0).any())
        assert torch.all(arg[got > 0] == 0) and torch.all(arg[got == 0] == -1)
        got2, arg2 = ops.conv_pool([(low.view(-1, C).float().cuda(), None)], wp, 1, 0, T, T, bias=bc, want_arg=True, fused=fused)
        pre = ref_pre([low.view(-1, C)], w, b, T, 0)
        later = (pre[:, :, 2] > pre[:, :, 0] + 1e-3) & (pre[:, :, 2] > 1e-3)
        assert bool(later.any()) and torch.all(arg2.cpu()[later] == 2)


def test_device_sequence_count_leaves_the_rest_untouched():
    n_seq, T, N, C, n_src, win, pad, P = 37, 8, 100, 20, 3, 3, 1, 6
    xs, src, w, b = make_problem(n_seq, T, N, C, n_src, win, (True, False, True), seed=31)
    pre = ref_pre(xs, w, b, T, pad)
    wp, bc = ops.conv_pool_pack(w.float().cuda()), b.float().cuda()
    for live in (21, 16, 0):                                           # inside a tile, on a tile edge, nothing
        count = torch.tensor([live], dtype=torch.int32, device='cuda')
        for fused in (True, False):
            big = torch.full((n_seq, 3 * N), 7.0, device='cuda')
            barg = torch.full((n_seq, N), 99, dtype=torch.int32, device='cuda')
            ops.conv_pool(src, wp, win, pad, P, T, bias=bc, out=big[:, N:2 * N], arg=barg, n_seq_dev=count, fused=fused)
            if live:
                check_pool(big[:live, N:2 * N], barg[:live], pre[:live], P, 'count %d' % live)
            assert torch.all(big[live:] == 7.0) and torch.all(big[:, :N] == 7.0) and torch.all(big[:, 2 * N:] == 7.0)
            assert torch.all(barg[live:] == 99)


def test_a_sequence_has_the_same_bits_wherever_it_sits():
    n_seq, T, N, C, n_src, win, pad, P = 37, 8, 132, 300, 3, 3, 1, 6
    V = 53
    tables = [rnd(V, C, seed=40 + s).float().cuda() for s in range(n_src)]
    g = torch.Generator().manual_seed(41)
    ids = [torch.randint(0, V, (n_seq, T), generator=g, dtype=torch.int32) for _ in range(n_src)]
    w, b = rnd(N, C, win, n_src, seed=42, scale=0.05), rnd(N, seed=43)
    wp, bc = ops.conv_pool_pack(w.float().cuda()), b.float().cuda()
    run = lambda rows: ops.conv_pool([(tables[s], ids[s][rows].reshape(-1).contiguous().cuda()) for s in range(n_src)], wp, win, pad, P, T,
                                     bias=bc, want_arg=True, fused=True)
    full, full_arg = run(torch.arange(n_seq))
    k = 19                                                             # slot 3 of the second tile
    alone, alone_arg = run(torch.tensor([k]))
    assert torch.equal(alone[0], full[k]) and torch.equal(alone_arg[0], full_arg[k])
    other = torch.tensor([30, 2, k, 5, 11])                            # another batch, another slot
    moved, moved_arg = run(other)
    assert torch.equal(moved[2], full[k]) and torch.equal(moved_arg[2], full_arg[k])
    assert torch.equal(moved[0], full[30]) and torch.equal(moved[4], full[11])


# The edges of the shared tile product (csrc/conv_frag.h conv_tile_product) as conv_pool_sp_kernel drives it: T = 12 puts 10 whole
# sequences into a 128-row tile and leaves 8 tile rows dead, 11 sequences leave one for the second tile, C = 36 masks most of the second
# chunk, N = 132 makes a second column block of 4; the tap walks one gathered source or a gathered and two dense ones, each with a
# leading dimension of its own.
EDGE = dict(n_seq=11, T=12, N=132, C=36, V=29)
EDGE_LDA = (36, 40, 44)


def edge_sources(n_src, order):
    """-> (fp64 dense sources, device (a, ids) pairs) with the sequences in ``order``."""
    n_seq, T, C, V = EDGE['n_seq'], EDGE['T'], EDGE['C'], EDGE['V']
    g = torch.Generator().manual_seed(301)
    table = rnd(V, C, seed=302)
    ids = torch.randint(0, V, (n_seq, T), generator=g, dtype=torch.int32)
    ids[:, ::3] = 0
    ids = ids[order].reshape(-1).contiguous()
    xs, src = [table[ids.long()]], [(table.float().cuda(), ids.cuda())]
    for s in range(1, n_src):
        x = rnd(n_seq, T, C, seed=302 + s)[order].reshape(-1, C)
        buf = torch.full((n_seq * T, EDGE_LDA[s]), 9.0, device='cuda')
        buf[:, :C] = x.float().cuda()
        xs.append(x)
        src.append((buf[:, :C], None))
    return xs, src


def run_edge_pool(n_src, win, pad, split, order=None, live=None):
    """One fused launch on the edge problem -> pooled, arg (filled with 7.0 / 99 first), the fp64 pre-activations, P."""
    n_seq, T, N, C = EDGE['n_seq'], EDGE['T'], EDGE['N'], EDGE['C']
    P = T - win + 1
    xs, src = edge_sources(n_src, torch.arange(n_seq) if order is None else order)
    w = rnd(N, C, win, n_src, seed=310 + win, scale=3.0 / math.sqrt(n_src * win * C))
    b = rnd(N, seed=311, scale=0.5)
    out = torch.full((n_seq, N), 7.0, device='cuda')
    arg = torch.full((n_seq, N), 99, dtype=torch.int32, device='cuda')
    count = None if live is None else torch.tensor([live], dtype=torch.int32, device='cuda')
    prev = ops.set_split_gemm(split)
    try:
        ops.conv_pool(src, ops.conv_pool_pack(w.float().cuda()), win, pad, P, T, bias=b.float().cuda(), out=out, arg=arg, n_seq_dev=count,
                      fused=True)
    finally:
        ops.set_split_gemm(prev)
    return out, arg, ref_pre(xs, w, b, T, pad), P


@pytest.mark.parametrize('split', [True, False])
@pytest.mark.parametrize('win,pad', [(2, 0), (2, 1), (3, 1)])
@pytest.mark.parametrize('n_src', [1, 3])
def test_fused_tile_edges(n_src, win, pad, split):
    n_seq = EDGE['n_seq']
    full, full_arg, pre, P = run_edge_pool(n_src, win, pad, split)
    check_pool(full, full_arg, pre, P, 'edge')
    # a device count of 10: the second tile returns, sequence 10 keeps what it held, the position included
    part, part_arg = run_edge_pool(n_src, win, pad, split, live=10)[:2]
    assert torch.equal(part[:10], full[:10]) and torch.equal(part_arg[:10], full_arg[:10])
    assert torch.all(part[10] == 7.0) and torch.all(part_arg[10] == 99)
    # the batch in reverse order: every sequence in another tile slot, the last one now first -- the same bits
    back, back_arg = run_edge_pool(n_src, win, pad, split, order=torch.arange(n_seq - 1, -1, -1))[:2]
    assert torch.equal(back.flip(0), full) and torch.equal(back_arg.flip(0), full_arg)


def test_long_sequences_take_the_unfused_form():
    n_seq, T, N, C, n_src, win, pad, P = 3, 130, 36, 20, 3, 3, 1, 128
    xs, src, w, b = make_problem(n_seq, T, N, C, n_src, win, (True, False, True), seed=51)
    pre = ref_pre(xs, w, b, T, pad)
    wp, bc = ops.conv_pool_pack(w.float().cuda()), b.float().cuda()
    got, arg = ops.conv_pool(src, wp, win, pad, P, T, bias=bc, want_arg=True)
    check_pool(got, arg, pre, P, 'T = 130')
    with pytest.raises(ValueError, match='T = 130'):
        ops.conv_pool(src, wp, win, pad, P, T, bias=bc, fused=True)


@pytest.mark.parametrize('n_seq,T,P,N', [(1, 1, 1, 4), (37, 8, 6, 100), (5, 30, 27, 132), (3, 128, 128, 400)])
def test_pool_and_its_backward_against_fp64_autograd(n_seq, T, P, N):
    pre = rnd(n_seq * T, N, seed=61 + T).requires_grad_(True)
    b = rnd(N, seed=62, scale=0.3)
    dpooled = rnd(n_seq, N, seed=63)
    act = torch.relu(pre.view(n_seq, T, N) + b)[:, :P]
    pooled = act.max(dim=1).values
    (pooled * dpooled).sum().backward()
    wide = torch.full((n_seq * T, N + 8), 5.0, device='cuda')
    wide[:, 4:N + 4] = pre.detach().float().cuda()
    got, arg = ops.relu_maxpool(wide[:, 4:N + 4], n_seq, T, P, bias=b.float().cuda(), want_arg=True)
    assert rel_err(got.cpu().numpy(), pooled.detach().numpy()) < 1e-6
    dwide = torch.full((n_seq * T, N + 8), 3.0, device='cuda')
    ops.relu_maxpool_bwd(dpooled.float().cuda(), arg, T, out=dwide[:, 4:N + 4])
    want = pre.grad.float()
    assert torch.equal(dwide[:, 4:N + 4].cpu(), torch.where(want != 0, dpooled.float().repeat_interleave(T, dim=0), torch.zeros(())))
    assert torch.all(dwide[:, :4] == 3.0) and torch.all(dwide[:, N + 4:] == 3.0)
    assert torch.equal(ops.relu_maxpool_bwd(dpooled.float().cuda(), arg, T), dwide[:, 4:N + 4])


@pytest.mark.parametrize('specs,T,C,per', [(((3, 1, 14),), 16, 300, 100), (((1, 0, 8), (2, 0, 7), (3, 1, 6), (4, 1, 5)), 8, 20, 36),
                                          (((5, 2, 26),), 30, 300, 132)])
def test_conv_pool_backward_against_fp64_autograd(specs, T, C, per):
    """training._ConvPool (kernel 1 forward, kernel 3 + the windowed weight / data gradient kernels backward): dW, dbias and the three
    dX against the autograd of the fp64 statement."""
    n_seq = 13
    xs = [rnd(n_seq * T, C, seed=71 + s).requires_grad_(True) for s in range(3)]
    ws = [rnd(per, C, win, 3, seed=80 + i, scale=3.0 / math.sqrt(3 * win * C)).requires_grad_(True) for i, (win, _, _) in enumerate(specs)]
    bs = [rnd(per, seed=90 + i, scale=0.5).requires_grad_(True) for i in range(len(specs))]
    dout = rnd(n_seq, per * len(specs), seed=99)
    want = torch.cat([torch.relu(ref_pre(xs, w, b, T, pad))[:, :, :P].max(dim=2).values for w, b, (_, pad, P) in zip(ws, bs, specs)], dim=1)
    (want * dout).sum().backward()
    dev = lambda t: t.detach().float().cuda().requires_grad_(True)
    dxs, params = [dev(x) for x in xs], []
    for w, b in zip(ws, bs):
        params += [dev(w), dev(b)]
    got = TR._ConvPool.apply(*dxs, T, specs, *params)
    assert rel_err(got.detach().cpu().numpy(), want.detach().numpy()) < KTOL
    (got * dout.float().cuda()).sum().backward()
    worst = 0.0
    for mine, ref in zip(dxs + params, xs + [t for pair in zip(ws, bs) for t in pair]):
        assert mine.grad is not None and mine.grad.shape == ref.grad.shape
        worst = max(worst, rel_err(mine.grad.cpu().numpy(), ref.grad.numpy()))
    print('conv-pool backward vs fp64: worst %.2e' % worst)
    assert worst < TOL, worst


def test_pack_is_the_conv2d_layout():
    w = rnd(8, 12, 4, 3, seed=5).float().cuda()
    want = torch.einsum('ocjs->osjc', w).reshape(8, -1)
    assert torch.equal(ops.conv_pool_pack(w), want)


def test_arguments_are_checked_before_any_launch():
    lib = _lib.load()
    x = torch.zeros(16, 20, device='cuda')
    w = torch.zeros(8, 3 * 20, device='cuda')
    good = dict(sources=[(x, None)], w=w, window=3, pad=1, P=6, T=8)
    ops.conv_pool(**good, fused=True)
    for bad in (dict(T=5), dict(window=9), dict(window=0), dict(P=9), dict(P=0), dict(pad=3), dict(w=w[:, :40].contiguous()),
                dict(w=torch.zeros(6, 60, device='cuda')), dict(sources=[]), dict(sources=[(x, None)] * 4),
                dict(sources=[(x[:, :18].contiguous(), None)], w=torch.zeros(8, 54, device='cuda')),
                dict(sources=[(x, None), (torch.zeros(8, 20, device='cuda'), None)], w=torch.zeros(8, 120, device='cuda'))):
        with pytest.raises(ValueError):
            ops.conv_pool(**dict(good, **bad), fused=True)
    with pytest.raises(TypeError):
        ops.conv_pool([(x.cpu(), None)], w, 3, 1, 6, 8)
    # the C entry points themselves
    out = torch.full((2, 8), 7.0, device='cuda')

    def args(**over):
        a = _lib.ConvPoolArgs()
        a.a[0], a.lda[0] = x.data_ptr(), 20
        a.w, a.ldw, a.pooled, a.ldp = w.data_ptr(), 60, out.data_ptr(), 8
        a.n_seq, a.T, a.N, a.C, a.n_src, a.window, a.pad, a.P = 2, 8, 8, 20, 1, 3, 1, 6
        for k, v in over.items():
            if k in ('lda0',):
                a.lda[0] = v
            else:
                setattr(a, k, v)
        return ctypes.byref(a)

    assert lib.lime_conv_pool_f32(None, None) == -1
    for over, code in ((dict(n_src=0), -1), (dict(n_src=4), -1), (dict(T=129), -2), (dict(window=9), -1), (dict(P=0), -1), (dict(pad=3), -1),
                       (dict(C=18), -2), (dict(N=6), -2), (dict(ldw=59), -1), (dict(ldp=4), -1), (dict(lda0=16), -1), (dict(w=None), -1),
                       (dict(w=w.data_ptr() + 4), -2), (dict(n_seq=0), -1)):
        assert lib.lime_conv_pool_f32(args(**over), None) == code, over
        assert b'lime_conv_pool_f32' in lib.lime_last_error_string()
    assert lib.lime_relu_maxpool_f32(None, 8, None, None, 8, None, 0, 2, 8, 6, 8, None, None) == -1
    assert lib.lime_relu_maxpool_f32(x.data_ptr(), 20, None, out.data_ptr(), 8, None, 0, 2, 8, 9, 8, None, None) == -1
    assert lib.lime_relu_maxpool_f32(x.data_ptr(), 20, None, out.data_ptr(), 8, None, 0, 2, 8, 6, 6, None, None) == -2
    assert lib.lime_relu_maxpool_bwd_f32(None, 8, None, 8, None, 8, 2, 8, 8, None) == -1
    assert lib.lime_relu_maxpool_bwd_f32(out.data_ptr(), 8, out.data_ptr(), 8, x.data_ptr(), 6, 2, 8, 8, None) == -1
    torch.cuda.synchronize()
    assert torch.all(out == 7.0)
