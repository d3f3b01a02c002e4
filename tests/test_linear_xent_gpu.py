"""lime_linear_xent_f32 (csrc/linear_xent_f32.hip): the linear classifier and its cross-entropy in one launch, against a float64
statement written here, at the project's kernel bound KTOL = 2e-5 by helpers.rel_err.

    z = x w^T + b;  row_loss = scale (logsumexp(z) - z[target]);  dlogits = scale (softmax(z) - onehot(target));  dx = dlogits w

A target outside [0, C) is the all-zero one-hot row: exact zeros in row_loss, dlogits and dx.  The shapes: one row, fewer rows than a
workgroup's four waves, one more than 16 workgroups' worth, several passes of the grid's stride; D that is no multiple of 4 (the scalar
accesses), one float4 group, more than 64 groups a lane (400: two registers of x); C = 1 (the loss is exactly 0), C beyond one register
of logits a lane (65, 1024).  The issue's six (D, C) all keep w in LDS, so four more take the other routes: w beyond 64 KB read through
L2 with and without 16-byte accesses, and rows wider than 2048 columns, which are streamed instead of kept in registers."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import rel_err
from lime_cikm25_amd import _lib, ops

pytestmark = pytest.mark.gpu
KTOL = 2e-5

MS = [1, 3, 64, 65, 257]
SHAPES = [(4, 1), (6, 2), (36, 18), (400, 18), (20, 65), (8, 1024),
          (36, 512), (38, 500),          # w = 72 KB / 76 KB: read through L2, 16-byte and scalar accesses
          (2052, 2), (2051, 3)]          # 513 float4 groups: the row of x is streamed, 16-byte and scalar accesses
SCALE = 0.3 / 7.0


def problem(M, D, C, seed=0):
    """x as the left half of a [M, 2D] buffer and as its own tensor, w, b, and targets with -1 and C among them from three rows on."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * M + 13 * D + C)
    wide = torch.randn(M, 2 * D, generator=g)
    w = torch.randn(C, D, generator=g) / D ** 0.5
    b = torch.randn(C, generator=g)
    t = torch.randint(0, C, (M,), generator=g, dtype=torch.int32)
    if M >= 3:
        t[1], t[M - 1] = -1, C
    return wide, w, b, t


def statement(x, w, b, t, scale):
    """The contract in float64 -> (loss, row_loss [M], dlogits [M, C], dx [M, D])."""
    x, w = x.double(), w.double()
    z = x @ w.t() + (b.double() if b is not None else 0.0)
    C = w.shape[0]
    hit = (t >= 0) & (t < C)
    onehot = torch.zeros_like(z)
    onehot[hit, t[hit].long()] = 1.0
    lse = torch.logsumexp(z, dim=1)
    row = scale * (lse - (z * onehot).sum(1)) * hit
    d = scale * (torch.softmax(z, dim=1) - onehot) * hit[:, None]
    return row.sum(), row, d, d @ w


def run(x, w, b, t, scale=SCALE, want_grads=True):
    out = ops.linear_xent(x, w, b, t, scale, want_grads=want_grads)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('D,C', SHAPES)
@pytest.mark.parametrize('M', MS)
def test_against_the_float64_statement(M, D, C):
    wide, w, b, t = problem(M, D, C)
    wg, bg, tg = w.cuda(), b.cuda(), t.cuda()
    dense = wide[:, :D].contiguous().cuda()
    sliced = wide.cuda()[:, :D]                                            # ldx = 2 D: a column slice
    assert M == 1 or (dense.stride(0), sliced.stride(0)) == (D, 2 * D)
    miss = ~((t >= 0) & (t < C))
    assert M < 3 or int(miss.sum()) == 2
    for bias in (bg, None):
        want = statement(wide[:, :D], w, b if bias is not None else None, t, SCALE)
        got = {}
        for name, x in (('ldx = D', dense), ('ldx = 2 D', sliced)):
            loss, row, d, dx = run(x, wg, bias, tg)
            assert loss.shape == (1,) and row.shape == (M,) and d.shape == (M, C) and dx.shape == (M, D)
            errs = [rel_err(a.cpu().numpy(), r.numpy()) for a, r in zip((loss, row, d, dx), want)]
            print('M %d D %d C %d %s %s: loss %.2e row_loss %.2e dlogits %.2e dx %.2e' % (
                (M, D, C, name, 'bias' if bias is not None else 'no bias') + tuple(errs)))
            assert max(errs) < KTOL, errs
            # a row without a target: exact zeros
            assert (row.cpu()[miss] == 0).all() and (d.cpu()[miss] == 0).all() and (dx.cpu()[miss] == 0).all()
            if C == 1:
                assert float(loss) == 0.0 and (row == 0).all()
            got[name] = (loss, row, d, dx)
            # the loss alone: the same bits without the gradients
            loss2, row2, d2, dx2 = run(x, wg, bias, tg, want_grads=False)
            assert d2 is None and dx2 is None and torch.equal(loss2, loss) and torch.equal(row2, row)
        # the leading dimension changes no bit
        assert all(torch.equal(a, c) for a, c in zip(got['ldx = D'], got['ldx = 2 D']))


def test_a_single_row_without_a_target_is_all_zero():
    for D, C in ((36, 18), (6, 2), (20, 65)):
        wide, w, b, _ = problem(1, D, C)
        for t in (-1, C, -2 ** 31, 2 ** 31 - 1):
            loss, row, d, dx = run(wide[:, :D].contiguous().cuda(), w.cuda(), b.cuda(), torch.tensor([t], dtype=torch.int32).cuda())
            assert float(loss) == 0.0 and (row == 0).all() and (d == 0).all() and (dx == 0).all()


def test_an_unaligned_slice_takes_the_scalar_accesses():
    """D % 4 == 0 but x starts 4 bytes behind a 16-byte boundary: the same assignment of elements to lanes, the same bits."""
    M, D, C = 65, 36, 18
    wide, w, b, t = problem(M, D, C)
    shifted = torch.cat([torch.zeros(M, 1), wide], dim=1).cuda()[:, 1:1 + D]
    assert shifted.data_ptr() % 16 == 4
    a = run(wide[:, :D].contiguous().cuda(), w.cuda(), b.cuda(), t.cuda())
    c = run(shifted, w.cuda(), b.cuda(), t.cuda())
    assert all(torch.equal(p, q) for p, q in zip(a, c))


@pytest.mark.parametrize('D,C', [(400, 18), (6, 2), (20, 65), (36, 512), (2052, 2)])
def test_a_rows_bits_depend_on_neither_M_nor_its_place_nor_the_run(D, C):
    M = 257
    wide, w, b, t = problem(M, D, C, seed=1)
    x, wg, bg, tg = wide[:, :D].contiguous().cuda(), w.cuda(), b.cuda(), t.cuda()
    _, row, d, dx = run(x, wg, bg, tg)
    _, row_b, d_b, dx_b = run(x, wg, bg, tg)
    assert torch.equal(row, row_b) and torch.equal(d, d_b) and torch.equal(dx, dx_b)                 # two runs
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(5)).cuda()
    _, row_p, d_p, dx_p = run(x[perm].contiguous(), wg, bg, tg[perm].contiguous())
    assert torch.equal(row_p, row[perm]) and torch.equal(d_p, d[perm]) and torch.equal(dx_p, dx[perm])   # another place
    for r in (0, 2, 130, 255):                                                                          # alone, and in a smaller M
        _, row_1, d_1, dx_1 = run(x[r:r + 1].contiguous(), wg, bg, tg[r:r + 1].contiguous())
        assert torch.equal(row_1[0], row[r]) and torch.equal(d_1[0], d[r]) and torch.equal(dx_1[0], dx[r])
    _, row_s, d_s, dx_s = run(x[100:165].contiguous(), wg, bg, tg[100:165].contiguous())
    assert torch.equal(row_s, row[100:165]) and torch.equal(d_s, d[100:165]) and torch.equal(dx_s, dx[100:165])


def test_the_scalar_is_the_fixed_order_sum_of_the_rows():
    M, D, C = 257, 400, 18
    wide, w, b, t = problem(M, D, C, seed=2)
    loss, row, _, _ = run(wide[:, :D].contiguous().cuda(), w.cuda(), b.cuda(), t.cuda(), scale=0.3 / M)
    assert torch.equal(loss, ops.colsum(row.view(M, 1)))
    hit = (t >= 0) & (t < C)                                               # all but rows 1 and M - 1
    want = torch.nn.functional.cross_entropy((wide[:, :D].double() @ w.double().t() + b.double())[hit], t[hit].long(),
                                             reduction='sum') * 0.3 / M
    assert abs(float(loss) - float(want)) < KTOL * float(want)


def test_refusals_come_before_any_launch():
    lib = _lib.load()
    M, D, C = 5, 8, 3
    x = torch.randn(M, D).cuda()
    w = torch.randn(C, D).cuda()
    t = torch.zeros(M, dtype=torch.int32).cuda()
    outs = [torch.full((M,), float('nan')).cuda(), torch.full((M, C), float('nan')).cuda(), torch.full((M, D), float('nan')).cuda()]
    p = lambda v: ctypes.c_void_p(v.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(M=M, D=D, C=C, ldx=D, lddx=D, x=x, row=outs[0]):
        return lib.lime_linear_xent_f32(p(x) if x is not None else None, ldx, p(w), None, p(t), 1.0, p(row) if row is not None else None,
                                        p(outs[1]), p(outs[2]), lddx, M, D, C, s)

    bad, unsupported = _lib.CONSTANTS['LIME_ERR_BAD_ARG'], _lib.CONSTANTS['LIME_ERR_UNSUPPORTED']
    assert (bad, unsupported) == (-1, -2)
    assert call(M=0) == bad and call(C=0) == bad and call(D=0) == bad and call(M=-1) == bad
    assert call(ldx=D - 1) == bad and b'ldx' in lib.lime_last_error_string()
    assert call(lddx=D - 1) == bad
    assert call(x=None) == bad and call(row=None) == bad
    assert call(C=1025) == unsupported and b'1025' in lib.lime_last_error_string()
    torch.cuda.synchronize()
    assert all(torch.isnan(o).all() for o in outs), 'a refused call wrote an output'
    assert call() == 0
    torch.cuda.synchronize()
    assert all(torch.isfinite(o).all() for o in outs)


def test_the_wrapper_checks_on_the_host():
    x, w, t = torch.randn(4, 8).cuda(), torch.randn(3, 8).cuda(), torch.zeros(4, dtype=torch.int32).cuda()
    with pytest.raises(ValueError, match='columns'):
        ops.linear_xent(x, torch.randn(3, 9).cuda(), None, t, 1.0)
    with pytest.raises(ValueError, match='C <= 1024'):
        ops.linear_xent(x, torch.randn(1025, 8).cuda(), None, torch.zeros(4, dtype=torch.int32).cuda(), 1.0)
    with pytest.raises(ValueError, match='M >= 1'):
        ops.linear_xent(x[:0], w, None, t[:0], 1.0)
    with pytest.raises(TypeError, match='int32'):
        ops.linear_xent(x, w, None, t.long(), 1.0)
    with pytest.raises(ValueError, match='elements'):
        ops.linear_xent(x, w, None, t[:3], 1.0)
    with pytest.raises(ValueError, match='elements'):
        ops.linear_xent(x, w, torch.zeros(4).cuda(), t, 1.0)
    with pytest.raises(TypeError):
        ops.linear_xent(x.double(), w, None, t, 1.0)
    with pytest.raises(ValueError, match='unit column stride'):
        ops.linear_xent(torch.randn(8, 4).cuda().t(), w, None, t, 1.0)
