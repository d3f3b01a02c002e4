"""lime_pool_match_f32 (csrc/user_pool_match_f32.hip, ops.pool_match) on the MI355X: against an fp64 torch statement of the same sums,
the same bits for a row in any batch (both launch forms) and on a repeat run, the two-launch form of the same function, and argument
checks that return an error code before any launch."""
import ctypes

import pytest
import torch

from helpers import rel_err
from lime_cikm25_amd import _lib, ops

pytestmark = pytest.mark.gpu
KTOL = 2e-5                     # kernel level against fp64, as tests/test_attn_pool_gpu.py


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale


def _problem(B, N, H, A, D, seed, masked=False):
    hidden = torch.tanh(rnd(B * H, A, seed=seed, scale=2.0))
    w2 = rnd(A, seed=seed + 1, scale=4.0 / A ** 0.5)
    x = rnd(B * H, D, seed=seed + 2)
    cand = rnd(B, N, D, seed=seed + 3)
    remaining = rnd(B, N, seed=seed + 4, scale=30.0)
    remaining.view(-1)[::5] = 0.0
    mask = None
    if masked:
        g = torch.Generator().manual_seed(seed + 5)
        mask = torch.rand(B, H, generator=g) < 0.6
        mask[min(1, B - 1)] = False                            # a fully masked row: the uniform softmax
    return hidden, w2, x, cand, remaining, mask


def ref(hidden, w2, x, cand, remaining, mask, B, H, alpha, beta, use_weight, use_penalty):
    """fp64: layers.py:288-299 from the tanh hidden state, then util.py:23-49."""
    s = (hidden @ w2).view(B, H)
    if mask is not None:
        s = s.masked_fill(~mask, -1e9)
    u = (torch.softmax(s, dim=1).unsqueeze(2) * x.view(B, H, -1)).sum(dim=1)
    base = (u.unsqueeze(1) * cand).sum(dim=-1)
    if use_weight:
        if use_penalty:
            w = torch.sigmoid(alpha * remaining)
            w = (remaining >= 0).double() * w + (remaining < 0).double() * beta * w
        else:
            w = torch.sigmoid(alpha * remaining.abs())
        base = base * w
    return u, base


def f32(*ts):
    return [None if t is None else (t.cuda() if t.dtype == torch.bool else t.float().cuda().contiguous()) for t in ts]


ALPHA, BETA = 0.05, 0.3


@pytest.mark.parametrize('H', [1, 10, 50, 64, 200, 512])
@pytest.mark.parametrize('N', [1, 5, 100])
@pytest.mark.parametrize('masked', [False, True])
def test_against_fp64(H, N, masked):
    B, A, D = (2100 if H <= 10 and N <= 5 else 9), 400, 400    # 2100 rows: the wave-per-row form; 9: a workgroup per row
    p = _problem(B, N, H, A, D, seed=H + N, masked=masked)
    d = f32(*p)
    for use_weight, use_penalty in ((True, True), (True, False), (False, False)):
        wu, wl = ref(*p, B, H, ALPHA, BETA, use_weight, use_penalty)
        u, l = ops.pool_match(d[0], d[1], d[2], B, H, cand=d[3], remaining=d[4], alpha=ALPHA, beta=BETA, use_weight=use_weight,
                              use_penalty=use_penalty, mask=d[5], fused=True)
        eu, el = rel_err(u.cpu().numpy(), wu.numpy()), rel_err(l.cpu().numpy(), wl.numpy())
        print('H %d N %d masked %s weight %s penalty %s: user %.2e logits %.2e' % (H, N, masked, use_weight, use_penalty, eu, el))
        assert eu < KTOL and el < KTOL, (eu, el)


@pytest.mark.parametrize('B', [5, 2100])
def test_either_output_may_be_left_out(B):
    N, H, A, D = 3, 50, 400, 400
    d = f32(*_problem(B, N, H, A, D, seed=3, masked=True))
    kw = dict(cand=d[3], remaining=d[4], alpha=ALPHA, beta=BETA, use_weight=True, use_penalty=True, mask=d[5], fused=True)
    u, l = ops.pool_match(d[0], d[1], d[2], B, H, **kw)
    u2, none = ops.pool_match(d[0], d[1], d[2], B, H, want_logits=False, mask=d[5], fused=True)
    none2, l2 = ops.pool_match(d[0], d[1], d[2], B, H, want_user=False, **kw)
    assert none is None and none2 is None
    assert torch.equal(u, u2) and torch.equal(l, l2)


@pytest.mark.parametrize('A,D', [(400, 400), (64, 84), (30, 20), (401, 400)])
def test_other_widths_and_strided_operands(A, D):
    """A not a multiple of 4 (element-wise loads of hidden / w2) and row-strided views of wider buffers."""
    B, N, H = 7, 2, 13
    p = _problem(B, N, H, A, D, seed=A + D)
    wu, wl = ref(*p, B, H, ALPHA, BETA, True, True)
    d = f32(*p)
    wide_h = torch.zeros((B * H, A + 8), device='cuda')
    wide_h[:, :A] = d[0]
    wide_x = torch.zeros((B * H, D + 12), device='cuda')
    wide_x[:, 4:4 + D] = d[2]
    for hid, x in ((d[0], d[2]), (wide_h[:, :A], wide_x[:, 4:4 + D])):
        u, l = ops.pool_match(hid, d[1], x, B, H, cand=d[3], remaining=d[4], alpha=ALPHA, beta=BETA, use_weight=True, use_penalty=True,
                              fused=True)
        assert rel_err(u.cpu().numpy(), wu.numpy()) < KTOL and rel_err(l.cpu().numpy(), wl.numpy()) < KTOL


@pytest.mark.parametrize('H,N', [(50, 1), (50, 5), (7, 3), (512, 2)])
def test_a_row_has_the_same_bits_in_any_batch(H, N):
    """The same row in a batch of 1, 7 (a workgroup per row) and 4096 rows (a wave per row), and on a second run."""
    A, D = 400, 400
    big = 4096
    g = torch.Generator(device='cuda').manual_seed(H * 3 + N)                  # fp32 operands made on the device (6.7 GB at H = 512)
    r = lambda *shape: torch.rand(*shape, generator=g, device='cuda') * 2 - 1
    d = [torch.tanh(2 * r(big * H, A)), r(A) * 0.2, r(big * H, D), r(big, N, D), r(big, N) * 30, torch.rand(big, H, generator=g, device='cuda') < 0.6]
    d[5][1] = False
    run = lambda r0, n: ops.pool_match(d[0][r0 * H:(r0 + n) * H], d[1], d[2][r0 * H:(r0 + n) * H], n, H, cand=d[3][r0:r0 + n],
                                       remaining=d[4][r0:r0 + n], alpha=ALPHA, beta=BETA, use_weight=True, use_penalty=True,
                                       mask=d[5][r0:r0 + n], fused=True)
    u_all, l_all = run(0, big)
    u_again, l_again = run(0, big)
    assert torch.equal(u_all, u_again) and torch.equal(l_all, l_again)
    for r in (0, 1, 2050, big - 1):
        u1, l1 = run(r, 1)
        assert torch.equal(u1[0], u_all[r]) and torch.equal(l1[0], l_all[r]), r
    for r0 in (0, 1001, big - 7):
        u7, l7 = run(r0, 7)
        assert torch.equal(u7, u_all[r0:r0 + 7]) and torch.equal(l7, l_all[r0:r0 + 7]), r0


def test_the_bits_do_not_depend_on_the_candidate_count():
    B, H, A, D = 6, 50, 400, 400
    d = f32(*_problem(B, 100, H, A, D, seed=77))
    kw = dict(alpha=ALPHA, beta=BETA, use_weight=True, use_penalty=True, fused=True)
    u100, l100 = ops.pool_match(d[0], d[1], d[2], B, H, cand=d[3], remaining=d[4], **kw)
    u3, l3 = ops.pool_match(d[0], d[1], d[2], B, H, cand=d[3][:, :3].contiguous(), remaining=d[4][:, :3].contiguous(), **kw)
    assert torch.equal(u100, u3) and torch.equal(l100[:, :3], l3)


@pytest.mark.parametrize('B,N', [(32, 5), (2048, 1)])
def test_two_launch_form_agrees(B, N):
    H, A, D = 50, 400, 400
    d = f32(*_problem(B, N, H, A, D, seed=9, masked=True))
    kw = dict(cand=d[3], remaining=d[4], alpha=ALPHA, beta=BETA, use_weight=True, use_penalty=True, mask=d[5])
    u1, l1 = ops.pool_match(d[0], d[1], d[2], B, H, fused=True, **kw)
    u2, l2 = ops.pool_match(d[0], d[1], d[2], B, H, fused=False, **kw)
    assert rel_err(u1.cpu().numpy(), u2.cpu().numpy()) < KTOL and rel_err(l1.cpu().numpy(), l2.cpu().numpy()) < KTOL


def test_bad_arguments_return_an_error_code_without_a_launch():
    lib = _lib.load()
    B, N, H, A, D = 4, 2, 5, 8, 8
    hidden, x = torch.zeros(B * H, A, device='cuda'), torch.zeros(B * H, D + 4, device='cuda')
    w2, cand, rem = torch.zeros(A, device='cuda'), torch.zeros(B, N, D, device='cuda'), torch.zeros(B, N, device='cuda')
    user, logits = torch.full((B, D), 7.0, device='cuda'), torch.full((B, N), 7.0, device='cuda')
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def call(hidden_p=P(hidden), x_p=P(x), cand_p=P(cand), rem_p=P(rem), user_p=P(user), logits_p=P(logits), H=H, D=D, ldx=D + 4, N=N):
        return lib.lime_pool_match_f32(hidden_p, A, P(w2), x_p, ldx, None, cand_p, rem_p, 0.1, 0.5, 1, 1, user_p, logits_p, B, N, H, A, D, None)

    assert call() == 0
    torch.cuda.synchronize()
    user.fill_(7.0), logits.fill_(7.0)
    assert call(D=6) == -1                                     # D % 4 != 0
    assert call(H=0) == -1
    assert call(N=0) == -1
    assert call(user_p=None, logits_p=None) == -1 and b'NULL' in lib.lime_last_error_string()
    assert call(hidden_p=None) == -1
    assert call(x_p=P(x, 4)) == -1                             # misaligned pointers
    assert call(cand_p=P(cand, 4)) == -1
    assert call(user_p=P(user, 4)) == -1
    assert call(ldx=D + 1) == -1
    assert call(rem_p=None) == -1                              # use_weight without remaining
    assert call(cand_p=None) == -1
    assert call(H=513) == -2                                   # outside what the kernel is built for
    torch.cuda.synchronize()
    assert torch.all(user == 7.0) and torch.all(logits == 7.0)   # nothing ran
