"""The bidirectional LSTM step kernel (csrc/lstm_f32.hip, ops.lstm / ops.lstm_bwd) alone on the MI355X, against torch.nn.LSTM in fp64
on the CPU through pack_padded_sequence / pad_packed_sequence with the same weights: hout (exact zeros behind every length), h_n and
c_n of both directions, the device row count, a row's bits wherever it sits, the backward against fp64 autograd, repeatability."""
import functools

import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from helpers import rel_err
from lime_cikm25_amd import ops

pytestmark = pytest.mark.gpu
TOL = 1e-3                      # the project's tolerance (test_naml_gpu.py)
E = 20                          # input width: a multiple of 4, the smallest the GEMM kernels take without a fallback


def _weights(h, seed):
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / h ** 0.5
    u = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) * k).float()
    return {'weight_ih_l0': u(4 * h, E), 'weight_hh_l0': u(4 * h, h), 'bias_ih_l0': u(4 * h), 'bias_hh_l0': u(4 * h),
            'weight_ih_l0_reverse': u(4 * h, E), 'weight_hh_l0_reverse': u(4 * h, h), 'bias_ih_l0_reverse': u(4 * h),
            'bias_hh_l0_reverse': u(4 * h)}


def _lengths(kind, R, T, seed):
    if kind == 'ones':
        return torch.ones(R, dtype=torch.int64)
    if kind == 'full':
        return torch.full((R,), T, dtype=torch.int64)
    g = torch.Generator().manual_seed(seed)
    l = torch.randint(1, T + 1, (R,), generator=g)
    l[0] = 1                                                     # mixed always holds a length-1 and a full sequence (when R allows)
    l[-1] = T
    if R > 2:
        l[R // 2] = 1
    return l


@functools.lru_cache(maxsize=None)
def problem(h, R, T, kind):
    """Inputs and the fp64 reference with its gradients, computed once per shape and shared by the tests (never modified)."""
    seed = 1000 * h + 10 * R + T
    w = _weights(h, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = (torch.rand(R, T, E, generator=g) * 2 - 1).float()
    lens = _lengths(kind, R, T, seed + 2)
    gw_h = (torch.rand(R, T, 2 * h, generator=g) * 2 - 1).double()      # the loss weights every hout entry and c_n
    gw_c = (torch.rand(2, R, h, generator=g) * 2 - 1).double()
    ref = torch.nn.LSTM(E, h, batch_first=True, bidirectional=True).double()
    ref.load_state_dict({k: v.double() for k, v in w.items()})
    xd = x.double().requires_grad_(True)
    out, (h_n, c_n) = ref(pack_padded_sequence(xd, lens, batch_first=True, enforce_sorted=False))
    hout, _ = pad_packed_sequence(out, batch_first=True, total_length=T)
    loss = (hout * gw_h).sum() + (c_n * gw_c).sum()
    loss.backward()
    grads = {k: p.grad.detach() for k, p in ref.named_parameters()}
    return dict(w=w, x=x, lens=lens, gw_h=gw_h, gw_c=gw_c, hout=hout.detach(), h_n=h_n.detach(), c_n=c_n.detach(), dx=xd.grad.detach(),
                grads=grads)


def _device_weights(w):
    wih = torch.cat([w['weight_ih_l0'], w['weight_ih_l0_reverse']]).cuda().contiguous()
    bias = torch.cat([w['bias_ih_l0'] + w['bias_hh_l0'], w['bias_ih_l0_reverse'] + w['bias_hh_l0_reverse']]).cuda().contiguous()
    whh = torch.stack([w['weight_hh_l0'], w['weight_hh_l0_reverse']]).cuda().contiguous()
    return wih, bias, whh


def run_forward(p, R, T, save=False, **kw):
    wih, bias, whh = _device_weights(p['w'])
    x = p['x'].reshape(R * T, E).cuda().contiguous()
    gi = ops.linear(x, wih, bias=bias)
    lens = p['lens'].to(torch.int32).cuda()
    return ops.lstm(gi, whh, lens, T, save=save, **kw), (x, wih, whh, lens)


SHAPES = [(16, 1, 1, 'ones'), (16, 7, 8, 'mixed'), (16, 130, 33, 'mixed'), (16, 130, 8, 'full'), (48, 1, 8, 'full'), (48, 7, 33, 'mixed'),
          (48, 130, 1, 'ones'), (48, 130, 8, 'ones'), (400, 1, 33, 'mixed'), (400, 7, 1, 'ones'), (400, 7, 8, 'full'), (400, 130, 8, 'mixed'),
          (400, 130, 33, 'mixed')]


@pytest.mark.parametrize('h,R,T,kind', SHAPES)
def test_forward_against_fp64(h, R, T, kind):
    p = problem(h, R, T, kind)
    (hout, c), _ = run_forward(p, R, T)
    torch.cuda.synchronize()
    hout = hout.view(R, T, 2 * h).cpu()
    lens = p['lens']
    idx = torch.arange(R)
    h_n = torch.stack([hout[idx, lens - 1, :h], hout[:, 0, h:]])
    errs = (rel_err(hout, p['hout']), rel_err(h_n, p['h_n']), rel_err(c.cpu(), p['c_n']))
    print('h=%d R=%d T=%d %s: hout %.2e h_n %.2e c_n %.2e' % ((h, R, T, kind) + errs))
    behind = torch.arange(T)[None, :] >= lens[:, None]
    assert torch.equal(hout[behind], torch.zeros_like(hout[behind])), 'hout rows behind a length must stay exactly zero'
    assert max(errs) < TOL


@pytest.mark.parametrize('h,R,T,n', [(16, 130, 8, 65), (48, 7, 8, 3), (400, 130, 8, 64), (16, 7, 8, 0)])
def test_device_row_count_bounds_the_rows(h, R, T, n):
    p = problem(h, R, T, 'mixed')
    POISON = 12345.0
    hout = torch.zeros(R * T, 2 * h, device='cuda')
    hout.view(R, T, 2 * h)[n:] = POISON
    c = torch.full((2, R, h), POISON, device='cuda')
    (hout, c), _ = run_forward(p, R, T, hout=hout, c=c, n_rows_dev=torch.tensor([n], dtype=torch.int32, device='cuda'))
    hout = hout.view(R, T, 2 * h).cpu()
    c = c.cpu()
    assert bool((hout[n:] == POISON).all()) and bool((c[:, n:] == POISON).all())
    if n:
        e = (rel_err(hout[:n], p['hout'][:n]), rel_err(c[:, :n], p['c_n'][:, :n]))
        print('n_rows_dev %d of %d: hout %.2e c_n %.2e' % (n, R, e[0], e[1]))
        assert max(e) < TOL


@pytest.mark.parametrize('h', [16, 48, 400])
def test_a_rows_bits_do_not_depend_on_where_it_sits(h):
    R, T = 130, 8
    p = problem(h, R, T, 'mixed')
    (hout, c), _ = run_forward(p, R, T)
    hout = hout.view(R, T, 2 * h)
    for row, pos in ((3, 0), (3, 100), (129, 17), (65, 64)):
        # the row alone ...
        q = dict(p, x=p['x'][row:row + 1], lens=p['lens'][row:row + 1])
        (h1, c1), _ = run_forward(q, 1, T)
        assert torch.equal(h1.view(T, 2 * h), hout[row]) and torch.equal(c1[:, 0], c[:, row])
        # ... and at another position of another batch, under a device row count
        R2 = 117
        x2 = p['x'][:R2].clone()
        l2 = p['lens'][:R2].clone()
        x2[pos], l2[pos] = p['x'][row], p['lens'][row]
        (h2, c2), _ = run_forward(dict(p, x=x2, lens=l2), R2, T, n_rows_dev=torch.tensor([pos + 1], dtype=torch.int32, device='cuda'))
        assert torch.equal(h2.view(R2, T, 2 * h)[pos], hout[row]) and torch.equal(c2[:, pos], c[:, row])


def run_backward(p, R, T, h):
    (hout, c, saved), (x, wih, whh, lens) = run_forward(p, R, T, save=True)
    dhout = p['gw_h'].reshape(R * T, 2 * h).float().cuda().contiguous()
    dgi = ops.lstm_bwd(dhout, p['gw_c'].float().cuda(), whh, lens, T, saved)
    dwih, dbias = ops.linear_wgrad(dgi, x, want_bias=True)
    dx = ops.linear(dgi, wih.t().contiguous())
    h_prev = saved[2]
    dwhh = [ops.linear_wgrad(dgi[:, d * 4 * h:(d + 1) * 4 * h], h_prev[:, d * h:(d + 1) * h]) for d in (0, 1)]
    return dict(hout=hout, c=c, dgi=dgi, dwih=dwih, dbias=dbias, dx=dx, dwhh=dwhh)


@pytest.mark.parametrize('h,R,T,kind', [(16, 7, 8, 'mixed'), (48, 130, 8, 'mixed'), (48, 7, 33, 'mixed'), (400, 7, 8, 'full'), (400, 130, 8, 'mixed'),
                                        (16, 1, 1, 'ones'), (48, 130, 8, 'ones')])
def test_backward_against_fp64_autograd(h, R, T, kind):
    p = problem(h, R, T, kind)
    assert int(p['lens'].min()) == 1 or kind == 'full'
    got = run_backward(p, R, T, h)
    torch.cuda.synchronize()
    g = p['grads']
    want = {'weight_ih_l0': got['dwih'][:4 * h], 'weight_ih_l0_reverse': got['dwih'][4 * h:], 'weight_hh_l0': got['dwhh'][0],
            'weight_hh_l0_reverse': got['dwhh'][1], 'bias_ih_l0': got['dbias'][:4 * h], 'bias_hh_l0': got['dbias'][:4 * h],
            'bias_ih_l0_reverse': got['dbias'][4 * h:], 'bias_hh_l0_reverse': got['dbias'][4 * h:]}
    errs = {k: rel_err(v.cpu(), g[k]) for k, v in want.items()}
    errs['x'] = rel_err(got['dx'].view(R, T, E).cpu(), p['dx'])
    print('h=%d R=%d T=%d %s: %s' % (h, R, T, kind, ' '.join('%s %.2e' % kv for kv in errs.items())))
    pad = torch.arange(T)[None, :] >= p['lens'][:, None]
    dgi = got['dgi'].view(R, T, 8 * h).cpu()
    assert torch.equal(dgi[pad], torch.zeros_like(dgi[pad])), 'padding tokens have no gradient'
    assert max(errs.values()) < TOL


def test_forward_and_backward_repeat_bitwise():
    h, R, T = 48, 130, 8
    p = problem(h, R, T, 'mixed')
    a, b = run_backward(p, R, T, h), run_backward(p, R, T, h)
    for k in ('hout', 'c', 'dgi', 'dwih', 'dbias', 'dx'):
        assert torch.equal(a[k], b[k]), k
    assert all(torch.equal(x, y) for x, y in zip(a['dwhh'], b['dwhh']))


def test_arguments_are_checked_before_any_launch():
    whh = torch.zeros(2, 4 * 24, 24, device='cuda')
    with pytest.raises(ValueError, match='multiple of 16'):
        ops.lstm(torch.zeros(8, 8 * 24, device='cuda'), whh, torch.ones(1, dtype=torch.int32, device='cuda'), 8)
    with pytest.raises(ValueError):
        ops.lstm(torch.zeros(8, 100, device='cuda'), torch.zeros(2, 64, 16, device='cuda'), torch.ones(1, dtype=torch.int32, device='cuda'), 8)


def test_mask_lengths():
    g = torch.Generator().manual_seed(5)
    m = torch.rand(37, 19, generator=g) < 0.5
    m[3] = False
    got = ops.mask_lengths(m.cuda(), min_len=1).cpu()
    assert torch.equal(got, m.sum(1).clamp(min=1).to(torch.int32))

