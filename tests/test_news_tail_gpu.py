"""The launches of the news-side tail over the distinct news (DESIGN.md "Distinct news behind the encoders"): the xin assembly, the
counted intent_fuse and the grouped mid-M GEMM with one device-side row count per problem.  Everything bitwise: a counted launch
must give the rows below its count exactly what the uncounted launch gives them, and leave the rest alone."""
import pytest
import torch

from lime_cikm25_amd import ops

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


def _randn(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).cuda()


def _count(c):
    return torch.tensor([c], dtype=torch.int32, device='cuda')


@pytest.mark.parametrize('nblk_t,nblk_b', [(1, 4), (4, 1)])
def test_news_xin_equals_mean_pool_and_gather(nblk_t, nblk_b):
    M, E, ldx = 70, 300, 352
    cap = M + 1
    g = torch.Generator().manual_seed(3)
    tb, bb = _randn(cap * nblk_t, E, seed=1), _randn(cap * nblk_b, E, seed=2)
    title_row = torch.randint(0, cap, (cap,), generator=g, dtype=torch.int32).cuda()
    body_row = torch.randint(0, cap, (cap,), generator=g, dtype=torch.int32).cuda()
    # the mean pool of the compacted path (the counted form: mean_pool_flat_kernel, rows added in order), then the expansion
    want_t = ops.gather_rows(title_row, ops.mean_pool(tb, cap, nblk_t, n_seq_dev=_count(cap)), torch.empty((cap, E), device='cuda'))
    want_b = ops.gather_rows(body_row, ops.mean_pool(bb, cap, nblk_b, n_seq_dev=_count(cap)), torch.empty((cap, E), device='cuda'))
    for c in (0, 1, 40, cap):
        nw = ops.NewsCompacted()
        nw.n, nw.title_row, nw.body_row = M, title_row, body_row
        nw.counts = torch.tensor([c, 3 * c, max(c - 1, 0), 0], dtype=torch.int32, device='cuda')
        xin = torch.full((2 * cap, ldx), SENTINEL, device='cuda')
        ops.news_xin(tb, nblk_t, bb, nblk_b, nw, xin, E)
        torch.cuda.synchronize()
        assert torch.equal(xin[:c, :E], want_t[:c]) and torch.equal(xin[cap:cap + c, :E], want_b[:c]), c
        assert bool((xin[c:cap] == SENTINEL).all()) and bool((xin[cap + c:] == SENTINEL).all()), c        # rows at or beyond the count
        assert bool((xin[:, E:] == SENTINEL).all()), c                                                    # the topic columns are not its
    assert float(want_t.abs().max()) > 0


def test_intent_fuse_with_a_device_count():
    M, k, D, A = 37, 3, 400, 200
    intents, hidden = _randn(2 * M * k, D, seed=4), torch.tanh(_randn(2 * M * k, A, seed=5))
    a2t, a2b = _randn(A, seed=6), _randn(A, seed=7)
    want = ops.intent_fuse(intents, hidden, a2t, a2b, torch.full((M, 900), SENTINEL, device='cuda'), M, k, D, A)
    assert bool((want[:, 2 * D:] == SENTINEL).all()) and bool(torch.isfinite(want).all())
    for c in (0, 1, M):
        got = ops.intent_fuse(intents, hidden, a2t, a2b, torch.full((M, 900), SENTINEL, device='cuda'), M, k, D, A, m_dev=_count(c))
        torch.cuda.synchronize()
        assert torch.equal(got[:c], want[:c]), c
        assert bool((got[c:] == SENTINEL).all()), c


def test_grouped_gemm_with_one_device_count_per_problem():
    M, N, K = 200, 400, 352
    a = [_randn(M, K, seed=10 + i) for i in range(2)]
    w = [_randn(N, K, seed=20 + i) * 0.05 for i in range(2)]
    bias = [_randn(N, seed=30 + i) for i in range(2)]
    full = ops.linear_group([dict(a=a[i], w=w[i], bias=bias[i], act='tanh') for i in range(2)])
    counts = [0, 1, 63, 64, 65, M]
    for c0, c1 in zip(counts, reversed(counts)):
        outs = [torch.full((M, N), SENTINEL, device='cuda') for _ in range(2)]
        ops.linear_group([dict(a=a[i], w=w[i], bias=bias[i], act='tanh', out=outs[i], m_dev=_count(c)) for i, c in enumerate((c0, c1))])
        torch.cuda.synchronize()
        for i, c in enumerate((c0, c1)):
            assert torch.equal(outs[i][:c], full[i][:c]), (c0, c1, i)
            assert bool((outs[i][c:] == SENTINEL).all()), (c0, c1, i)
    assert ops._lib.load().lime_last_linear_kernel() == b'gemm_mid_group_kernel'
