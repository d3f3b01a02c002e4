"""ops.topk_segments (lime_topk_segments_f32, csrc/topk_segments_f32.hip) on the MI355X against a numpy statement of the order: a
stable sort on (is NaN, score descending with -0.0 == +0.0, position).  Positions must match exactly and scores bit for bit.  Scores
come from a small set of values, so ties are everywhere; segments are empty, shorter and longer than k, one chunk of 4096 exactly,
one more, and several chunks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LENS = [0, 1, 127, 128, 129, 4096, 4097, 9000]
VALUES = np.array([-np.inf, -2.5, -1e-30, -0.0, 0.0, 1e-30, 1.0, np.float32(1.0000001), 3.5, np.inf, np.nan], dtype=np.float32)


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from lime_cikm25_amd import ops as _ops
    return _ops


def statement(scores, offsets, k):
    """(positions int32 [U, k], scores fp32 [U, k]) by the documented order."""
    U = len(offsets) - 1
    pos, top = np.full((U, k), -1, dtype=np.int32), np.full((U, k), -np.inf, dtype=np.float32)
    for u in range(U):
        s = scores[offsets[u]:offsets[u + 1]]
        nan = np.isnan(s)
        value = np.where(nan, 0.0, s).astype(np.float64) + 0.0                        # (-0.0 + 0.0 = +0.0: the zeros tie)
        order = np.lexsort((np.arange(s.size), -value, nan))[:k]                      # NaN last, then descending, then position
        pos[u, :order.size], top[u, :order.size] = order, s[order]
    return pos, top


def draw(lens, seed):
    rng = np.random.default_rng(seed)
    p = np.ones(VALUES.size)
    p[-1] = 0.05                                                                      # a few NaNs
    scores = VALUES[rng.choice(VALUES.size, size=int(np.sum(lens)), p=p / p.sum())]
    return scores, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def same(got, want):
    (gp, gt), (wp, wt) = got, want
    assert gp.dtype == torch.int32 and gt.dtype == torch.float32
    assert np.array_equal(gp.cpu().numpy(), wp)
    assert np.array_equal(gt.cpu().numpy().view(np.int32), wt.view(np.int32))         # the input's bits: signed zeros, NaNs


SCORES, OFFSETS = draw(LENS, 7)
WANT = {k: statement(SCORES, OFFSETS, k) for k in (1, 10, 128)}


@pytest.mark.parametrize('k', [1, 10, 128])
def test_ragged_segments_follow_the_documented_order(ops, k):
    assert np.isnan(SCORES).sum() > 10 and (SCORES == 0).sum() > 100 and np.signbit(SCORES[SCORES == 0]).any()
    s, o = torch.from_numpy(SCORES).cuda(), torch.from_numpy(OFFSETS).cuda()
    same(ops.topk_segments(s, o, k), WANT[k])
    same(ops.topk_segments(s, o, k), WANT[k])                                         # and again: the same bits
    pos, top = WANT[k]
    assert (pos[0] == -1).all() and np.isneginf(top[0]).all()                          # the empty segment: a row of -1 / -inf
    assert pos[1, 0] == 0 and (pos[1, 1:] == -1).all()


def test_segments_in_another_order_give_the_same_rows(ops):
    """The split into chunks depends on where a segment starts in the grid, the result does not."""
    perm = [7, 0, 5, 3, 6, 1, 4, 2]
    scores = np.concatenate([SCORES[OFFSETS[u]:OFFSETS[u + 1]] for u in perm])
    offsets = np.concatenate([[0], np.cumsum([LENS[u] for u in perm])]).astype(np.int64)
    pos, top = ops.topk_segments(torch.from_numpy(scores).cuda(), torch.from_numpy(offsets).cuda(), 10)
    same((pos, top), (WANT[10][0][perm], WANT[10][1][perm]))


@pytest.mark.parametrize('U,C', [(7, 300), (3, 5000)])
def test_a_rectangle_equals_topk_rows(ops, U, C):
    scores, offsets = draw([C] * U, 11)
    s = torch.from_numpy(scores).cuda()
    pos, top = ops.topk_segments(s, torch.from_numpy(offsets).cuda(), 16)
    rp, rt = ops.topk_rows(s.view(U, C), 16)
    assert torch.equal(pos, rp) and torch.equal(top.view(torch.int32), rt.view(torch.int32))


def test_no_scores_at_all(ops):
    pos, top = ops.topk_segments(torch.empty(0, device='cuda'), torch.zeros(4, dtype=torch.int64, device='cuda'), 3)
    assert pos.shape == (3, 3) and (pos == -1).all() and torch.isneginf(top).all()


def test_workspace_contract(ops, monkeypatch):
    """Exactly lime_topk_segments_workspace floats, zero-filled and poisoned: the same bits; one float fewer: refused before any launch
    (test_workspace_contract_gpu.py's harness: guard bands, three poisons, untouched outputs after the refusal)."""
    from lime_cikm25_amd import _lib
    from test_workspace_contract_gpu import contract
    lib = _lib.load()
    s, o = torch.from_numpy(SCORES).cuda(), torch.from_numpy(OFFSETS).cuda()
    need = int(lib.lime_topk_segments_workspace(len(LENS), SCORES.size))
    assert need == 2 * (len(LENS) + 1) + 2 * (SCORES.size // 4096) * 128 * 2
    contract(monkeypatch, ops, [need], lambda h: ops.topk_segments(s, o, 10), lambda pos, top: same((pos, top), WANT[10]))
    ws = torch.zeros(need, device='cuda')
    pos, top = torch.zeros(len(LENS), 10, dtype=torch.int32, device='cuda'), torch.zeros(len(LENS), 10, device='cuda')
    st = lib.lime_topk_segments_f32(ops._p(s), ops._p(o), len(LENS), SCORES.size, 10, ops._p(pos), ops._p(top), ops._p(ws), need - 1, ops._stream())
    torch.cuda.synchronize()
    assert st != 0 and not pos.any() and not top.any()


@pytest.mark.parametrize('k', [0, 129])
def test_k_out_of_range_is_refused(ops, k):
    from lime_cikm25_amd import _lib
    s, o = torch.from_numpy(SCORES).cuda(), torch.from_numpy(OFFSETS).cuda()
    with pytest.raises(ValueError, match='1 <= k <= 128'):
        ops.topk_segments(s, o, k)
    lib = _lib.load()
    need = int(lib.lime_topk_segments_workspace(len(LENS), SCORES.size))
    ws = torch.zeros(need, device='cuda')
    out = torch.zeros(len(LENS) * 129, dtype=torch.int32, device='cuda')
    assert lib.lime_topk_segments_f32(ops._p(s), ops._p(o), len(LENS), SCORES.size, k, ops._p(out), ops._p(out), ops._p(ws), need, ops._stream()) == -2
