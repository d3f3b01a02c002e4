"""lime_topk_rows_f32 (csrc/topk_rows_f32.hip) on the MI355X: positions and scores, bit for bit, against a numpy stable sort under the
order the header states -- descending score; equal scores (+0.0 == -0.0) lower position first; a NaN behind every number, NaNs in
position order; slots behind the C-th hold -1 / -inf -- on rows built to hit the edges.  The kernel takes a row in chunks of 4096
columns: C sits on either side of one chunk, of two, and of the 31 chunk lists its merge takes per round."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 4096
NEG_INF_BITS = np.float32(-np.inf).view(np.int32)


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from lime_cikm25_amd import ops as _ops
    from lime_cikm25_amd import _lib
    _lib.load()
    return _ops


def expected(scores, k):
    """numpy statement of the order: stable sorts, last key first -- position (implicit), then the score descending with the zeros
    folded, then NaN-ness."""
    U, C = scores.shape
    pos = np.full((U, k), -1, dtype=np.int32)
    top = np.full((U, k), -np.inf, dtype=np.float32)
    for u in range(U):
        row = scores[u]
        nan = np.isnan(row)
        value = np.where(nan, 0.0, row).astype(np.float64) + 0.0           # -0.0 + 0.0 = +0.0: the zeros tie
        order = np.argsort(-value, kind='stable')                          # descending, ties in position order
        order = order[np.argsort(nan[order], kind='stable')]               # NaNs behind every number, in position order
        n = min(k, C)
        pos[u, :n] = order[:n]
        top[u, :n] = row[order[:n]]
    return pos, top


def check(ops, scores, k, what=''):
    if isinstance(scores, np.ndarray):
        scores = torch.from_numpy(scores).cuda()
    pos, top = ops.topk_rows(scores, k)
    torch.cuda.synchronize()
    want_pos, want_top = expected(scores.cpu().numpy(), k)
    assert pos.dtype == torch.int32 and top.dtype == torch.float32 and pos.shape == top.shape == (scores.shape[0], k)
    assert np.array_equal(pos.cpu().numpy(), want_pos), what
    assert np.array_equal(top.cpu().numpy().view(np.int32), want_top.view(np.int32)), what      # bitwise: the sign of a zero, a NaN's payload
    return pos, top


def edge_rows(C, seed):
    """Seven rows of C scores: all equal; +-0.0 mixed with a few values; blocks of -inf; one NaN among numbers; NaNs and -inf and numbers;
    few distinct values (many ties); plain random."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((7, C), dtype=np.float32)
    rows[0] = 1.5
    rows[1] = rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], dtype=np.float32), size=C)
    rows[2] = rng.standard_normal(C).astype(np.float32)
    rows[2, : C // 3] = -np.inf
    rows[2, C // 2: C // 2 + max(1, C // 5)] = -np.inf
    rows[3] = rng.standard_normal(C).astype(np.float32)
    rows[3, C // 2] = np.nan
    rows[4] = rng.choice(np.array([np.nan, -np.inf, np.inf, 0.0, -0.0, 2.0], dtype=np.float32), size=C)
    rows[5] = rng.integers(-2, 3, size=C).astype(np.float32)
    rows[6] = rng.standard_normal(C).astype(np.float32)
    return rows


@pytest.mark.parametrize('C', [1, 2, 127, 128, 129, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1, 31 * CHUNK + 5, 32 * CHUNK + 1])
def test_edge_rows_at_every_chunk_boundary(ops, C):
    rows = edge_rows(C, seed=C)
    for k in sorted({1, 10, 128}):
        check(ops, rows, k, 'C %d k %d' % (C, k))


@pytest.mark.parametrize('C', [1, 5, 100])
def test_k_equal_to_and_beyond_the_row(ops, C):
    rows = edge_rows(C, seed=7 + C)
    check(ops, rows, C if C <= 128 else 128)                               # k = C
    pos, top = check(ops, rows, min(128, C + 9))                           # k > C: trailing -1 / -inf
    if C + 9 <= 128:
        assert (pos[:, C:] == -1).all() and np.array_equal(top[:, C:].cpu().numpy().view(np.int32), np.full((7, 9), NEG_INF_BITS))


def test_a_row_that_holds_only_nans_and_infinities(ops):
    rows = np.full((2, 300), np.nan, dtype=np.float32)
    rows[1] = -np.inf
    rows[1, 17] = np.nan
    pos, _ = check(ops, rows, 20)
    assert pos[0].tolist() == list(range(20)) and pos[1].tolist() == [i for i in range(21) if i != 17]


def test_large_rows_and_the_leading_dimension(ops):
    """C = 2^20 + 3 (257 chunks: nine merge rounds), and a row-strided view: the columns behind C belong to someone else."""
    C = (1 << 20) + 3
    big = torch.from_numpy(edge_rows(C + 50, seed=3)[[1, 4, 6]]).cuda()
    big[:, C:] = float('inf')                                              # must never be seen
    view = big[:, :C]
    assert view.stride(0) == C + 50
    pos, top = check(ops, view, 128)
    again = ops.topk_rows(view, 128)
    assert torch.equal(again[0], pos) and torch.equal(again[1].view(torch.int32), top.view(torch.int32))
    small = torch.from_numpy(edge_rows(77, seed=4)).cuda()
    check(ops, small[:, 3:40], 10)                                         # an offset, strided view of one chunk


def test_exact_workspace_filled_with_nans(ops):
    """Exactly lime_topk_rows_workspace() floats, NaN-filled, inside a guarded allocation: enough, nothing written outside, and the
    contents on entry do not matter."""
    from lime_cikm25_amd import _lib
    lib = _lib.load()
    U, C, k = 3, 3 * CHUNK + 11, 64
    scores = torch.from_numpy(edge_rows(C, seed=9)[:U]).cuda()
    need = int(lib.lime_topk_rows_workspace(U, C))
    assert need == U * 4 * 128 * 2
    want_pos, want_top = expected(scores.cpu().numpy(), k)
    GUARD = 1 << 12
    results = []
    for fill in (float('nan'), 0.0, -1.0):
        raw = torch.full((need + 2 * GUARD,), 12345.0, dtype=torch.float32, device='cuda')
        raw[GUARD:GUARD + need] = fill
        pos = torch.empty((U, k), dtype=torch.int32, device='cuda')
        top = torch.empty((U, k), dtype=torch.float32, device='cuda')
        st = lib.lime_topk_rows_f32(scores.data_ptr(), C, U, C, k, pos.data_ptr(), top.data_ptr(), raw.data_ptr() + 4 * GUARD, need,
                                    torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert st == 0
        assert bool((raw[:GUARD] == 12345.0).all()) and bool((raw[GUARD + need:] == 12345.0).all()), 'written outside the workspace'
        assert np.array_equal(pos.cpu().numpy(), want_pos) and np.array_equal(top.cpu().numpy().view(np.int32), want_top.view(np.int32))
        results.append((pos, top))
    # one float less is refused
    st = lib.lime_topk_rows_f32(scores.data_ptr(), C, U, C, k, pos.data_ptr(), top.data_ptr(), raw.data_ptr() + 4 * GUARD, need - 1, None)
    assert st == -1


def test_wrapper_refuses_bad_arguments(ops):
    s = torch.zeros(2, 8, device='cuda')
    with pytest.raises(ValueError):
        ops.topk_rows(s, 0)
    with pytest.raises(TypeError):
        ops.topk_rows(torch.zeros(2, 8), 1)
    with pytest.raises(ValueError):
        ops.topk_rows(s[:, ::2], 1)
    from lime_cikm25_amd import _lib
    with pytest.raises(_lib.LimeHipError, match='128'):
        ops.topk_rows(s, 129)
