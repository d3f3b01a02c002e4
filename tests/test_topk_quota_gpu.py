"""ops.topk_rows_quota / ops.topk_segments_quota (lime_topk_rows_quota_f32 / lime_topk_segments_quota_f32, csrc/topk_quota_f32.hip) on
the MI355X: positions and score bits equal to ``recommend.quota_topk`` -- the host statement of the quota walk, itself held against a
literal sequential walk in test_topk_quota_cpu.py.  The kernel takes a row in chunks of 4096 columns, walks each chunk's sorted keys and
merges 31 chunk lists per round: C sits on either side of one chunk, in the middle of three, and one past 31 chunks (two rounds)."""
import numpy as np
import pytest
import torch

from lime_cikm25_amd import recommend
from quota_cases import CHUNK, crowded, drop_mask, edge_rows, group_keys, same

pytestmark = pytest.mark.gpu

U = 3
NEG_INF_BITS = np.float32(-np.inf).view(np.int32)
_WANT = {}


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from lime_cikm25_amd import ops as _ops
    from lime_cikm25_amd import _lib
    _lib.load()
    return _ops


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rows_case(C):
    """(scores [U, C], keys [C] over 6 groups) and their device copies, once per C."""
    if C not in _WANT:
        scores, keys = edge_rows(U, C, seed=C), group_keys(C, 6, seed=C + 1)
        _WANT[C] = (scores, keys, dev(scores), dev(keys))
    return _WANT[C]


@pytest.mark.parametrize('C', [1, 37, CHUNK, CHUNK + 1, 9000, CHUNK * 31 + 1])
def test_rows_equal_the_host_walk_at_every_chunk_boundary(ops, C):
    scores, keys, s, g = rows_case(C)
    for k in (1, 10, 128):
        for quota in sorted({1, 2, k}):
            same(ops.topk_rows_quota(s, g, quota, k, n_keys=6), recommend.quota_topk(scores, keys, k, quota), 'C %d k %d quota %d' % (C, k, quota))


def test_crowded_chunks_filter_before_they_cut(ops):
    """C = 8192: one group owns the 300 best scores of each chunk; k = 10, quota = 2: eight results come from the other groups."""
    scores, keys = crowded()
    want = recommend.quota_topk(scores, keys, 10, 2)
    assert (keys[want[0][0]] == 0).sum() == 2 and (want[0] >= 0).all()
    pos, top = ops.topk_rows_quota(dev(scores), dev(keys), 2, 10, n_keys=7)
    same((pos, top), want)
    assert (keys[pos.cpu().numpy()[0]] != 0).sum() == 8


@pytest.mark.parametrize('C', [37, 9000])
def test_a_quota_that_binds_nowhere_is_the_plain_topk(ops, C):
    scores, keys, s, g = rows_case(C)
    for k in (1, 10, 128):
        want = tuple(x.cpu().numpy() for x in ops.topk_rows(s, k))
        same(ops.topk_rows_quota(s, g, k, k, n_keys=6), want)
        same(ops.topk_rows_quota(s, g, 1 << 30, k, n_keys=6), want)
    lens = [0, 1, 7, 130, 5000]
    off = dev(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    flat, fkeys = dev(edge_rows(1, sum(lens), seed=3)[0]), dev(group_keys(sum(lens), 6, seed=4))
    for k in (10, 128):
        same(ops.topk_segments_quota(flat, off, fkeys, k, k, n_keys=6), tuple(x.cpu().numpy() for x in ops.topk_segments(flat, off, k)))


@pytest.mark.parametrize('C', [5, 300, CHUNK + 9])
def test_one_group_gives_quota_entries_then_nothing(ops, C):
    scores = edge_rows(U, C, seed=C)
    keys = np.zeros(C, dtype=np.int32)
    for quota in (1, 3, 20):
        pos, top = ops.topk_rows_quota(dev(scores), dev(keys), quota, 10, n_keys=1)
        same((pos, top), recommend.quota_topk(scores, keys, 10, quota))
        n = min(quota, C, 10)
        pos, top = pos.cpu().numpy(), top.cpu().numpy()
        assert (pos[:, :n] >= 0).all() and (pos[:, n:] == -1).all() and (top[:, n:].view(np.int32) == NEG_INF_BITS).all()


@pytest.mark.parametrize('C', [37, 9000])
def test_drop_mask_and_the_schedule_view(ops, C):
    scores, keys = edge_rows(6, C, seed=C + 2), group_keys(C, 6, seed=C)
    s, g = dev(scores), dev(keys)
    for R in (6, 3, 1):                                                     # drop_rows = U; the [S U, C] view over a [U, C] mask; one row
        drop = drop_mask(R, C, seed=R)
        want = recommend.quota_topk(scores, keys, 10, 2, drop)
        same(ops.topk_rows_quota(s, g, 2, 10, drop=dev(drop), n_keys=6), want, 'bool mask, %d rows' % R)
        same(ops.topk_rows_quota(s, g, 2, 10, drop=dev(drop.astype(np.uint8) * 7), n_keys=6), want, 'uint8 mask, %d rows' % R)
        got = ops.topk_rows_quota(s, g, 2, 10, drop=dev(drop), n_keys=6)[0].cpu().numpy()
        for u in range(6):
            assert not drop[u % R][got[u][got[u] >= 0]].any()
    everything = np.ones((1, C), dtype=bool)
    pos, top = ops.topk_rows_quota(s, g, 2, 10, drop=dev(everything), n_keys=6)
    assert (pos == -1).all() and torch.isneginf(top).all()


@pytest.mark.parametrize('C', [37, 9000])
def test_keys_out_of_range_are_dropped_not_read_past(ops, C):
    scores, keys = edge_rows(U, C, seed=C + 5), group_keys(C, 6, seed=C).astype(np.int64)
    keys[::7], keys[3::7], keys[5::7] = -1, 6, 2 ** 31 - 1                  # below, the first beyond n_keys = 6, far beyond
    keys[0] = -2 ** 31
    host = np.where((keys >= 0) & (keys < 6), keys, -1)
    same(ops.topk_rows_quota(dev(scores), dev(keys.astype(np.int32)), 2, 10, n_keys=6), recommend.quota_topk(scores, host, 10, 2))
    off = np.array([0, C // 2, C], dtype=np.int64)
    same(ops.topk_segments_quota(dev(scores[0]), dev(off), dev(keys.astype(np.int32)), 2, 10, n_keys=6),
         recommend.quota_topk_segments(scores[0], off, host, 10, 2))


def test_segments_of_every_kind_in_one_call(ops):
    lens = [0, 1, 7, 130, 5000, 0, 2 * CHUNK + 1, 3]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    P = int(off[-1])
    scores, keys, drop = edge_rows(1, P, seed=11)[0], group_keys(P, 6, seed=12), drop_mask(1, P, seed=13)[0]
    s, o, g = dev(scores), dev(off), dev(keys)
    for k in (1, 10, 128):
        for quota in sorted({1, 2, k}):
            same(ops.topk_segments_quota(s, o, g, quota, k, n_keys=6), recommend.quota_topk_segments(scores, off, keys, k, quota),
                 'k %d quota %d' % (k, quota))
    same(ops.topk_segments_quota(s, o, g, 2, 10, drop=dev(drop), n_keys=6), recommend.quota_topk_segments(scores, off, keys, 10, 2, drop))
    pos, top = ops.topk_segments_quota(torch.empty(0, device='cuda'), torch.zeros(4, dtype=torch.int64, device='cuda'),
                                       torch.empty(0, dtype=torch.int32, device='cuda'), 2, 3)
    assert pos.shape == (3, 3) and (pos == -1).all() and torch.isneginf(top).all()


def test_row_strided_view(ops):
    """ld > C: the columns behind C belong to someone else and must never be seen."""
    for C in (40, CHUNK + 5):
        big = dev(edge_rows(U, C + 50, seed=C))
        big[:, C:] = float('inf')
        view = big[:, :C]
        assert view.stride(0) == C + 50
        keys = group_keys(C, 6, seed=C)
        same(ops.topk_rows_quota(view, dev(keys), 2, 10, n_keys=6), recommend.quota_topk(view.cpu().numpy(), keys, 10, 2))


def test_two_runs_are_bit_equal(ops):
    scores, keys, s, g = rows_case(CHUNK * 31 + 1)
    a, b = ops.topk_rows_quota(s, g, 2, 128, n_keys=6), ops.topk_rows_quota(s, g, 2, 128, n_keys=6)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_bad_arguments_are_refused_without_a_launch(ops):
    from lime_cikm25_amd import _lib
    s, g = torch.zeros(2, 8, device='cuda'), torch.zeros(8, dtype=torch.int32, device='cuda')
    for bad in (dict(k=0), dict(quota=0), dict(keys=g[:7]), dict(drop=torch.zeros(2, 7, dtype=torch.bool, device='cuda')),
                dict(drop=torch.zeros(8, dtype=torch.bool, device='cuda'))):
        with pytest.raises(ValueError):
            ops.topk_rows_quota(**{**dict(scores=s, keys=g, quota=1, k=1), **bad})
    with pytest.raises(TypeError):
        ops.topk_rows_quota(s, g.long(), 1, 1)
    with pytest.raises(TypeError):
        ops.topk_rows_quota(torch.zeros(2, 8), g, 1, 1)
    with pytest.raises(_lib.LimeHipError, match='128'):
        ops.topk_rows_quota(s, g, 1, 129)
    with pytest.raises(_lib.LimeHipError, match='8192'):
        ops.topk_rows_quota(s, g, 1, 1, n_keys=8193)
    o = torch.tensor([0, 3, 8], device='cuda')
    with pytest.raises(ValueError):
        ops.topk_segments_quota(s.view(-1)[:8], o, g, 0, 1)
    with pytest.raises(ValueError):
        ops.topk_segments_quota(s.view(-1)[:8], o, g, 1, 129)
    with pytest.raises(_lib.LimeHipError, match='8192'):
        ops.topk_segments_quota(s.view(-1)[:8], o, g, 1, 1, n_keys=8193)
    lib = _lib.load()
    pos, top = torch.full((2, 1), 77, dtype=torch.int32, device='cuda'), torch.full((2, 1), 77.0, device='cuda')
    st = lib.lime_topk_rows_quota_f32(s.data_ptr(), 8, 2, 8, g.data_ptr(), 8, 0, None, 0, 1, pos.data_ptr(), top.data_ptr(), None, 0, None)
    torch.cuda.synchronize()
    assert st == -1 and (pos == 77).all() and (top == 77.0).all()          # refused: the outputs were not touched


def test_exact_workspaces_filled_with_nans(ops):
    """Exactly the promised floats, NaN-filled (and two other fills), inside a guarded allocation: enough, nothing written outside, the
    contents on entry do not matter; one float fewer is refused."""
    from lime_cikm25_amd import _lib
    lib = _lib.load()
    C, k, quota, GUARD = 3 * CHUNK + 11, 64, 3, 1 << 12
    scores, keys = edge_rows(U, C, seed=9), group_keys(C, 6, seed=10)
    s, g = dev(scores), dev(keys)
    stream = torch.cuda.current_stream().cuda_stream
    need = int(lib.lime_topk_rows_quota_workspace(U, C))
    assert need == U * 4 * 128 * 2
    want = recommend.quota_topk(scores, keys, k, quota)
    lens = [0, 5000, 1, 2 * CHUNK + 1, 130]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    P = int(off[-1])
    o = dev(off)
    need_seg = int(lib.lime_topk_segments_quota_workspace(len(lens), P))
    assert need_seg == 12 + 2 * (P // CHUNK) * 128 * 2
    want_seg = recommend.quota_topk_segments(scores.reshape(-1)[:P], off, np.tile(keys, U)[:P], k, quota)
    flat, fkeys = s.view(-1)[:P].contiguous(), dev(np.tile(keys, U)[:P])
    pos = torch.empty((len(lens), k), dtype=torch.int32, device='cuda')
    top = torch.empty((len(lens), k), dtype=torch.float32, device='cuda')
    for fill in (float('nan'), 0.0, -1.0):
        for floats, call, n_rows, expect in (
                (need, lambda w: lib.lime_topk_rows_quota_f32(s.data_ptr(), C, U, C, g.data_ptr(), 6, quota, None, 0, k, pos.data_ptr(),
                                                              top.data_ptr(), w, need, stream), U, want),
                (need_seg, lambda w: lib.lime_topk_segments_quota_f32(flat.data_ptr(), o.data_ptr(), len(lens), P, fkeys.data_ptr(), 6, quota, None,
                                                                      k, pos.data_ptr(), top.data_ptr(), w, need_seg, stream), len(lens), want_seg)):
            raw = torch.full((floats + 2 * GUARD,), 12345.0, dtype=torch.float32, device='cuda')
            raw[GUARD:GUARD + floats] = fill
            st = call(raw.data_ptr() + 4 * GUARD)
            torch.cuda.synchronize()
            assert st == 0
            assert bool((raw[:GUARD] == 12345.0).all()) and bool((raw[GUARD + floats:] == 12345.0).all()), 'written outside the workspace'
            same((pos[:n_rows], top[:n_rows]), expect, 'fill %r' % fill)
    w = raw.data_ptr() + 4 * GUARD
    assert lib.lime_topk_rows_quota_f32(s.data_ptr(), C, U, C, g.data_ptr(), 6, quota, None, 0, k, pos.data_ptr(), top.data_ptr(), w, need - 1,
                                        None) == -1
    assert lib.lime_topk_segments_quota_f32(flat.data_ptr(), o.data_ptr(), len(lens), P, fkeys.data_ptr(), 6, quota, None, k, pos.data_ptr(),
                                            top.data_ptr(), w, need_seg - 1, None) == -1
