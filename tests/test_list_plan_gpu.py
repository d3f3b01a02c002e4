"""ops.list_plan (lime_list_plan_count + lime_list_plan, csrc/list_plan.hip) on the MI355X against recommend.list_plan, the host
statement: all four outputs exactly, on lists shorter and longer than the placement chunk of 256 pairs and tables of 5, 300 and 8192
bins; then the refusals, the run-to-run bits and what a key outside the table does."""
import numpy as np
import pytest
import torch

from lime_cikm25_amd import recommend

pytestmark = pytest.mark.gpu

LENS = [0, 1, 37, 300, 1000]
GUARD, SENTINEL = 64, -0x5A5A5A5B


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from lime_cikm25_amd import ops as _ops
    return _ops


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def same_plan(got, want):
    assert got.order.dtype == torch.int64 and got.group_offsets.dtype == torch.int64 and got.slot_key.dtype == torch.int32
    assert np.array_equal(got.n_distinct, want.n_distinct) and got.n_distinct.dtype == np.int32
    for name in ('order', 'group_offsets', 'slot_key'):
        assert np.array_equal(getattr(got, name).cpu().numpy(), getattr(want, name)), name


def on_device(keys, offsets):
    return torch.from_numpy(np.asarray(keys, dtype=np.int32)).cuda(), torch.from_numpy(np.asarray(offsets, dtype=np.int64)).cuda()


@pytest.mark.parametrize('T_all', [5, 300, 8192])
def test_lists_of_five_lengths_equal_the_host_plan(ops, T_all):
    keys = np.random.default_rng(T_all).integers(0, T_all, size=sum(LENS))
    offsets = offsets_of(LENS)
    want = recommend.list_plan(keys, offsets)
    got = ops.list_plan(*on_device(keys, offsets), n_keys=T_all)
    same_plan(got, want)
    assert want.n_distinct.max() == min(T_all, len(set(keys[-1000:].tolist()))) and want.n_distinct[0] == 0
    again = ops.list_plan(*on_device(keys, offsets), n_keys=T_all)                    # two runs: identical bits
    same_plan(again, want)
    if T_all == 300:                                                                  # a table larger than the keys need changes nothing
        same_plan(ops.list_plan(*on_device(keys, offsets)), want)


def test_one_list_holding_every_key_once(ops):
    keys = np.random.default_rng(1).permutation(8192)
    want = recommend.list_plan(keys, [0, 8192])
    assert want.n_distinct.tolist() == [8192] and np.array_equal(want.slot_key, np.arange(8192))
    same_plan(ops.list_plan(*on_device(keys, [0, 8192]), n_keys=8192), want)


def test_one_key_a_thousand_times(ops):
    keys = np.full(1000, 7)                                                           # four placement chunks, one cursor
    want = recommend.list_plan(keys, [0, 1000])
    assert np.array_equal(want.order, np.arange(1000)) and want.group_offsets.tolist() == [0, 1000]
    same_plan(ops.list_plan(*on_device(keys, [0, 1000]), n_keys=8), want)


def test_more_slots_than_any_list_needs(ops):
    keys = np.random.default_rng(2).integers(0, 5, size=sum(LENS))
    offsets = offsets_of(LENS)
    want = recommend.list_plan(keys, offsets, slots=9)
    assert want.slot_key.shape == (5 * 9,)
    same_plan(ops.list_plan(*on_device(keys, offsets), slots=9, n_keys=5), want)
    # the counts a caller already holds are taken as they are: no second count, the same plan
    same_plan(ops.list_plan(*on_device(keys, offsets), slots=9, n_keys=5, n_distinct=want.n_distinct), want)
    with pytest.raises(ValueError, match='5 distinct keys'):
        ops.list_plan(*on_device(keys, offsets), slots=4, n_keys=5)


def test_no_user_and_no_pair(ops):
    same_plan(ops.list_plan(*on_device([], [0]), n_keys=4), recommend.list_plan([], [0]))
    same_plan(ops.list_plan(*on_device([], [0, 0, 0]), n_keys=4), recommend.list_plan([], [0, 0, 0]))


def test_a_table_of_8193_bins_is_refused(ops):
    from lime_cikm25_amd._lib import LimeHipError
    with pytest.raises(LimeHipError, match='8192'):
        ops.list_plan(*on_device([0, 1], [0, 2]), n_keys=8193)


def guarded(n, dtype):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + n]


@pytest.mark.parametrize('bad', [300, -1, 2 ** 31 - 1])
@pytest.mark.parametrize('user', ['last', 'middle'])
def test_a_key_outside_the_table_stays_inside_the_buffers(ops, bad, user):
    """One pair with a key outside [0, T_all), every output between guard elements.  The guards are untouched, order is still a
    permutation that keeps every user's range, every pair with a key in range is in its right group and the bad pair takes no slot.
    In the LAST user's list it lies behind group_offsets[U S]: in no group.  (In another user's list it lies behind that user's last
    key, in the rows of the user's last slot: a CSR whose groups join up has no other place for it.)"""
    from lime_cikm25_amd import _lib
    lib = _lib.load()
    T_all, lens = 300, [5, 300, 0, 41]
    offsets = offsets_of(lens)
    U, P = len(lens), int(offsets[-1])
    keys = np.random.default_rng(3).integers(0, T_all, size=P).astype(np.int64)
    at = P - 20 if user == 'last' else 100
    keys[at] = bad
    k_dev, o_dev = on_device(keys.astype(np.int32), offsets)
    nd_buf, nd = guarded(U, torch.int32)
    _lib.check(lib.lime_list_plan_count(ops._p(k_dev), ops._p(o_dev), U, P, T_all, ops._p(nd), ops._stream()), 'lime_list_plan_count')
    valid = np.ones(P, dtype=bool)
    valid[at] = False
    want_nd = [len(set(keys[offsets[u]:offsets[u + 1]][valid[offsets[u]:offsets[u + 1]]].tolist())) for u in range(U)]
    assert nd.cpu().tolist() == want_nd                                               # the bad key is no key
    S = max(want_nd)
    order_buf, order = guarded(P, torch.int64)
    goff_buf, goff = guarded(U * S + 1, torch.int64)
    skey_buf, skey = guarded(U * S, torch.int32)
    _lib.check(lib.lime_list_plan(ops._p(k_dev), ops._p(o_dev), U, P, T_all, S, ops._p(order), ops._p(goff), ops._p(skey), ops._stream()),
               'lime_list_plan')
    torch.cuda.synchronize()
    for buf, n in ((nd_buf, U), (order_buf, P), (goff_buf, U * S + 1), (skey_buf, U * S)):
        assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + n:] == SENTINEL).all(), 'a guard element was written'
    order, goff, skey = order.cpu().numpy(), goff.cpu().numpy(), skey.cpu().numpy()
    for u in range(U):
        assert sorted(order[offsets[u]:offsets[u + 1]].tolist()) == list(range(offsets[u], offsets[u + 1]))
    assert (skey >= 0).all() and (skey < T_all).all() and (np.diff(goff) >= 0).all() and goff[0] == 0
    grouped = np.zeros(P, dtype=bool)
    for u in range(U):
        distinct = sorted(set(keys[offsets[u]:offsets[u + 1]][valid[offsets[u]:offsets[u + 1]]].tolist()))
        for s, key in enumerate(distinct):
            members = order[goff[u * S + s]:goff[u * S + s + 1]]
            members = members[valid[members]]
            assert skey[u * S + s] == key and (keys[members] == key).all() and members.tolist() == sorted(members.tolist())
            assert len(members) == ((keys[offsets[u]:offsets[u + 1]] == key) & valid[offsets[u]:offsets[u + 1]]).sum()
            grouped[members] = True
    assert np.array_equal(grouped, valid)                                             # every pair in range is in its right group
    if user == 'last':
        assert goff[-1] == P - 1 and order[P - 1] == at                               # ... and the bad pair is in none
    else:
        assert goff[-1] == P and order[offsets[2] - 1] == at                          # behind user 1's last key, inside user 1's range
