"""lime_slate_metrics_f32 (csrc/slate_metrics.hip) on the MI355X against recommend.slate_metrics, the fp64 host statement: statuses,
counts and the columns that are sums of fp64 table entries or counts are EQUAL; the intra-list distance is held to the forward error
bound of two fp32 inverse norms and one fp32 dot product of length E, (2 E + 8) 2^-24; the sums are bitwise independent of the
reduction grid, of a slate's place in the batch and of the leading dimension of the positions."""
import ctypes
import math

import numpy as np
import pytest
import torch

from lime_cikm25_amd import _lib, ops
from slate_cases import host_metrics, slate_case

pytestmark = pytest.mark.gpu

U24, U53 = 2.0 ** -24, 2.0 ** -53
EXACT = (0, 1, 2, 3, 5, 6, 7)                     # value is accumulated in fp64 in slot order: exact as well


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).cuda()


def upload(case):
    return dict(positions=dev(case['positions']), offsets=dev(case['offsets']), news=dev(case['news']), labels=dev(case['labels']),
                skip=dev(case['skip']), value=dev(case['value']), table=dev(case['table']), keys=dev(case['keys']))


def run(case, t=None, k=None, **kw):
    t = upload(case) if t is None else t
    res = ops.slate_metrics(t['positions'], case['k'] if k is None else k, t['offsets'], t['news'], t['labels'], t['skip'], t['value'],
                            t['table'], t['keys'], n=case['n'], n_keys=case['n_keys'], **kw)
    torch.cuda.synchronize()
    return res


def check(case, res, want=None, what=''):
    """The kernel's result against the host statement, by the bounds in this file's docstring; prints the largest deviations."""
    per_w, status_w, sums_w, counts_w = host_metrics(case) if want is None else want
    per, status = res.per_slate.cpu().numpy(), res.status.cpu().numpy()
    sums, counts = res.sums.cpu().numpy(), res.counts.cpu().numpy()
    R, E = case['R'], case['E']
    assert per.shape == (R, 8) and status.shape == (R,)
    assert np.array_equal(status, status_w) and np.array_equal(counts, counts_w)
    for c in EXACT:
        assert np.array_equal(per[:, c], per_w[:, c]), 'column %d differs by %.3e' % (c, np.abs(per[:, c] - per_w[:, c]).max())
    ild = float(np.abs(per[:, 4] - per_w[:, 4]).max()) if R else 0.0
    print('%s R %d k %d E %d: ILD max |kernel - fp64| %.3e (bound %.3e)' % (what, R, case['k'], E, ild, (2 * E + 8) * U24))
    assert ild <= (2 * E + 8) * U24
    # the sums: the kernel's own per_slate over the counted sets.  R 2^-53 max|column| is below the spacing of fp64 at the sum where the
    # terms are alike, so the yardstick must not round on the way: math.fsum, the exact sum rounded once.
    skipped = np.zeros(R, dtype=bool) if case['skip'] is None else case['skip'].astype(bool)
    sets = (status == 0, ~skipped & (per[:, 6] >= 2), ~skipped & (per[:, 6] >= 1))
    for c in range(8):
        col = per[sets[0 if c < 4 else 1 if c == 4 else 2], c]
        bound = R * U53 * (np.abs(col).max() if col.size else 0.0)
        off = abs(sums[c] - math.fsum(col.tolist()))
        assert off <= bound, 'sum of column %d: off by %.3e (bound %.3e)' % (c, off, bound)
    return ild


SHAPES = {
    'one_slot': dict(R=1, k=1, E=4, n=5, n_keys=1, lens=[1]),
    'three': dict(R=3, k=2, ldp=5, E=4, n=9, n_keys=3, lens=[1, 2, 9]),
    'ten': dict(R=257, k=10, E=64, n=50, n_keys=7, lens=[1, 4, 299, 0]),
    'ten_wide': dict(R=257, k=10, ldp=13, E=400, n=300, n_keys=270, lens=[1, 4, 299]),
    'sixteen': dict(R=257, k=16, ldp=19, E=64, n=50, n_keys=7, max_len=40, lens=[1, 15, 16, 17, 299]),      # the widest slate of a wave
    'seventeen': dict(R=257, k=17, E=64, n=50, n_keys=7, max_len=40, lens=[1, 16, 17, 18, 299]),            # the first of a workgroup
    'full': dict(R=3, k=128, E=64, n=400, n_keys=270, max_len=299, lens=[299, 150, 128]),
    'full_wide': dict(R=40, k=128, ldp=131, E=400, n=400, n_keys=7, max_len=299, lens=[299, 1, 127]),
    'past_the_grid': dict(R=70000, k=2, E=4, n=40, n_keys=7, max_len=6),
    'pool': dict(R=257, k=10, ldp=13, E=64, n=50, n_keys=7, pool=True, max_len=299),
    'pool_small': dict(R=3, k=2, E=4, n=9, n_keys=1, pool=True, max_len=1),
}


@pytest.mark.parametrize('name', list(SHAPES))
def test_kernel_equals_the_host_statement(name):
    case = slate_case(11, **SHAPES[name])
    want = host_metrics(case)
    check(case, run(case), want, name)
    if name in ('ten', 'ten_wide', 'pool'):                            # conditions on the generator: every branch is in the case
        assert sorted(set(want[1].tolist())) == ([1] if case['offsets'] is None else [0, 1, 2, 3])
        assert (want[0][:, 6] == 0).any() and (want[0][:, 6] == case['k']).any()
    if name in ('full', 'full_wide'):
        assert want[0][:, 6].max() >= 120                              # (a few ids outside the table are planted)


@pytest.mark.parametrize('absent', ['labels', 'skip', 'value', 'table', 'keys', 'all'])
def test_every_optional_input_may_be_absent(absent):
    off = ['labels', 'skip', 'value', 'table', 'keys'] if absent == 'all' else [absent]
    case = slate_case(12, R=257, k=10, ldp=13, E=64, n=50, n_keys=7, lens=[1, 4, 299], **{name: False for name in off})
    res = run(case)
    check(case, res, what='without ' + absent)
    per = res.per_slate.cpu().numpy()
    for name, cols in (('labels', (0, 1, 2, 3)), ('value', (7,)), ('table', (4,)), ('keys', (5,))):
        if name in off:
            assert (per[:, cols] == 0).all()
    if 'labels' in off:
        assert (res.status == 1).all() and int(res.counts[0]) == 0


def test_a_table_that_is_a_column_view_or_unaligned():
    case = slate_case(13, R=64, k=10, E=64, n=50, n_keys=7)
    t = upload(case)
    want = host_metrics(case)
    wide = torch.zeros((case['n'], 96), dtype=torch.float32, device='cuda')
    wide[:, 16:80] = t['table']
    a = run(case, dict(t, table=wide[:, 16:80]))                       # 16-byte aligned rows, leading dimension 96
    b = run(case, dict(t, table=wide[:, 15:79].copy_(t['table'])))    # rows that start 4 bytes off: the scalar-load instantiation
    check(case, a, want, 'column view')
    check(case, b, want, 'unaligned')
    assert torch.equal(a.per_slate, run(case, t).per_slate)
    assert torch.equal(a.per_slate, b.per_slate)                      # the same sums in the same order whatever the load width


def test_sums_do_not_depend_on_the_reduction_grid_or_the_run():
    case = slate_case(14, R=3001, k=5, E=8, n=50, n_keys=7, max_len=12)
    t = upload(case)
    a = run(case, t)
    for blocks in (0, 1, 7):
        b = run(case, t, reduce_blocks=blocks)
        assert torch.equal(a.sums, b.sums) and torch.equal(a.counts, b.counts)                # bitwise: fp64 compared for equality
        assert torch.equal(a.per_slate, b.per_slate) and torch.equal(a.status, b.status)
    check(case, a, what='reduction grid')


def test_a_slate_does_not_feel_its_place_in_the_batch():
    case = slate_case(15, R=300, k=10, E=64, n=50, n_keys=7)
    t = upload(case)
    whole = run(case, t)
    r0, r1 = 100, 200
    middle = dict(t, positions=t['positions'][r0:r1], offsets=t['offsets'][r0:r1 + 1], skip=t['skip'][r0:r1])
    assert middle['positions'].data_ptr() != t['positions'].data_ptr()
    a = run(case, middle)                                              # rows 100 .. 199 where they lie
    b = run(case, {k: (v.clone() if k in ('positions', 'offsets', 'skip') else v) for k, v in middle.items()})     # ... as rows 0 .. 99
    assert torch.equal(a.per_slate, whole.per_slate[r0:r1]) and torch.equal(a.status, whole.status[r0:r1])
    assert torch.equal(a.per_slate, b.per_slate) and torch.equal(a.sums, b.sums) and torch.equal(a.counts, b.counts)
    assert int(a.counts[2]) > 50


def test_a_prefix_of_a_wider_slate_is_the_slate_at_the_smaller_k():
    case = slate_case(16, R=257, k=10, E=64, n=50, n_keys=7)
    t = upload(case)
    a = run(case, t, k=5)                                              # the first 5 of ldp = 10, in place
    b = run(case, dict(t, positions=t['positions'][:, :5].contiguous()), k=5)
    c = run(case, dict(t, positions=t['positions'][:, :5]), k=5)       # the same as a [R, 5] view with row stride 10
    for other in (b, c):
        assert torch.equal(a.per_slate, other.per_slate) and torch.equal(a.status, other.status)
        assert torch.equal(a.sums, other.sums) and torch.equal(a.counts, other.counts)
    check(dict(case, k=5), a, what='prefix')
    assert not torch.equal(a.per_slate[:, 0], run(case, t).per_slate[:, 0])


def test_no_slates_is_a_success_with_zero_sums():
    case = slate_case(17, R=0, k=3, E=4, n=5, n_keys=2)
    res = run(case)
    assert res.per_slate.shape == (0, 8) and (res.sums == 0).all() and (res.counts == 0).all()
    # the C entry itself: no launch, the sums and counts cleared
    lib = _lib.load()
    buf = torch.full((16,), 7.0, dtype=torch.float64, device='cuda')
    cnt = torch.full((3,), 7, dtype=torch.int64, device='cuda')
    a = good_args(buf, cnt)
    a.R = 0
    assert lib.lime_slate_metrics_f32(ctypes.byref(a), None) == 0
    torch.cuda.synchronize()
    assert (buf[:8] == 0).all() and (buf[8:] == 7).all() and (cnt == 0).all()


_KEEP = []


def good_args(sums=None, counts=None):
    """An args struct the entry accepts (one slate of two slots over a pool of two rows), every pointer a live device buffer."""
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device='cuda')
    t = dict(positions=i32(0, 1), news=i32(0, 1), disc=torch.ones(128, dtype=torch.float64, device='cuda'),
             per_slate=torch.zeros(8, dtype=torch.float64, device='cuda'), status=i32(0),
             sums=torch.zeros(8, dtype=torch.float64, device='cuda') if sums is None else sums,
             counts=torch.zeros(3, dtype=torch.int64, device='cuda') if counts is None else counts,
             table=torch.ones((2, 8), dtype=torch.float32, device='cuda'), labels=torch.zeros(2, dtype=torch.uint8, device='cuda'),
             offsets=torch.tensor([0, 2], dtype=torch.int64, device='cuda'))
    _KEEP.append(t)
    a = _lib.SlateMetricsArgs()
    for name in ('positions', 'news', 'disc', 'per_slate', 'status', 'sums', 'counts'):
        setattr(a, name, t[name].data_ptr())
    a.R, a.P, a.ldp, a.ld, a.n, a.k, a.E = 1, 2, 2, 0, 2, 2, 0
    a._t = t
    return a


def test_the_entry_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    call = lambda a: lib.lime_slate_metrics_f32(ctypes.byref(a), None)
    BAD, UNSUPPORTED = _lib.CONSTANTS['LIME_ERR_BAD_ARG'], _lib.CONSTANTS['LIME_ERR_UNSUPPORTED']
    assert call(good_args()) == 0
    assert lib.lime_slate_metrics_f32(None, None) == BAD
    for name in ('positions', 'news', 'disc', 'per_slate', 'status', 'sums', 'counts'):
        a = good_args()
        setattr(a, name, None)
        assert call(a) == BAD and b'NULL' in lib.lime_last_error_string(), name
    a = good_args()
    a.labels = a._t['labels'].data_ptr()                               # labels without offsets
    assert call(a) == BAD and b'offsets' in lib.lime_last_error_string()
    a.offsets = a._t['offsets'].data_ptr()
    assert call(a) == 0
    for field, value in (('R', -1), ('k', 0), ('k', 3), ('n', 0), ('reserved', 1), ('reduce_blocks', -1)):
        a = good_args()
        setattr(a, field, value)
        assert call(a) == BAD, (field, value)
    a = good_args()
    a.table, a.E, a.ld = a._t['table'].data_ptr(), 8, 4                # ld < E
    assert call(a) == BAD
    a.ld = 8
    assert call(a) == 0
    a.E, a.ld = 6, 8                                                   # rows are read in quads
    assert call(a) == UNSUPPORTED
    a = good_args()
    a.k, a.ldp = 129, 129
    assert call(a) == UNSUPPORTED and b'128' in lib.lime_last_error_string()
    torch.cuda.synchronize()
