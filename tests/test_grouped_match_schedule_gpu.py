"""lime_grouped_match_schedule_f32 (csrc/grouped_match_schedule_f32.hip) on the MI355X against a float64 host statement of its formula
written here: per (slot s, pair p of group i)
    s[h] = (kp[i H + h] . qa[index[p]] + kp[i H + h] . qt[occ[s, p]]) * scale,   a = softmax_h(s),
    logits[s, p] = (sum_h a[h] (g[i H + h] . ca[index[p]] + g[i H + h] . ct[occ[s, p]])) * w(remaining[s, p])

The error bound.  Both errors are helpers.rel_err against that statement: the schedule kernel's must not exceed TWICE the error of
lime_grouped_match_occurrence_f32 run slot by slot on the same inputs -- the factorised form rounds two partial sums where the
composed form rounds one -- plus one fp32 ulp of the largest |logit|.  The ulp is an absolute amount and rel_err a relative one: an
element's absolute error is divided by max(|want|, floor) with floor the mean magnitude of the non-zero reference entries, so one ulp
of the largest |logit| is worth at most ulp / floor on rel_err's scale, and that is the margin added.  The yardstick itself has to be
well inside KTOL (half of it) for the seeds used.  Both figures are printed per case.

Without occurrence tables (n_occ = 0, a baseline model) the result is lime_grouped_match_indexed_f32's per slot, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu

KTOL = 2e-5
ALPHA, BETA = 0.3, 0.7
N_TABLE = 37
GROUPS = [0, 1, 63, 64, 65, 130, 0]      # pairs per group in one plan: empty, one, a tile less one, a tile, one past it, three tiles, empty
P = sum(GROUPS)
HS = [1, 3, 50]
SHAPES = [(4, 4), (8, 12), (16, 20), (36, 52)]        # below, at and above the 16-column chunk
N_OCCS = [0, 1, 4, 100]
SLOTS = [1, 2, 5]
FLAGS = [(False, False), (True, False), (True, True), (False, True)]       # (use_weight, use_penalty)


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from lime_cikm25_amd import ops as _ops
    from lime_cikm25_amd import _lib
    _lib.load()
    return _ops


def make(H, A, D, n_occ, S, sizes=GROUPS, n=N_TABLE, seed=0):
    rng = np.random.default_rng(seed)
    G, pairs = len(sizes), int(sum(sizes))
    u = lambda *s: rng.uniform(-1.0, 1.0, size=s).astype(np.float32)
    remaining = rng.uniform(-3.0, 3.0, size=(S, pairs)).astype(np.float32)           # positive, negative ...
    if pairs > 4:
        remaining[:, 1], remaining[:, 2] = 0.0, -0.0                                 # ... and both zeros
    index = rng.integers(0, n, size=pairs).astype(np.int32)
    index[-1] = n - 1
    occ = rng.integers(0, max(n_occ, 1), size=(S, pairs)).astype(np.int32)
    occ[:, -1] = max(n_occ, 1) - 1
    return dict(kp=u(G * H, A), g=u(G * H, D), qa=u(n, A), ca=u(n, D), qt=u(max(n_occ, 1), A), ct=u(max(n_occ, 1), D), index=index, occ=occ,
                remaining=remaining, offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), H=H, n_occ=n_occ)


def on_device(d):
    return {k: torch.from_numpy(v).cuda() for k, v in d.items() if isinstance(v, np.ndarray)}


def scale_of(A):
    return 1.0 / float(np.sqrt(np.float32(A)))


def weight64(r, use_penalty):
    r = r.astype(np.float64)
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    if use_penalty:
        w = sig(np.float64(np.float32(ALPHA)) * r)
        return np.where(r >= 0, w, np.float64(np.float32(BETA)) * w)
    return sig(np.float64(np.float32(ALPHA)) * np.abs(r))


def statement(d, use_weight, use_penalty):
    """The formula above in float64 -> [S, P]."""
    H, n_occ = d['H'], d['n_occ']
    f = lambda k: d[k].astype(np.float64)
    kp, g, qa, ca, qt, ct = (f(k) for k in ('kp', 'g', 'qa', 'ca', 'qt', 'ct'))
    scale = np.float64(np.float32(scale_of(kp.shape[1])))
    S, pairs = d['occ'].shape
    out = np.zeros((S, pairs))
    off = d['offsets']
    for i in range(len(off) - 1):
        rows = np.arange(off[i], off[i + 1])
        if rows.size == 0:
            continue
        kpi, gi = kp[i * H:(i + 1) * H], g[i * H:(i + 1) * H]
        sa, ma = qa[d['index'][rows]] @ kpi.T, ca[d['index'][rows]] @ gi.T                      # [pairs, H]
        for s in range(S):
            sc, m = sa, ma
            if n_occ:
                sc, m = sa + qt[d['occ'][s, rows]] @ kpi.T, ma + ct[d['occ'][s, rows]] @ gi.T
            sc = sc * scale
            e = np.exp(sc - sc.max(axis=1, keepdims=True))
            out[s, rows] = (e * m).sum(axis=1) / e.sum(axis=1)
    return out * weight64(d['remaining'], use_penalty) if use_weight else out


def run_schedule(ops, t, d, use_weight=True, use_penalty=True, **kw):
    tables = dict(occ=t['occ'], qt=t['qt'], ct=t['ct']) if d['n_occ'] else {}
    tables.update(kw)
    return ops.grouped_match_schedule(t['kp'], t['g'], t['qa'], t['ca'], t['remaining'], t['offsets'], t['index'], d['H'],
                                      scale_of(t['kp'].shape[1]), ALPHA, BETA, use_weight, use_penalty, slots=t['remaining'].shape[0], **tables)


def run_twin(ops, t, d, use_weight=True, use_penalty=True):
    """The yardstick: lime_grouped_match_occurrence_f32 (lime_grouped_match_indexed_f32 without tables) slot by slot -> [S, P]."""
    S = t['remaining'].shape[0]
    out = []
    for s in range(S):
        tables = dict(occ=t['occ'][s].contiguous(), qt=t['qt'], ct=t['ct']) if d['n_occ'] else {}
        out.append(ops.grouped_match(t['kp'], t['g'], t['qa'], t['ca'], t['remaining'][s].contiguous(), t['offsets'], d['H'],
                                     scale_of(t['kp'].shape[1]), ALPHA, BETA, use_weight, use_penalty, index=t['index'], **tables))
    return torch.stack(out)


@pytest.mark.parametrize('n_occ', N_OCCS)
@pytest.mark.parametrize('A,D', SHAPES)
@pytest.mark.parametrize('H', HS)
def test_error_against_float64_and_the_baseline_form(ops, H, A, D, n_occ):
    worst = (0.0, 0.0)
    for S in SLOTS:
        d = make(H, A, D, n_occ, S, seed=1000 * H + 10 * A + n_occ + S)
        t = on_device(d)
        for use_weight, use_penalty in FLAGS:
            got = run_schedule(ops, t, d, use_weight, use_penalty)
            twin = run_twin(ops, t, d, use_weight, use_penalty)
            assert got.shape == (S, P) and got.dtype == torch.float32 and torch.isfinite(got).all()
            if n_occ == 0:
                assert torch.equal(got, twin), 'the baseline form must have the indexed kernel\'s bits'
            want = statement(d, use_weight, use_penalty)
            e, ey = rel_err(got.cpu().numpy(), want), rel_err(twin.cpu().numpy(), want)
            floor = float(np.abs(want[want != 0]).mean())
            ulp = float(np.spacing(np.float32(np.abs(want).max()))) / floor
            print('H %d A %d D %d n_occ %d S %d weight %d penalty %d: schedule %.3e, yardstick %.3e, bound %.3e'
                  % (H, A, D, n_occ, S, use_weight, use_penalty, e, ey, 2 * ey + ulp))
            worst = max(worst, (e, ey))
            assert ey <= KTOL / 2, 'the yardstick is not well inside KTOL for this seed'
            assert e <= 2 * ey + ulp
    print('H %d A %d D %d n_occ %d: worst schedule %.3e (yardstick there %.3e)' % ((H, A, D, n_occ) + worst))


def as_bits(x):
    return x.cpu().numpy().view(np.int32)


@pytest.mark.parametrize('H,A,D,n_occ', [(50, 36, 52, 100), (3, 16, 20, 4), (50, 8, 12, 0)])
def test_bits_do_not_depend_on_the_slots(ops, H, A, D, n_occ):
    """Permuted slots give permuted results, fewer slots the same results, a slot given twice the same bits twice."""
    d = make(H, A, D, n_occ, 5, seed=7)
    t = on_device(d)
    first = run_schedule(ops, t, d)
    assert np.array_equal(as_bits(first), as_bits(run_schedule(ops, t, d))), 'two runs differ'
    perm = [3, 0, 4, 4, 1, 2, 0]
    t2 = dict(t, occ=t['occ'][perm].contiguous(), remaining=t['remaining'][perm].contiguous())
    assert np.array_equal(as_bits(run_schedule(ops, t2, d)), as_bits(first)[perm])
    for S in (1, 2):
        t3 = dict(t, occ=t['occ'][:S].contiguous(), remaining=t['remaining'][:S].contiguous())
        assert np.array_equal(as_bits(run_schedule(ops, t3, d)), as_bits(first)[:S])


@pytest.mark.parametrize('H,A,D,n_occ', [(50, 36, 52, 100), (1, 4, 4, 1), (3, 16, 20, 0)])
def test_bits_do_not_depend_on_the_plan(ops, H, A, D, n_occ):
    """The same pairs in another group order, in another order inside their group (another place in the tile), behind a stranger
    group, under another P and G and against larger tables that hold the same rows at other places."""
    S = 2
    d = make(H, A, D, n_occ, S, seed=21)
    first = as_bits(run_schedule(ops, on_device(d), d))
    rng = np.random.default_rng(22)
    n2, n_occ2 = 97, max(n_occ, 1) + 12                                    # (112 occurrences x H 50 are inside the kernel's LDS bound)
    place, place_occ = rng.permutation(n2)[:N_TABLE], rng.permutation(n_occ2)[:max(n_occ, 1)]
    stranger = make(H, A, D, n_occ2 if n_occ else 0, S, sizes=[37], n=n2, seed=23)
    tabs = {k: stranger[k].copy() for k in ('qa', 'ca', 'qt', 'ct')}
    tabs['qa'][place], tabs['ca'][place] = d['qa'], d['ca']
    if n_occ:
        tabs['qt'][place_occ], tabs['ct'][place_occ] = d['qt'], d['ct']
    perm = [5, 3, 1, 6, 4, 0, 2]                                           # new place -> old group
    sizes, rows = [37], []
    for i in perm:
        lo, hi = int(d['offsets'][i]), int(d['offsets'][i + 1])
        rows.append(rng.permutation(np.arange(lo, hi)))
        sizes.append(hi - lo)
    rows = np.concatenate(rows)
    grp = lambda name: np.concatenate([stranger[name]] + [d[name][i * H:(i + 1) * H] for i in perm])
    d2 = dict(tabs, kp=grp('kp'), g=grp('g'), H=H, n_occ=n_occ2 if n_occ else 0,
              index=np.concatenate([stranger['index'], place[d['index'][rows]].astype(np.int32)]),
              occ=np.concatenate([stranger['occ'], place_occ[d['occ'][:, rows]].astype(np.int32)], axis=1),
              remaining=np.concatenate([stranger['remaining'], d['remaining'][:, rows]], axis=1),
              offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    second = as_bits(run_schedule(ops, on_device(d2), d2))
    assert second.shape == (S, P + 37)
    assert np.array_equal(second[:, 37:], first[:, rows])


def test_ids_and_offsets_outside_their_range_are_clamped_and_nothing_else_is_written(ops):
    """index against n, occ against n_occ and the offsets against [0, P] -- on tables that lie inside larger allocations whose rows in
    front of and behind them hold NaN -- and logits inside a guarded allocation: the S P floats are written, the guards are not."""
    from lime_cikm25_amd import _lib
    lib = _lib.load()
    H, A, D, n, n_occ, S = 7, 16, 20, N_TABLE, 100, 3
    d = make(H, A, D, n_occ, S, sizes=[3, 67, 5, 0], seed=31)
    pairs = 75
    top, low = np.iinfo(np.int32).max, np.iinfo(np.int32).min
    bad_i, bad_o = d['index'].copy(), d['occ'].copy()
    bad_i[0], bad_i[1], bad_i[2], bad_i[6], bad_i[74] = n, -1, top, low, n + 1000
    bad_o[0, 0], bad_o[1, 3], bad_o[2, 4], bad_o[0, 7], bad_o[2, 73], bad_o[1, 0] = low, n_occ, -1, top, n_occ + 5, n_occ
    bad_off = np.array([-5, 3, 70, pairs + 100, 50], dtype=np.int64)       # below 0, past P, decreasing at the end: an empty group
    fixed = dict(index=np.clip(bad_i.astype(np.int64), 0, n - 1).astype(np.int32),
                 occ=np.clip(bad_o.astype(np.int64), 0, n_occ - 1).astype(np.int32), offsets=np.array([0, 3, 70, pairs, pairs], dtype=np.int64))
    t = on_device(d)
    pad = 8

    def inside_nan(x):
        big = torch.full((x.shape[0] + 2 * pad, x.shape[1]), float('nan'), device='cuda')
        big[pad:pad + x.shape[0]] = x
        return big[pad:pad + x.shape[0]]
    t.update({k: inside_nan(t[k]) for k in ('qa', 'ca', 'qt', 'ct')})
    dev = lambda a: torch.from_numpy(a).cuda()
    want = run_schedule(ops, dict(t, index=dev(fixed['index']), occ=dev(fixed['occ']), offsets=dev(fixed['offsets'])), d, n=n, n_occ=n_occ)
    assert torch.isfinite(want).all()
    e = rel_err(want.cpu().numpy(), statement(dict(d, **fixed), True, True))
    assert e <= KTOL, e
    # the bad plan, straight through the C entry into a guarded logits buffer
    GUARD = 256
    raw = torch.full((S * pairs + 2 * GUARD,), -12345.0, device='cuda')
    bi, bo, boff = dev(bad_i), dev(bad_o), dev(bad_off)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    st = lib.lime_grouped_match_schedule_f32(p(t['kp']), p(t['g']), p(t['qa']), p(t['ca']), p(t['qt']), p(t['ct']), p(t['remaining']), p(boff),
                                             p(bi), n, p(bo), n_occ, ctypes.c_void_p(raw.data_ptr() + 4 * GUARD), 4, pairs, S, H, A, D,
                                             scale_of(A), ALPHA, BETA, 1, 1, None)
    assert st == 0, lib.lime_last_error_string()
    torch.cuda.synchronize()
    assert (raw[:GUARD] == -12345.0).all() and (raw[GUARD + S * pairs:] == -12345.0).all(), 'a write outside logits'
    assert torch.equal(raw[GUARD:GUARD + S * pairs].view(S, pairs), want)
    # n and n_occ below the tables' rows: the clamp is against them, not against the allocation
    few = run_schedule(ops, t, d, n=10, n_occ=3)
    low_ids = dict(t, index=dev(np.minimum(d['index'], 9)), occ=dev(np.minimum(d['occ'], 2)))
    assert torch.equal(few, run_schedule(ops, low_ids, d, n=n, n_occ=n_occ))


def test_pairs_outside_every_group_are_not_written(ops):
    from lime_cikm25_amd import _lib
    lib = _lib.load()
    H, A, D, S = 3, 8, 12, 2
    d = make(H, A, D, 4, S, sizes=[5, 6], seed=41)
    t = on_device(d)
    off = torch.tensor([2, 5, 9], dtype=torch.int64, device='cuda')        # pairs 0, 1, 9 and 10 are in no group
    out = torch.full((S, 11), 777.0, device='cuda')
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    st = lib.lime_grouped_match_schedule_f32(p(t['kp']), p(t['g']), p(t['qa']), p(t['ca']), p(t['qt']), p(t['ct']), p(t['remaining']), p(off),
                                             p(t['index']), N_TABLE, p(t['occ']), 4, p(out), 2, 11, S, H, A, D, scale_of(A), ALPHA, BETA, 1, 1,
                                             None)
    assert st == 0, lib.lime_last_error_string()
    torch.cuda.synchronize()
    assert (out[:, [0, 1, 9, 10]] == 777.0).all() and (out[:, 2:9] != 777.0).all()


def test_ops_check_the_schedule_s_arguments_on_the_host(ops):
    z = lambda *s: torch.zeros(*s, device='cuda')
    off = torch.tensor([0, 2], dtype=torch.int64, device='cuda')
    idx = torch.zeros(2, dtype=torch.int32, device='cuda')
    occ = torch.zeros(3, 2, dtype=torch.int32, device='cuda')
    args = (z(4, 8), z(4, 8), z(3, 8), z(3, 8), None, off, idx, 4, 1.0)
    assert ops.grouped_match_schedule(*args, occ=occ, qt=z(5, 8), ct=z(5, 8)).shape == (3, 2)
    assert ops.grouped_match_schedule(*args, slots=4).shape == (4, 2)
    with pytest.raises(ValueError, match='slot count'):
        ops.grouped_match_schedule(*args)
    with pytest.raises(ValueError, match='must agree'):
        ops.grouped_match_schedule(*args, occ=occ, qt=z(5, 8), ct=z(5, 8), slots=2)
    with pytest.raises(ValueError, match=r'occ must be \[S, P\]'):
        ops.grouped_match_schedule(*args, occ=occ[:, :1], qt=z(5, 8), ct=z(5, 8), slots=3)
    with pytest.raises(ValueError, match='needs ct'):
        ops.grouped_match_schedule(*args, occ=occ, qt=z(5, 8))
    with pytest.raises(ValueError, match=r'remaining must be \[S, P\]'):
        ops.grouped_match_schedule(z(4, 8), z(4, 8), z(3, 8), z(3, 8), z(3, 1), off, idx, 4, 1.0, use_weight=True, occ=occ, qt=z(5, 8),
                                   ct=z(5, 8), slots=3)
    from lime_cikm25_amd import _lib
    with pytest.raises(_lib.LimeHipError, match='bytes of LDS'):
        ops.grouped_match_schedule(z(128, 8), z(128, 8), z(3, 8), z(3, 8), None, torch.tensor([0, 2], dtype=torch.int64, device='cuda'), idx,
                                   128, 1.0, occ=occ, qt=z(100, 8), ct=z(100, 8))
