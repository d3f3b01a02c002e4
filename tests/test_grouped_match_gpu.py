"""lime_grouped_match_f32 (csrc/grouped_match_f32.hip) on the MI355X against a float64 host statement of its formulas,

    s[h] = kp[i, h] . qp[p] / sqrt(A),  alpha = softmax_h(s),  logit[p] = (sum_h alpha[h] (g[i, h] . cand[p])) * w(remaining[p]),

with lime_interest_match_f32 -- run per group on the same inputs -- as the yardstick of the error: the new kernel re-associates that
kernel's sums, so it may be off by at most twice that kernel's own maximum error plus one ulp of the largest |logit| (the margin
tests/test_split_gemm_gpu.py gives a re-associated sum).  Both errors are printed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GROUPS = [0, 1, 63, 64, 65, 130]          # pairs per group, in one call: empty, one, around the 64-pair tile, three tiles
ALPHA, BETA = 0.7, 0.3


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from lime_cikm25_amd import ops as _ops
    from lime_cikm25_amd import _lib
    _lib.load()
    return _ops


def make(H, A, D, sizes=GROUPS, seed=0, remaining=None):
    rng = np.random.default_rng(seed)
    G, P = len(sizes), int(sum(sizes))
    u = lambda *s: rng.uniform(-1.0, 1.0, size=s).astype(np.float32)
    d = dict(kp=u(G * H, A), g=u(G * H, D), qp=u(P, A), cand=u(P, D), H=H,
             remaining=(rng.uniform(-3.0, 3.0, size=P).astype(np.float32) if remaining is None else np.asarray(remaining, np.float32)),
             offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    return d


def weight64(r, use_weight, use_penalty):
    r = r.astype(np.float64)
    if not use_weight:
        return np.ones_like(r)
    with np.errstate(over='ignore'):
        if use_penalty:
            w = 1.0 / (1.0 + np.exp(-ALPHA * r))
            return np.where(r >= 0, w, BETA * w)
        return 1.0 / (1.0 + np.exp(-ALPHA * np.abs(r)))


def reference(d, use_weight, use_penalty):
    """float64 logits [P]."""
    H, A = d['H'], d['kp'].shape[1]
    out = np.zeros(d['qp'].shape[0])
    for i in range(len(d['offsets']) - 1):
        lo, hi = int(d['offsets'][i]), int(d['offsets'][i + 1])
        if hi == lo:
            continue
        kp, g = d['kp'][i * H:(i + 1) * H].astype(np.float64), d['g'][i * H:(i + 1) * H].astype(np.float64)
        s = d['qp'][lo:hi].astype(np.float64) @ kp.T / np.sqrt(float(A))                  # [n, H]
        a = np.exp(s - s.max(axis=1, keepdims=True))
        a /= a.sum(axis=1, keepdims=True)
        out[lo:hi] = (a * (d['cand'][lo:hi].astype(np.float64) @ g.T)).sum(axis=1)
    return out * weight64(d['remaining'], use_weight, use_penalty)


def run_new(ops, d, use_weight, use_penalty):
    t = {k: torch.from_numpy(v).cuda() for k, v in d.items() if k != 'H'}
    A = d['kp'].shape[1]
    return ops.grouped_match(t['kp'], t['g'], t['qp'], t['cand'], t['remaining'], t['offsets'], d['H'], 1.0 / float(np.sqrt(np.float32(A))),
                             ALPHA, BETA, use_weight, use_penalty)


def run_old(ops, d, use_weight, use_penalty):
    """lime_interest_match_f32 per group: B = 1 row with the group's history, N = the group's pairs."""
    H, (A, D) = d['H'], (d['kp'].shape[1], d['g'].shape[1])
    t = {k: torch.from_numpy(v).cuda() for k, v in d.items() if k not in ('H', 'offsets')}
    out = torch.zeros(d['qp'].shape[0], dtype=torch.float32, device='cuda')
    for i in range(len(d['offsets']) - 1):
        lo, hi = int(d['offsets'][i]), int(d['offsets'][i + 1])
        if hi == lo:
            continue
        _, logits = ops.interest_match(t['kp'][i * H:(i + 1) * H].reshape(-1), t['qp'][lo:hi].reshape(-1), t['g'][i * H:(i + 1) * H].reshape(-1),
                                       t['cand'][lo:hi].reshape(-1), t['remaining'][lo:hi], 1, hi - lo, H, A, D,
                                       1.0 / float(np.sqrt(np.float32(A))), ALPHA, BETA, use_weight, use_penalty, want_logits=True, want_user=False)
        out[lo:hi] = logits.view(-1)
    return out


def check_error(ops, d, use_weight, use_penalty, what):
    want = reference(d, use_weight, use_penalty)
    new = run_new(ops, d, use_weight, use_penalty).cpu().numpy()
    old = run_old(ops, d, use_weight, use_penalty).cpu().numpy()
    assert np.isfinite(new).all()
    e_new, e_old = float(np.abs(new - want).max()), float(np.abs(old - want).max())
    ulp = float(np.spacing(np.float32(np.abs(want).max())))
    print('%s: grouped match max err %.3e, interest match max err %.3e, one ulp of max |logit| %.3e (bound %.3e)' % (
        what, e_new, e_old, ulp, 2 * e_old + ulp))
    assert e_new <= 2 * e_old + ulp, '%s: %.3e > 2 x %.3e + %.3e' % (what, e_new, e_old, ulp)
    return new


@pytest.mark.parametrize('A,D', [(8, 12), (40, 24), (400, 400)])
@pytest.mark.parametrize('H', [1, 7, 16, 50, 128])
def test_sizes_against_float64(ops, H, A, D):
    check_error(ops, make(H, A, D, seed=H + A), True, True, 'H %d A %d D %d' % (H, A, D))


@pytest.mark.parametrize('use_weight,use_penalty', [(False, False), (True, False), (True, True), (False, True)])
def test_weight_and_penalty_switches(ops, use_weight, use_penalty):
    check_error(ops, make(50, 400, 400, seed=11), use_weight, use_penalty, 'weight %s penalty %s' % (use_weight, use_penalty))


@pytest.mark.parametrize('use_penalty', [True, False])
def test_saturated_weights(ops, use_penalty):
    """|remaining| beyond 350 / alpha: sigmoid gives exactly 0 and exactly 1 in fp32 -- with the expired penalty an expired news scores
    exactly zero, a fresh one its unweighted logit; small values beside them."""
    sizes = [5, 70]
    P = sum(sizes)
    r = np.random.default_rng(5).uniform(-2.0, 2.0, size=P)
    r[0::3] = -600.0
    r[1::3] = 600.0
    d = make(7, 40, 24, sizes=sizes, seed=12, remaining=r)
    got = check_error(ops, d, True, use_penalty, 'saturated, penalty %s' % use_penalty)
    plain = run_new(ops, d, False, False).cpu().numpy()
    if use_penalty:
        assert (got[0::3] == 0.0).all(), 'a weight of exactly 0 must give an exact zero'
    else:
        assert np.array_equal(got[0::3], plain[0::3])                      # sigmoid(alpha |r|) = 1
    assert np.array_equal(got[1::3], plain[1::3])
    assert (np.abs(got[2::3]) < np.abs(plain[2::3])).all()


def test_a_pairs_bits_do_not_depend_on_the_layout(ops):
    """The same pairs in another group order, in another order inside their group, between other neighbours and under another P."""
    H, A, D = 50, 400, 400
    d = make(H, A, D, seed=21)
    first = run_new(ops, d, True, True).cpu().numpy()
    assert np.array_equal(first, run_new(ops, d, True, True).cpu().numpy()), 'two runs differ'
    rng = np.random.default_rng(22)
    perm = [4, 2, 5, 0, 1, 3]                                              # new place -> old group
    extra = make(H, A, D, sizes=[37], seed=23)                             # a stranger group in front
    sizes, rows = [37], [np.arange(37) + 10 ** 6]
    for i in perm:
        lo, hi = int(d['offsets'][i]), int(d['offsets'][i + 1])
        members = rng.permutation(np.arange(lo, hi))
        rows.append(members)
        sizes.append(hi - lo)
    rows = np.concatenate(rows)
    old = rows < 10 ** 6
    pick = lambda name: np.concatenate([extra[name], d[name][rows[old]]])
    grp = lambda name: np.concatenate([extra[name]] + [d[name][i * H:(i + 1) * H] for i in perm])
    d2 = dict(kp=grp('kp'), g=grp('g'), qp=pick('qp'), cand=pick('cand'), remaining=pick('remaining'), H=H,
              offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    second = run_new(ops, d2, True, True).cpu().numpy()
    assert second.shape[0] == first.shape[0] + 37
    assert np.array_equal(second[37:].view(np.int32), first[rows[old]].view(np.int32))


def test_offsets_behind_the_last_pair_are_clamped(ops):
    d = make(7, 8, 12, sizes=[3, 4], seed=31)
    full = run_new(ops, d, False, False).cpu().numpy()
    d['offsets'] = np.array([0, 3, 1 << 40], dtype=np.int64)               # behind P: clamped to P
    assert np.array_equal(run_new(ops, d, False, False).cpu().numpy(), full)


def test_out_of_range_dims_are_unsupported(ops):
    from lime_cikm25_amd import _lib
    lib = _lib.load()
    z = lambda *s: torch.zeros(*s, device='cuda')
    off = torch.tensor([0, 1], dtype=torch.int64, device='cuda')
    for H, A, D in ((129, 8, 8), (4, 2052, 8), (4, 8, 2052), (4, 6, 8)):
        kp, g, qp, cand, out = z(H, A), z(H, D), z(1, A), z(1, D), z(1)
        st = lib.lime_grouped_match_f32(kp.data_ptr(), g.data_ptr(), qp.data_ptr(), cand.data_ptr(), None, off.data_ptr(), out.data_ptr(),
                                        1, 1, H, A, D, 1.0, 0.0, 0.0, 0, 0, None)
        assert st == -2, (H, A, D, st)                                     # LIME_ERR_UNSUPPORTED
    with pytest.raises(_lib.LimeHipError, match='128'):
        ops.grouped_match(z(129, 8), z(129, 8), z(1, 8), z(1, 8), None, off, 129, 1.0)
