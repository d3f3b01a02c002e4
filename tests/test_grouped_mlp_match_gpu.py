"""lime_grouped_mlp_match_f32 and its indexed twin (csrc/grouped_mlp_match_f32.hip) on the MI355X against a float64 host statement of
the MLP click predictor behind the history-vs-candidate attention,

    s[h] = kp[i, h] . qp[p] / sqrt(A),  a = softmax_h(s),  user = sum_h a[h] g[i, h],
    logit[p] = relu(cat[user, cand[p]] . mlp_w^T + mlp_b) . out_w + out_b,

with the COMPOSED form -- lime_interest_match_f32's user rows per group, then ops.mlp_predictor on lime_linear_f32 -- on the same
inputs as the yardstick of the error: the fused kernel re-associates the composed form's sums (W_u (sum_h a g) becomes sum_h a (W_u g)),
so it may be off by at most twice the composed form's own maximum error plus one ulp of the largest |logit| (the margin
tests/test_grouped_match_gpu.py gives a re-associated sum).  Both errors are printed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GROUPS = [0, 1, 63, 64, 65, 130]          # pairs per group, in one call: empty, one, around the 64-pair tile, three tiles


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from lime_cikm25_amd import ops as _ops
    from lime_cikm25_amd import _lib
    _lib.load()
    return _ops


def make(H, A, Dh, sizes=GROUPS, seed=0):
    """The function's own inputs: D = 2 Dh as in the model (mlp: 2 D -> D // 2)."""
    rng = np.random.default_rng(seed)
    G, P, D = len(sizes), int(sum(sizes)), 2 * Dh
    u = lambda *s: rng.uniform(-1.0, 1.0, size=s).astype(np.float32)
    return dict(kp=u(G * H, A), g=u(G * H, D), qp=u(P, A), cand=u(P, D), mlp_w=(u(Dh, 2 * D) / np.float32(np.sqrt(D))), mlp_b=u(Dh),
                out_w=u(Dh), out_b=u(1), H=H, offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))


def reference(d):
    """float64 logits [P]."""
    H, A, D = d['H'], d['kp'].shape[1], d['g'].shape[1]
    f = lambda k: d[k].astype(np.float64)
    out = np.zeros(d['qp'].shape[0])
    for i in range(len(d['offsets']) - 1):
        lo, hi = int(d['offsets'][i]), int(d['offsets'][i + 1])
        if hi == lo:
            continue
        s = f('qp')[lo:hi] @ f('kp')[i * H:(i + 1) * H].T / np.sqrt(float(A))             # [n, H]
        a = np.exp(s - s.max(axis=1, keepdims=True))
        a /= a.sum(axis=1, keepdims=True)
        user = a @ f('g')[i * H:(i + 1) * H]                                              # [n, D]
        hidden = np.maximum(np.concatenate([user, f('cand')[lo:hi]], axis=1) @ f('mlp_w').T + f('mlp_b'), 0.0)
        out[lo:hi] = hidden @ f('out_w') + f('out_b')[0]
    return out


def scale_of(d):
    return 1.0 / float(np.sqrt(np.float32(d['kp'].shape[1])))


def operands(ops, d):
    """The kernel's operands from the function's inputs, as the model makes them: gu and nw on lime_linear_f32."""
    t = {k: torch.from_numpy(v).cuda() for k, v in d.items() if k != 'H'}
    D = d['g'].shape[1]
    t['gu'] = ops.linear(t['g'], t['mlp_w'][:, :D], None)
    t['nw'] = ops.linear(t['cand'], t['mlp_w'][:, D:], t['mlp_b'])
    return t


def run_fused(ops, d, t=None):
    t = operands(ops, d) if t is None else t
    return ops.grouped_mlp_match(t['kp'], t['gu'], t['qp'], t['nw'], t['out_w'], t['out_b'], t['offsets'], d['H'], scale_of(d))


def run_composed(ops, d):
    """lime_interest_match_f32 per group (B = 1 row with the group's history, N = the group's pairs) for the user rows, then the
    predictor on lime_linear_f32."""
    H, (A, D) = d['H'], (d['kp'].shape[1], d['g'].shape[1])
    t = {k: torch.from_numpy(v).cuda() for k, v in d.items() if k not in ('H', 'offsets')}
    out = torch.zeros(d['qp'].shape[0], dtype=torch.float32, device='cuda')
    for i in range(len(d['offsets']) - 1):
        lo, hi = int(d['offsets'][i]), int(d['offsets'][i + 1])
        if hi == lo:
            continue
        user, _ = ops.interest_match(t['kp'][i * H:(i + 1) * H].reshape(-1), t['qp'][lo:hi].reshape(-1), t['g'][i * H:(i + 1) * H].reshape(-1),
                                     t['cand'][lo:hi].reshape(-1), None, 1, hi - lo, H, A, D, scale_of(d), 0.0, 0.0, False, False,
                                     want_logits=False, want_user=True)
        out[lo:hi] = ops.mlp_predictor(user.view(hi - lo, D), t['cand'][lo:hi], t['mlp_w'], t['mlp_b'], t['out_w'], t['out_b'])
    return out


@pytest.mark.parametrize('A,Dh', [(8, 6), (40, 12), (400, 150), (400, 200), (400, 450)])
@pytest.mark.parametrize('H', [1, 7, 16, 50, 128])
def test_sizes_against_float64(ops, H, A, Dh):
    d = make(H, A, Dh, seed=H + A + Dh)
    want = reference(d)
    new = run_fused(ops, d).cpu().numpy()
    old = run_composed(ops, d).cpu().numpy()
    assert np.isfinite(new).all()
    e_new, e_old = float(np.abs(new - want).max()), float(np.abs(old - want).max())
    ulp = float(np.spacing(np.float32(np.abs(want).max())))
    print('H %d A %d Dh %d: fused max err %.3e, composed max err %.3e, one ulp of max |logit| %.3e (bound %.3e)' % (
        H, A, Dh, e_new, e_old, ulp, 2 * e_old + ulp))
    assert e_new <= 2 * e_old + ulp, 'H %d A %d Dh %d: %.3e > 2 x %.3e + %.3e' % (H, A, Dh, e_new, e_old, ulp)


def _call(lib, t, H, out, P=None, G=None, A=None, Dh=None, index=None, n=0, scale=1.0):
    A = t['kp'].shape[1] if A is None else A
    Dh = t['gu'].shape[1] if Dh is None else Dh
    G = t['offsets'].numel() - 1 if G is None else G
    P = out.numel() if P is None else P
    ptr = lambda x: None if x is None else x.data_ptr()
    if index is None:
        return lib.lime_grouped_mlp_match_f32(ptr(t['kp']), ptr(t['gu']), ptr(t['qp']), ptr(t['nw']), ptr(t['out_w']), ptr(t['out_b']),
                                              ptr(t['offsets']), ptr(out), G, P, H, A, Dh, scale, None)
    return lib.lime_grouped_mlp_match_indexed_f32(ptr(t['kp']), ptr(t['gu']), ptr(t['qp']), ptr(t['nw']), ptr(t['out_w']), ptr(t['out_b']),
                                                  ptr(t['offsets']), ptr(index), n, ptr(out), G, P, H, A, Dh, scale, None)


def test_pairs_outside_every_group_are_not_written(ops):
    from lime_cikm25_amd import _lib
    lib = _lib.load()
    d = make(7, 40, 12, sizes=[3, 70, 4], seed=41)
    t = operands(ops, d)
    full = run_fused(ops, d, t)
    t['offsets'] = torch.tensor([2, 3, 70, 75], dtype=torch.int64, device='cuda')         # pairs 0, 1, 75, 76 belong to no group
    marker = 12345.0
    out = torch.full((77,), marker, dtype=torch.float32, device='cuda')
    assert _call(lib, t, 7, out, scale=scale_of(d)) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[[0, 1, 75, 76]] == marker).all()
    assert (got[2:75] != marker).all() and np.isfinite(got).all()
    assert got[2] == full.cpu().numpy()[2]                                                # pair 2 is still a pair of group 0


def test_indexed_form_is_the_plain_form_on_gathered_rows_and_clamps(ops):
    d = make(50, 400, 150, seed=51)
    t = operands(ops, d)
    P = t['qp'].shape[0]
    n = 97
    rng = np.random.default_rng(52)
    qp_table, nw_table = torch.from_numpy(rng.uniform(-1, 1, size=(n, 400)).astype(np.float32)).cuda(), \
        torch.from_numpy(rng.uniform(-1, 1, size=(n, 150)).astype(np.float32)).cuda()
    index = torch.from_numpy(rng.integers(0, n, size=P).astype(np.int32)).cuda()
    args = (t['out_w'], t['out_b'], t['offsets'], d['H'], scale_of(d))
    plain = ops.grouped_mlp_match(t['kp'], t['gu'], qp_table[index.long()].contiguous(), nw_table[index.long()].contiguous(), *args)
    indexed = ops.grouped_mlp_match(t['kp'], t['gu'], qp_table, nw_table, *args, index=index)
    assert torch.equal(plain, indexed)
    bad = index.clone()
    bad[5], bad[100], bad[200] = -7, n, 2 ** 31 - 1                                       # clamped to 0, n - 1, n - 1
    want = index.clone()
    want[5], want[100], want[200] = 0, n - 1, n - 1
    assert torch.equal(ops.grouped_mlp_match(t['kp'], t['gu'], qp_table, nw_table, *args, index=bad),
                       ops.grouped_mlp_match(t['kp'], t['gu'], qp_table, nw_table, *args, index=want))
    # a table longer than n: rows behind n are never read
    short = ops.grouped_mlp_match(t['kp'], t['gu'], qp_table, nw_table, *args, index=bad, n=50)
    assert torch.equal(short, ops.grouped_mlp_match(t['kp'], t['gu'], qp_table[:50].contiguous(), nw_table[:50].contiguous(), *args,
                                                    index=bad.clamp(0, 49)))


def test_a_pairs_bits_do_not_depend_on_the_layout(ops):
    """The same pairs in another group order, in another order inside their group, between other neighbours and under another P; and
    two runs give the same bits."""
    H, A, Dh = 50, 400, 150
    d = make(H, A, Dh, seed=21)
    t = operands(ops, d)
    first = run_fused(ops, d, t)
    assert torch.equal(first, run_fused(ops, d, t)), 'two runs differ'
    first = first.cpu().numpy()
    rng = np.random.default_rng(22)
    perm = [4, 2, 5, 0, 1, 3]                                              # new place -> old group
    rows, sizes = [], [37]
    for i in perm:
        lo, hi = int(d['offsets'][i]), int(d['offsets'][i + 1])
        rows.append(rng.permutation(np.arange(lo, hi)))
        sizes.append(hi - lo)
    rows = torch.from_numpy(np.concatenate(rows)).cuda()
    u = lambda *s: torch.from_numpy(rng.uniform(-1, 1, size=s).astype(np.float32)).cuda()
    grp = lambda x, w: torch.cat([u(H, w)] + [x[i * H:(i + 1) * H] for i in perm])        # a stranger group in front
    t2 = dict(t, kp=grp(t['kp'], A), gu=grp(t['gu'], Dh), qp=torch.cat([u(37, A), t['qp'][rows]]), nw=torch.cat([u(37, Dh), t['nw'][rows]]),
              offsets=torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).cuda())
    second = run_fused(ops, d, t2).cpu().numpy()
    assert second.shape[0] == first.shape[0] + 37
    assert np.array_equal(second[37:].view(np.int32), first[rows.cpu().numpy()].view(np.int32))


def test_offsets_behind_the_last_pair_are_clamped(ops):
    d = make(7, 8, 6, sizes=[3, 4], seed=31)
    t = operands(ops, d)
    full = run_fused(ops, d, t)
    t['offsets'] = torch.tensor([0, 3, 1 << 40], dtype=torch.int64, device='cuda')        # behind P: clamped to P
    assert torch.equal(run_fused(ops, d, t), full)


def test_bad_arguments_are_refused_before_any_launch(ops):
    from lime_cikm25_amd import _lib
    lib = _lib.load()
    z = lambda *s: torch.zeros(*s, device='cuda')
    off = torch.tensor([0, 1], dtype=torch.int64, device='cuda')
    idx = torch.zeros(1, dtype=torch.int32, device='cuda')

    def tensors(H, A, Dh):
        return dict(kp=z(H, A), gu=z(H, Dh), qp=z(1, A), nw=z(1, Dh), out_w=z(Dh), out_b=z(1), offsets=off)
    for H, A, Dh in ((129, 8, 8), (4, 2052, 8), (4, 8, 2050), (4, 6, 8), (4, 8, 7)):      # LIME_ERR_UNSUPPORTED
        t = tensors(H, A, Dh)
        assert _call(lib, t, H, z(1)) == -2, (H, A, Dh)
        assert _call(lib, t, H, z(1), index=idx, n=1) == -2, (H, A, Dh)
    t = tensors(4, 8, 6)
    for name in ('kp', 'gu', 'qp', 'nw', 'out_w', 'offsets'):                             # NULL pointers: LIME_ERR_BAD_ARG
        assert _call(lib, dict(t, **{name: None}), 4, z(1), G=1, A=8, Dh=6) == -1, name
    assert _call(lib, dict(t, out_b=None), 4, z(1)) == 0                                  # no bias is a bias of 0
    assert _call(lib, t, 0, z(1)) == -1 and _call(lib, t, 4, z(1), P=-1) == -1            # bad dims
    assert _call(lib, dict(t, kp=z(4 * 8 + 1)[1:].view(4, 8)), 4, z(1)) == -1             # kp not 16-byte aligned
    assert _call(lib, dict(t, nw=z(7)[1:].view(1, 6)), 4, z(1)) == -1                     # nw not 8-byte aligned
    assert _call(lib, t, 4, z(1), index=None) == 0
    assert _call(lib, t, 4, z(1), index=idx, n=0) == -1                                   # pairs index an empty table
    assert _call(lib, t, 4, z(1), index=idx, n=-1) == -1
    torch.cuda.synchronize()
    with pytest.raises(_lib.LimeHipError, match='128'):
        ops.grouped_mlp_match(z(129, 8), z(129, 6), z(1, 8), z(1, 6), z(6), z(1), off, 129, 1.0)
    with pytest.raises(ValueError, match='G \\* H rows'):
        ops.grouped_mlp_match(z(5, 8), z(5, 6), z(1, 8), z(1, 6), z(6), z(1), off, 4, 1.0)
    with pytest.raises(ValueError, match='nw'):
        ops.grouped_mlp_match(z(4, 8), z(4, 6), z(1, 8), z(1, 8), z(6), z(1), off, 4, 1.0)
