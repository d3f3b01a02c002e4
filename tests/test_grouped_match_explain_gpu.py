"""lime_grouped_match_explain_f32 (csrc/grouped_match_explain_f32.hip) on the MI355X, through ``ops.grouped_match_explain``:

  * logits carry the BITS of ``ops.grouped_match`` on the same operands, in the plain, the indexed and the occurrence-composed form;
  * attn and contrib against ``recommend.explain_pairs`` (fp64), with the bar tests/test_grouped_match_gpu.py sets for the logits: at
    most twice the error of the same quantities composed in torch fp32 on the same operands, plus one ulp of the largest magnitude;
  * two derived bounds, the sums made in fp64, u = 2^-24, T the history tiles (1, 2, 4, 8 for H <= 16, 32, 64, 128):
        |sum_h attn - 1|          <= (4 T + 3) u                   -- den is a chain of 4 T + 1 additions, each quotient one rounding,
        |sum_h contrib - logit|   <= (4 T + 8) u sum_h |contrib|   -- 4 T + 2 roundings in the kernel's own sum chain, two for the
                                                                       division and the weight, three per written contribution, one of
                                                                       slack for the second-order terms;
  * top_slot / top_value are EXACTLY ``recommend.top_slots`` of the kernel's own dense output under the mask (no rounding can reorder
    anything), with a tie between two bit-identical history rows and an all-zero mask row;
  * weight against logits / base, the layout independence of a pair's bits, NULL dense outputs, clamped plans and the entry's statuses.

Groups of 65 (a second, partial tile), 1, 30 and 0 pairs; hist_div = 2 with two mask rows, the second all zero."""
import numpy as np
import pytest
import torch

from lime_cikm25_amd import recommend

pytestmark = pytest.mark.gpu

SIZES = [65, 1, 30, 0]
ALPHA, BETA = 0.7, 0.3
U24 = 2.0 ** -24
SHAPES = [(H, A, D) for H in (1, 5, 16, 17, 50, 128) for A, D in ((4, 4), (20, 36), (200, 400))]
N_TABLE, N_OCC = 41, 7


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from lime_cikm25_amd import ops as _ops
    from lime_cikm25_amd import _lib
    _lib.load()
    return _ops


def tiles(H):
    return 1 if H <= 16 else 2 if H <= 32 else 4 if H <= 64 else 8


_MADE = {}


def make(H, A, D, form='plain', sizes=SIZES, seed=0):
    """The operands of one call (numpy) -- made once per shape and form, never changed.  Group 0 has two bit-identical history rows
    (slots 0 and 1, both masked in); remaining lies on both sides of 0."""
    key = (H, A, D, form, tuple(sizes), seed)
    if key in _MADE:
        return _MADE[key]
    rng = np.random.default_rng(1000 * H + A + seed)
    G, P = len(sizes), int(sum(sizes))
    u = lambda *s: rng.uniform(-1.0, 1.0, size=s).astype(np.float32)
    d = dict(kp=u(G * H, A), g=u(G * H, D), H=H, scale=1.0 / float(np.sqrt(np.float32(A))),
             remaining=rng.uniform(-3.0, 3.0, size=P).astype(np.float32), offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    if H > 1:
        d['kp'][1], d['g'][1] = d['kp'][0], d['g'][0]
    mask = np.zeros(((G + 1) // 2, H), dtype=bool)
    mask[0] = rng.uniform(size=H) < 0.7
    mask[0, :2] = True
    d['mask'] = mask                                                       # (row 1 and up: all zero)
    if form == 'plain':
        d.update(qp=u(P, A), cand=u(P, D))
    else:
        d.update(qp=u(N_TABLE, A), cand=u(N_TABLE, D), index=rng.integers(0, N_TABLE, size=P).astype(np.int32))
        if form == 'occurrence':
            d.update(qt=u(N_OCC, A), ct=u(N_OCC, D), occ=rng.integers(0, N_OCC, size=P).astype(np.int32))
    _MADE[key] = d
    return d


def extra(d):
    return {k: d[k] for k in ('index', 'occ', 'qt', 'ct') if k in d}


def cuda(d):
    return {k: torch.from_numpy(v).cuda() for k, v in d.items() if isinstance(v, np.ndarray)}


def run(ops, d, m=3, by='contribution', use_weight=True, use_penalty=True, dense=True, hist_div=2, mask='own'):
    t = cuda(d)
    r = ops.grouped_match_explain(t['kp'], t['g'], t['qp'], t['cand'], t['remaining'], t['offsets'], d['H'], d['scale'], ALPHA, BETA,
                                  use_weight, use_penalty, mask=t['mask'] if isinstance(mask, str) else mask, hist_div=hist_div, m=m, by=by,
                                  dense=dense, **{k: t[k] for k in extra(d)})
    torch.cuda.synchronize()
    return r


def twin(ops, d, use_weight=True, use_penalty=True):
    t = cuda(d)
    return ops.grouped_match(t['kp'], t['g'], t['qp'], t['cand'], t['remaining'], t['offsets'], d['H'], d['scale'], ALPHA, BETA, use_weight,
                             use_penalty, **{k: t[k] for k in extra(d)})


def host(d, m=3, by='contribution', use_weight=True, use_penalty=True, hist_div=2):
    return recommend.explain_pairs(d['kp'], d['g'], d['qp'], d['cand'], d['remaining'], d['offsets'], d['H'], d['scale'], ALPHA, BETA,
                                   use_weight, use_penalty, d['mask'], hist_div, m, by, **extra(d))


def torch_terms(d, use_weight, use_penalty):
    """attn and contrib [P, H] composed in torch fp32 on the device: gather the groups' rows, two bmm, softmax, the weight."""
    t, H = cuda(d), d['H']
    qp, cand = t['qp'], t['cand']
    if 'index' in d:
        qp, cand = qp[t['index'].long()], cand[t['index'].long()]
        if 'occ' in d:
            qp, cand = qp + t['qt'][t['occ'].long()], cand + t['ct'][t['occ'].long()]
    sizes = torch.from_numpy(np.diff(d['offsets'])).cuda()
    group = torch.repeat_interleave(torch.arange(sizes.numel(), device='cuda'), sizes)
    s = torch.bmm(t['kp'].view(-1, H, qp.shape[1])[group], qp.unsqueeze(2)).squeeze(2) * d['scale']
    a = torch.softmax(s, dim=1)
    mm = torch.bmm(t['g'].view(-1, H, cand.shape[1])[group], cand.unsqueeze(2)).squeeze(2)
    r = t['remaining']
    if not use_weight:
        w = torch.ones_like(r)
    elif use_penalty:
        w = torch.sigmoid(ALPHA * r) * torch.where(r >= 0, torch.ones_like(r), torch.full_like(r, BETA))
    else:
        w = torch.sigmoid(ALPHA * r.abs())
    return a.cpu().numpy(), ((a * mm) * w.unsqueeze(1)).cpu().numpy()


def eligible(d, hist_div=2):
    sizes = np.diff(d['offsets'])
    group = np.repeat(np.arange(len(sizes)), sizes)
    return d['mask'][group // hist_div]


def check_dense(ops, d, what, use_weight=True, use_penalty=True):
    """The dense outputs of one run against fp64, under the torch-fp32 bar, and the two sum bounds -> the run."""
    m = min(3, d['H'])
    got = run(ops, d, m=m, use_weight=use_weight, use_penalty=use_penalty)
    want = host(d, m=m, use_weight=use_weight, use_penalty=use_penalty)
    ta, tc = torch_terms(d, use_weight, use_penalty)
    attn, contrib, logits = (x.cpu().numpy() for x in (got.attn, got.contrib, got.logits))
    assert np.isfinite(attn).all() and np.isfinite(contrib).all() and (attn >= 0).all()
    for name, mine, ref, theirs in (('attn', attn, want.attn, ta), ('contrib', contrib, want.contrib, tc)):
        e_new, e_old = float(np.abs(mine - ref).max()), float(np.abs(theirs - ref).max())
        ulp = float(np.spacing(np.float32(np.abs(ref).max())))
        print('%s %s: kernel max err %.3e, torch fp32 max err %.3e, one ulp of the largest %.3e (bound %.3e)' % (
            what, name, e_new, e_old, ulp, 2 * e_old + ulp))
        assert e_new <= 2 * e_old + ulp, '%s %s: %.3e > 2 x %.3e + %.3e' % (what, name, e_new, e_old, ulp)
    T = tiles(d['H'])
    one = np.abs(attn.astype(np.float64).sum(axis=1) - 1.0).max()
    gap = np.abs(contrib.astype(np.float64).sum(axis=1) - logits.astype(np.float64))
    room = (4 * T + 8) * U24 * np.abs(contrib.astype(np.float64)).sum(axis=1)
    print('%s: |sum attn - 1| max %.3e (bound %.3e); |sum contrib - logit| / bound max %.3f' % (
        what, one, (4 * T + 3) * U24, float((gap / np.maximum(room, 1e-300)).max())))
    assert one <= (4 * T + 3) * U24
    assert (gap <= room).all()
    check_selection(d, got, m, 'contribution')
    return got


def check_selection(d, got, m, by, hist_div=2):
    """top_slot / top_value are the host selection of the kernel's OWN dense output, bit for bit."""
    values = (got.contrib if by == 'contribution' else got.attn).cpu().numpy()
    slot, top = recommend.top_slots(values, eligible(d, hist_div), m)
    assert np.array_equal(got.top_slot.cpu().numpy(), slot)
    assert np.array_equal(got.top_value.cpu().numpy().view(np.int32), top.view(np.int32))


@pytest.mark.parametrize('form', ['plain', 'indexed', 'occurrence'])
@pytest.mark.parametrize('H,A,D', SHAPES)
def test_logits_have_the_twins_bits_and_the_terms_hold_to_fp64(ops, H, A, D, form):
    d = make(H, A, D, form)
    got = check_dense(ops, d, 'H %d A %d D %d %s' % (H, A, D, form))
    assert torch.equal(got.logits.view(torch.int32), twin(ops, d).view(torch.int32))
    P = got.logits.numel()
    assert got.attn.shape == got.contrib.shape == (P, H) and got.base.shape == got.weight.shape == (P,)


@pytest.mark.parametrize('H,A,D', SHAPES)
def test_the_selection_is_the_host_rule_on_the_kernels_own_terms(ops, H, A, D):
    d = make(H, A, D)
    first = None
    for by in ('contribution', 'attention'):
        for m in [m for m in (1, 3, 16) if m <= H]:
            got = run(ops, d, m=m, by=by)
            assert got.top_slot.shape == got.top_value.shape == (sum(SIZES), m) and got.top_slot.dtype == torch.int32
            check_selection(d, got, m, by)
            slot = got.top_slot.cpu().numpy()
            assert (slot[66:] == -1).all() and (got.top_value[66:] == 0).all()          # the all-zero mask row names nothing
            if H > 1:                                                               # rows 0 and 1 of group 0 tie: 0 right before 1
                c = got.contrib.cpu().numpy()
                assert np.array_equal(c[:65, 0].view(np.int32), c[:65, 1].view(np.int32))
                if m >= 2:
                    for p in range(65):
                        at = slot[p].tolist()
                        assert (0 in at) == (1 in at) or at[-1] == 0
                        if 1 in at:
                            assert at.index(1) == at.index(0) + 1
            live = int(d['mask'][0].sum())
            assert (slot[:66, :min(m, live)] >= 0).all() and (slot[:66, live:] == -1).all()
            # nothing but the selection moves with m and by
            if first is None:
                first = got
            for a, b in ((got.logits, first.logits), (got.attn, first.attn), (got.contrib, first.contrib), (got.weight, first.weight)):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('use_weight,use_penalty', [(False, False), (True, False), (True, True), (False, True)])
@pytest.mark.parametrize('form', ['plain', 'occurrence'])
def test_weight_and_penalty_switches(ops, form, use_weight, use_penalty):
    d = make(50, 200, 400, form)
    got = check_dense(ops, d, '%s weight %s penalty %s' % (form, use_weight, use_penalty), use_weight, use_penalty)
    assert torch.equal(got.logits.view(torch.int32), twin(ops, d, use_weight, use_penalty).view(torch.int32))
    logits, base, weight = (x.cpu().numpy().astype(np.float64) for x in (got.logits, got.base, got.weight))
    if not use_weight:
        assert (weight == 1.0).all() and np.array_equal(logits, base)
        return
    assert (d['remaining'] < 0).any() and (d['remaining'] > 0).any()
    # logits = fl(base weight): one rounding, so logits / base is the weight to one part in 2^24
    ok = np.abs(base) > 1e-30
    assert ok.sum() > len(base) // 2
    assert (np.abs(logits[ok] / base[ok] - weight[ok]) <= U24 * weight[ok] * (1 + 1e-6)).all()
    # and the weight itself: an fp32 exp, a sum and a quotient behind the fp64 statement -- within 1e-6 of it
    want = recommend.lifetime_weight(d['remaining'], ALPHA, BETA, use_weight, use_penalty)
    assert np.abs(weight - want).max() <= 1e-6 * np.abs(want).max()


def test_a_pairs_bits_do_not_depend_on_the_run_or_the_layout(ops):
    """Two runs; then the same pairs in another group order, in another order inside their group, behind a stranger group, under a
    larger P (hist_div = 1: every group brings its own mask row)."""
    H, A, D = 50, 200, 400
    d = dict(make(H, A, D, sizes=[65, 1, 30, 0, 37], seed=3))
    rng = np.random.default_rng(8)
    d['mask'] = rng.uniform(size=(5, H)) < 0.6
    names = ('logits', 'base', 'weight', 'attn', 'contrib', 'top_slot', 'top_value')
    first, again = run(ops, d, hist_div=1), run(ops, d, hist_div=1)
    for n in names:
        assert torch.equal(getattr(first, n).view(torch.int32), getattr(again, n).view(torch.int32)), n
    perm = [4, 2, 0, 3, 1]                                                 # new place -> old group
    other = make(H, A, D, sizes=[37], seed=4)
    sizes, rows = [37], []
    for i in perm:
        lo, hi = int(d['offsets'][i]), int(d['offsets'][i + 1])
        rows.append(rng.permutation(np.arange(lo, hi)))
        sizes.append(hi - lo)
    rows = np.concatenate(rows)
    pick = lambda name: np.concatenate([other[name], d[name][rows]])
    grp = lambda name: np.concatenate([other[name]] + [d[name][i * H:(i + 1) * H] for i in perm])
    d2 = dict(kp=grp('kp'), g=grp('g'), qp=pick('qp'), cand=pick('cand'), remaining=pick('remaining'), H=H, scale=d['scale'],
              mask=np.concatenate([np.ones((1, H), dtype=bool), d['mask'][perm]]), offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    second = run(ops, d2, hist_div=1)
    at = torch.from_numpy(rows).cuda()
    for n in names:
        assert torch.equal(getattr(second, n)[37:].view(torch.int32), getattr(first, n)[at].view(torch.int32)), n


def test_null_dense_outputs_leave_the_others_unchanged(ops):
    d = make(17, 20, 36, 'indexed')
    full, bare = run(ops, d), run(ops, d, dense=False)
    assert bare.attn is None and bare.contrib is None
    for n in ('logits', 'base', 'weight', 'top_slot', 'top_value'):
        assert torch.equal(getattr(full, n).view(torch.int32), getattr(bare, n).view(torch.int32)), n
    free = run(ops, d, mask=None)                                          # no mask: every slot is eligible
    slot, top = recommend.top_slots(free.contrib.cpu().numpy(), np.ones((sum(SIZES), 17), dtype=bool), 3)
    assert np.array_equal(free.top_slot.cpu().numpy(), slot) and np.array_equal(free.top_value.cpu().numpy().view(np.int32), top.view(np.int32))


def test_a_bad_plan_is_clamped_like_the_twins(ops):
    """index outside [0, n), occ outside [0, n_occ) and an offset behind P read and write in range: the results are those of the
    clamped plan.  Nothing here reads out of bounds -- the kernel clamps before it loads."""
    d = dict(make(16, 20, 36, 'occurrence'))
    P = sum(SIZES)
    odd = np.arange(P) % 3 == 0
    wild = dict(d, index=np.where(odd, np.int32(N_TABLE + 5), d['index']).astype(np.int32),
                occ=np.where(odd, np.int32(-3), d['occ']).astype(np.int32), offsets=np.array([0, 65, 66, 1 << 40, 1 << 41], dtype=np.int64))
    tame = dict(d, index=np.where(odd, np.int32(N_TABLE - 1), d['index']).astype(np.int32),
                occ=np.where(odd, np.int32(0), d['occ']).astype(np.int32), offsets=np.array([0, 65, 66, P, P], dtype=np.int64))
    a, b = run(ops, wild), run(ops, tame)
    for n in ('logits', 'base', 'weight', 'attn', 'contrib', 'top_slot', 'top_value'):
        assert torch.equal(getattr(a, n).view(torch.int32), getattr(b, n).view(torch.int32)), n
    assert torch.equal(a.logits.view(torch.int32), twin(ops, wild).view(torch.int32))


def test_the_entry_returns_its_statuses(ops):
    from lime_cikm25_amd import _lib
    lib = _lib.load()
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device='cuda')
    off = torch.tensor([0, 1], dtype=torch.int64, device='cuda')

    def call(H=32, m=3, kp_shift=0):
        kp, g, qp, cand = z(H * 8 + 4), z(H, 8), z(1, 8), z(1, 8)
        out = [z(1), z(1), z(1), z(1, H), z(1, H), z(1, 16, dtype=torch.int32), z(1, 16)]
        return lib.lime_grouped_match_explain_f32(kp.data_ptr() + kp_shift, g.data_ptr(), qp.data_ptr(), cand.data_ptr(), None, None, None,
                                                  off.data_ptr(), None, 0, None, 0, None, 1, m, 0, *[o.data_ptr() for o in out], 1, 1, H, 8, 8,
                                                  1.0, 0.0, 0.0, 0, 0, None)
    assert call(m=0) == -1 and call(m=17) == -2 and call(H=8, m=9) == -1 and call(H=129) == -2 and call(kp_shift=4) == -1
    assert call() == 0 and call(H=16, m=16) == 0
    torch.cuda.synchronize()
    with pytest.raises(_lib.LimeHipError, match='m 17'):
        ops.grouped_match_explain(z(32, 8), z(32, 8), z(1, 8), z(1, 8), None, off, 32, 1.0, m=17)
    with pytest.raises(ValueError, match='mask must be'):
        ops.grouped_match_explain(z(32, 8), z(32, 8), z(1, 8), z(1, 8), None, off, 32, 1.0, mask=z(2, 32, dtype=torch.uint8))
    with pytest.raises(ValueError, match="by must be"):
        ops.grouped_match_explain(z(32, 8), z(32, 8), z(1, 8), z(1, 8), None, off, 32, 1.0, by='gradient')
