"""lime_encoder_ffn_sp (csrc/ffn_sp_f32.hip) where its instruction stream reaches ahead of the tile it is working on: the layer-input
fragments of the next step -- and, behind a tile's last step, of the workgroup's NEXT tile -- are requested unconditionally with
branch-free offsets (a dead row or quad gets bit 31 of its buffer offset), and the residual rows of the epilogue the same way.  What
that can break and test_ffn_sp_gpu.py does not reach: a workgroup's second and third trip through the persistent loop, a next tile
that is partly or entirely dead (by M and by the device count), tiles shorter than a wave's share, quads beyond E, one pass and
eight.  Every launch writes into a sentinel-filled, wider buffer and is compared with the fp64 statement of test_ffn_sp_gpu.py.

pool32 runs wherever the row count allows it: the kernel's contract there is M % 32 == 0 and a device count that is a multiple of
32 (a wave's 32-token block is live or dead as a whole), so with pool32 the counts M - 3 and 128 cu - 5 become M - 32 and 128 cu - 32."""
import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu
TIGHT = 2e-5                                   # test_ffn_sp_gpu.py's bound for the split products
SENTINEL = 7.0
EPS = 1e-5


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available()
    from lime_cikm25_amd import ops as _ops
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


CASES = {       # name: (M or a function of the CU count, E, F)
    'second_trip': (lambda cu: 128 * (cu + 1) + 37, 300, 512),
    'third_trip': (lambda cu: 128 * (2 * cu + 1) + 64, 300, 512),
    'm1': (1, 300, 512),
    'm127': (127, 300, 512),
    'm129': (129, 300, 512),
    'm200': (200, 300, 512),
    'e64_one_pass': (288, 64, 128),
    'eight_passes': (288, 300, 1024),
}
_BUILT = {}


def case(ops, name):
    """Inputs, packed weights and the fp64 reference (rows and 32-row block means) of one case: computed once, shared, never
    written to."""
    if name in _BUILT:
        return _BUILT[name]
    M, E, F = CASES[name]
    M = M(ops.device_cus()) if callable(M) else M
    seed = 100 * sorted(CASES).index(name)
    c = dict(M=M, E=E, F=F)
    c['x'] = rnd(M, E, seed=seed + 1).cuda()
    w1 = rnd(F, E, seed=seed + 2, scale=E ** -0.5)
    c['b1'] = rnd(F, seed=seed + 3, scale=0.1).cuda()
    w2 = rnd(E, F, seed=seed + 4, scale=F ** -0.5)
    c['b2'] = rnd(E, seed=seed + 5, scale=0.1).cuda()
    c['g'] = (1 + rnd(E, seed=seed + 6, scale=0.2)).cuda()
    c['be'] = rnd(E, seed=seed + 7, scale=0.1).cuda()
    c['w1p'], c['w2p'] = ops.ffn_pack_sp(w1.cuda(), w2.cuda())
    d = lambda t: t.double().cpu()
    x = d(c['x'])
    h = torch.relu(x @ w1.double().T + d(c['b1']))
    c['rows'] = torch.nn.functional.layer_norm(x + h @ w2.double().T + d(c['b2']), (E,), d(c['g']), d(c['be']), EPS)
    c['means'] = c['rows'][:M // 32 * 32].reshape(-1, 32, E).mean(1)
    _BUILT[name] = c
    return c


def run(ops, c, pool32=False, m_dev=None, x=None):
    """The launch into a sentinel-filled buffer four columns wider than E; returns the whole buffer."""
    x = c['x'] if x is None else x
    M, E = x.shape[0], c['E']
    big = torch.full((M // 32 if pool32 else M, E + 4), SENTINEL, device='cuda')
    dev = None if m_dev is None else torch.tensor([m_dev], dtype=torch.int32, device='cuda')
    ops.encoder_ffn_sp(x, c['w1p'], c['w2p'], c['b1'], c['b2'], (c['g'], c['be']), EPS, pool32=pool32, m_dev=dev, out=big[:, :E])
    torch.cuda.synchronize()
    return big


def check(ops, name, pool32, counts):
    c = case(ops, name)
    M, E = c['M'], c['E']
    want = c['means'] if pool32 else c['rows']
    for m in counts:
        big = run(ops, c, pool32=pool32, m_dev=m).cpu()
        live = M if m is None else m
        rows = live // 32 if pool32 else live
        assert (big[:, E:] == SENTINEL).all(), (name, pool32, m)             # nothing written behind the E columns
        assert (big[rows:, :E] == SENTINEL).all(), (name, pool32, m)         # rows at or beyond the count untouched
        if rows:
            got = big[:rows, :E]
            assert torch.isfinite(got).all(), (name, pool32, m)
            e = rel_err(got, want[:rows])
            print('%s pool32=%s m_dev=%s: error %.3g' % (name, pool32, m, e))
            assert e < TIGHT, (name, pool32, m, e)


@pytest.mark.parametrize('name,pool32', [('second_trip', False), ('third_trip', False), ('third_trip', True)])
def test_later_trips_of_a_workgroup(ops, name, pool32):
    """The second and the third tile of a workgroup, the last one partly dead; then with device counts that cut three rows (a
    32-row block with pool32) off the end, that leave nothing, and that leave workgroup 0's second tile entirely dead.  (The
    second-trip M is no multiple of 32: no pool32 there.)"""
    c = case(ops, name)
    M, cu = c['M'], ops.device_cus()
    if pool32:
        check(ops, name, True, (None, M - 32, 0, 128 * cu - 32))
    else:
        check(ops, name, False, (None, M - 3, 0, 128 * cu - 5))


@pytest.mark.parametrize('name', ['m1', 'm127', 'm129', 'm200'])
def test_short_tiles(ops, name):
    """A tile shorter than a wave's share, and fetches that run past the only tile."""
    check(ops, name, False, (None,))


@pytest.mark.parametrize('pool32', [False, True])
@pytest.mark.parametrize('name', ['e64_one_pass', 'eight_passes'])
def test_other_widths(ops, name, pool32):
    """E = 64 with F = 128: quads beyond E, one pass.  E = 300 with F = 1024: eight passes."""
    M = case(ops, name)['M']
    check(ops, name, pool32, (None, M - 32, 0) if pool32 else (None, M - 3, 0))


def test_rows_do_not_depend_on_tile_or_launch(ops):
    """A 128-row block computed alone (M = 128) is bitwise what the same rows are at tile 1 and at tile n_cu (the second trip of
    workgroup 0) of a large launch, with and without a smaller device count."""
    c = case(ops, 'second_trip')
    cu, E = ops.device_cus(), c['E']
    whole = run(ops, c)[:, :E]
    fewer = run(ops, c, m_dev=128 * (cu + 1) + 5)[:, :E]
    for tile in (1, cu):
        r0 = 128 * tile
        alone = run(ops, c, x=c['x'][r0:r0 + 128])[:, :E]
        assert torch.equal(alone, whole[r0:r0 + 128]), tile
        assert torch.equal(alone, fewer[r0:r0 + 128]), tile


def test_bitwise_repeatable(ops):
    c = case(ops, 'third_trip')
    assert torch.equal(run(ops, c), run(ops, c))
    assert torch.equal(run(ops, c, pool32=True), run(ops, c, pool32=True))
