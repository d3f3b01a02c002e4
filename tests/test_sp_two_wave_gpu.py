"""lime_encoder_ffn_sp and lime_encoder_oproj_sp (csrc/ffn_sp_f32.hip, csrc/oproj_sp_f32.hip) at two waves per SIMD: eight waves per
128-token tile, wave w owns tokens 16 w .. 16 w + 15, and with pool32 a 32-token block is the pair of waves 2 b, 2 b + 1 -- the odd
wave hands its normalised values to the even one through the ring slot the tile's last step has just left, in two rounds.  What that
can break and the older suites do not reach: row counts that end on a 16-token boundary inside a tile (a dead wave beside a live
one), pairs of which some are dead, both parities of the staging slot on a workgroup's second tile (36 steps per tile at F = 512,
27 at F = 384, 9 at F = 128), and blocks whose bits must not depend on the pair or the tile that computes them.

Every launch writes into a sentinel-filled, wider buffer and is compared with an fp64 statement; bound: the project's split-product
bound of test_ffn_sp_gpu.py.  One input, one weight set and one fp64 reference per width, shared by every case (the small cases are
its leading rows) and never written to."""
import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu
TIGHT = 2e-5                                   # test_ffn_sp_gpu.py's bound for the split products
SENTINEL = 7.0
EPS = 1e-5
V = 500
PERIOD = 32


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available()
    from lime_cikm25_amd import ops as _ops
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


# ---------------------------------------------------------------------------------------------------------------- feed-forward
WIDTHS = {'e300_f512': (300, 512), 'e300_f384': (300, 384), 'e64_f128': (64, 128)}       # steps per tile: 36 (even), 27, 9 (odd)
_FFN = {}


def ffn_case(ops, width):
    """128 cu + 96 rows of input, packed weights and the fp64 rows / 32-row block means of one width."""
    if width in _FFN:
        return _FFN[width]
    E, F = WIDTHS[width]
    M = 128 * ops.device_cus() + 96
    seed = 1000 + 100 * sorted(WIDTHS).index(width)
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
    c['means'] = c['rows'].reshape(-1, 32, E).mean(1)
    _FFN[width] = c
    return c


def ffn_run(ops, c, x, pool32=False, m_dev=None):
    """The launch over the rows `x` into a sentinel-filled buffer four columns wider than E; returns the whole buffer."""
    M, E = x.shape[0], c['E']
    big = torch.full((M // 32 if pool32 else M, E + 4), SENTINEL, device='cuda')
    dev = None if m_dev is None else torch.tensor([m_dev], dtype=torch.int32, device='cuda')
    ops.encoder_ffn_sp(x, c['w1p'], c['w2p'], c['b1'], c['b2'], (c['g'], c['be']), EPS, pool32=pool32, m_dev=dev, out=big[:, :E])
    torch.cuda.synchronize()
    return big


def ffn_check(ops, width, M, pool32, counts):
    """The leading M rows of the width's input, once per device count."""
    c = ffn_case(ops, width)
    E = c['E']
    want = c['means'] if pool32 else c['rows']
    for m in counts:
        big = ffn_run(ops, c, c['x'][:M], pool32=pool32, m_dev=m).cpu()
        live = M if m is None else m
        rows = live // 32 if pool32 else live
        assert (big[:, E:] == SENTINEL).all(), (width, M, pool32, m)         # nothing written behind the E columns
        assert (big[rows:, :E] == SENTINEL).all(), (width, M, pool32, m)     # rows at or beyond the count untouched
        if rows:
            got = big[:rows, :E]
            assert torch.isfinite(got).all(), (width, M, pool32, m)
            e = rel_err(got, want[:rows])
            print('ffn %s M=%d pool32=%s m_dev=%s: error %.3g' % (width, M, pool32, m, e))
            assert e < TIGHT, (width, M, pool32, m, e)


FFN_ROWS = {'m8': 8, 'm16': 16, 'm24': 24, 'm40': 40, 'm136': 136}


@pytest.mark.parametrize('name', sorted(FFN_ROWS))
def test_ffn_rows_end_on_a_16_token_boundary(ops, name):
    """Half a wave, one wave, one and a half, two and a half, and a second tile of half a wave."""
    ffn_check(ops, 'e300_f512', FFN_ROWS[name], False, (None,))


FFN_CUTS = {'cut8': 152, 'cut24': 136}


@pytest.mark.parametrize('name', sorted(FFN_CUTS))
def test_ffn_device_count_cuts_rows_off_m160(ops, name):
    ffn_check(ops, 'e300_f512', 160, False, (FFN_CUTS[name],))


FFN_POOL_SMALL = {'m32': 32, 'm96': 96}


@pytest.mark.parametrize('name', sorted(FFN_POOL_SMALL))
def test_ffn_pool32_live_and_dead_pairs(ops, name):
    """One live pair beside three dead ones, three beside one; then the count one block lower, and nothing."""
    M = FFN_POOL_SMALL[name]
    ffn_check(ops, 'e300_f512', M, True, (None, M - 32, 0))


@pytest.mark.parametrize('width', sorted(WIDTHS))
def test_ffn_pool32_second_tile_both_slot_parities(ops, width):
    """M = 128 cu + 96: workgroup 0 runs a second tile, whose staging slot is the first tile's at F = 512 (an even number of steps
    per tile) and the other one at F = 384 and F = 128.  Then device counts that cut one block off, that leave the second tile's
    last live pair in the first round of tiles, and nothing."""
    c = ffn_case(ops, width)
    M, cu = c['M'], ops.device_cus()
    ffn_check(ops, width, M, True, (None, M - 32, 128 * cu - 32, 0))


def test_ffn_pool32_block_bits_do_not_depend_on_pair_or_tile(ops):
    """A 32-row block computed alone (M = 32, pair 0 of tile 0) is bitwise the same block at pair 0 and at pair 3 of tile 0 and at
    tile cu (workgroup 0's second tile) of the large launch; two runs of the large launch are bitwise equal."""
    c = ffn_case(ops, 'e300_f512')
    cu, E = ops.device_cus(), c['E']
    whole = ffn_run(ops, c, c['x'], pool32=True)
    assert torch.equal(whole, ffn_run(ops, c, c['x'], pool32=True))
    for r0 in (0, 96, 128 * cu, 128 * cu + 64):
        alone = ffn_run(ops, c, c['x'][r0:r0 + 32], pool32=True)
        assert torch.equal(alone[0, :E], whole[r0 // 32, :E]), r0


# -------------------------------------------------------------------------------------------------------------------- out_proj
OPROJ_ROWS = {'m8': 8, 'm24': 24, 'm136': 136, 'second_trip': lambda cu: 128 * cu + 40}
_OPROJ = {}


def oproj_case(ops):
    """128 cu + 40 rows of attention output, Wo, both residual forms and their fp64 references."""
    if _OPROJ:
        return _OPROJ
    E = 300
    M = 128 * ops.device_cus() + 40
    c = _OPROJ
    c.update(M=M, E=E)
    c['attn'] = rnd(M, E, seed=2001).cuda()
    w = rnd(E, E, seed=2002, scale=E ** -0.5)
    c['b'] = rnd(E, seed=2003, scale=0.1).cuda()
    c['g'] = (1 + rnd(E, seed=2004, scale=0.2)).cuda()
    c['be'] = rnd(E, seed=2005, scale=0.1).cuda()
    c['wp'] = ops.oproj_pack_sp(w.cuda())
    c['dense'] = rnd(M, E, seed=2006).cuda()
    c['table'], c['pe'] = rnd(V, E, seed=2007).cuda(), rnd(PERIOD, E, seed=2008, scale=0.5).cuda()
    c['ids'] = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(2009), dtype=torch.int32).cuda()
    d = lambda t: t.double().cpu()
    prod = d(c['attn']) @ w.double().T + d(c['b'])
    gathered = d(c['table'])[c['ids'].cpu().long()] + d(c['pe'])[torch.arange(M) % PERIOD]
    ln = lambda t: torch.nn.functional.layer_norm(t, (E,), d(c['g']), d(c['be']), EPS)
    c['want'] = {'dense': ln(d(c['dense']) + prod), 'gather': ln(gathered + prod)}
    return c


def oproj_run(ops, c, form, r0, M, m_dev=None):
    """The launch over rows r0 .. r0 + M (r0 a multiple of the period) into a sentinel-filled, wider buffer; returns the buffer."""
    E = c['E']
    assert r0 % PERIOD == 0
    big = torch.full((M, E + 4), SENTINEL, device='cuda')
    dev = None if m_dev is None else torch.tensor([m_dev], dtype=torch.int32, device='cuda')
    if form == 'dense':
        res = dict(res=c['dense'][r0:r0 + M])
    else:
        res = dict(res=c['table'], res_ids=c['ids'][r0:r0 + M].contiguous(), res_pe=c['pe'], res_period=PERIOD)
    ops.encoder_oproj_sp(c['attn'][r0:r0 + M], c['wp'], c['b'], (c['g'], c['be']), EPS, m_dev=dev, out=big[:, :E], **res)
    torch.cuda.synchronize()
    return big


@pytest.mark.parametrize('form', ['dense', 'gather'])
@pytest.mark.parametrize('name', sorted(OPROJ_ROWS))
def test_oproj_rows_end_on_a_16_token_boundary(ops, name, form):
    """res[row] and table[ids[row]] + pe[row % 32]; the whole count, eight rows fewer, and nothing."""
    c = oproj_case(ops)
    M, E = OPROJ_ROWS[name], c['E']
    M = M(ops.device_cus()) if callable(M) else M
    for m in (None, M - 8, 0):
        big = oproj_run(ops, c, form, 0, M, m_dev=m).cpu()
        rows = M if m is None else m
        assert (big[:, E:] == SENTINEL).all(), (name, form, m)
        assert (big[rows:, :E] == SENTINEL).all(), (name, form, m)
        if rows:
            got = big[:rows, :E]
            assert torch.isfinite(got).all(), (name, form, m)
            e = rel_err(got, c['want'][form][:rows])
            print('oproj %s %s m_dev=%s: error %.3g' % (name, form, m, e))
            assert e < TIGHT, (name, form, m, e)


@pytest.mark.parametrize('form', ['dense', 'gather'])
def test_oproj_rows_do_not_depend_on_tile_or_launch(ops, form):
    """A 128-row block computed alone is bitwise what the same rows are at tile 1 of the large launch, and the 40 rows of tile cu
    (workgroup 0's second trip) computed alone are what they are there, with and without a smaller device count."""
    c = oproj_case(ops)
    M, cu, E = c['M'], ops.device_cus(), c['E']
    whole = oproj_run(ops, c, form, 0, M)[:, :E]
    fewer = oproj_run(ops, c, form, 0, M, m_dev=M - 8)[:, :E]
    assert torch.equal(whole, oproj_run(ops, c, form, 0, M)[:, :E])
    alone = oproj_run(ops, c, form, 128, 128)[:, :E]
    assert torch.equal(alone, whole[128:256])
    assert torch.equal(alone, fewer[128:256])
    alone = oproj_run(ops, c, form, 128 * cu, 40)[:, :E]
    assert torch.equal(alone, whole[128 * cu:])
    assert torch.equal(alone[:32], fewer[128 * cu:128 * cu + 32])
