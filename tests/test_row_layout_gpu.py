"""The layout contract of the HBM-bound row kernels on the MI355X: every entry of tests/row_layout_cases.py at every body its host
dispatch can pick (16-byte, scalar by width, scalar by each leading dimension and each base pointer alone), at the first size whose
grid-stride loop makes a second sweep, and at its refusals -- against the fp64 / exact host statement of the operation, never against
a result read back from the GPU.  tests/test_row_layout_cpu.py proves that the table reaches what this docstring says it does.

Every case places the same logical operands at several layouts (C contiguous, V ld = cols + 4, S ld = cols + 1, O ld = cols + 4 at an
offset of one float, W ld = cols rounded up to 4; inputs and outputs independently where the dispatch looks at them independently)
inside buffers whose every other word is the sentinel 0x5A5AA5A5, and asserts per layout

1. the value: bitwise where the kernel moves or combines elements without a reduction, otherwise the bound of the operation's own test
   (1e-6 mean_pool, 5e-5 forward, 2e-4 backward against fp64) -- no bound of this file's own;
2. placement independence: the layouts of one case are torch.equal wherever the bodies sum in the same order (all the bitwise entries;
   mean_pool's flat and scalar bodies, which both add the rows in order, and the counted against the uncounted form); the row groups of
   mean_pool_vec4_kernel and the 16-lane rows of layernorm_bwd_vec_kernel associate differently from their scalar bodies and are held
   to fp64 only.  mean_pool's and news_xin's inputs are multiples of 1 / 64, so that every partial sum is exact in any order and
   1e-6 holds at S = 300 for either association: what is left is the rounding of 1 / S and of the product with it;
3. nothing outside the view is written: every word of every output buffer outside the view still holds the sentinel, and every input
   buffer comes back bit-identical;
4. refusals hold and touch nothing: the call raises (or the C entry returns LIME_ERR_UNSUPPORTED) and every buffer is bit for bit
   what it was.

fuse_rows with a gate: hipcc does not contract g * x + (1 - g) * y (a packed multiplication and an addition), so the comparison is
bitwise against the same expression in fp32 on the host.

Worst figures observed on the MI355X (each comparison prints its figure on a line that starts with 'PIN'; the whole file runs in
about 5 s; no case needed a bound of its own):

  kernel branch                                   reached by                                                  worst error (bound)
  embed_pe_kernel<4>                              1312 x 300, period 32, C / V, with and without pe           bitwise
  embed_pe_scalar_kernel by width                 dim 50 at ld 50 / 52 / 51                                   bitwise
  embed_pe_scalar_kernel by one operand alone     ld_table / ld_pe / ldo 301; table / pe / out off 1          bitwise
  embed_pe second sweep, <4> / scalar             28,000 x 300 / 7,100 x 301                                  bitwise
  mean_pool_flat_kernel (+ counted)               n_seq 700, S 1 / 3 / 16; live 0 / 333 / 700 / 900; n 37 live 20   7.9e-8 (1e-6), rows behind the count untouched
  mean_pool_vec4_kernel                           dim 4 / 300 / 1024, S 1 / 3 / 32 / 300, n_seq 3 / 37        8.1e-8 (1e-6)
  mean_pool_kernel                                dim 50 (ld 50, 52), dim 1028, ldx + 1, x off 1              8.1e-8 (1e-6), equal to the flat body's bits
  mean_pool counted: refusals                     S 17; ldx 301; x off 1; dim 50                              raises, nothing written
  news_xin_kernel                                 cap 9, dim 300, nblk 1 / 4 / 16, live 0 / 5 / 9 / 12, xin ld 400   bitwise (one block row), 0 (1e-6)
  news_xin: refusals                              each ld + 1, each base off 1, dim 50                        raises, nothing written
  fuse_rows_kernel add / gated                    (37, 300), (33, 33); each of lda, ldb, ldg, ldo + 1; off 1  bitwise; gated 1.2e-7 against fp64 (5e-5)
  fuse_rows second sweep                          (1800, 300) at ld 301                                       bitwise
  gather_rows_kernel (+ second sweep)             700 from 50 x 300 (rows 0, 49, repeats); (1800, 300)        bitwise
  row_scale_kernel (+ second sweep)               (700, 300) aligned and off 1; (1800, 300)                   bitwise
  pad_heads_kernel (+ second sweep)               6 x 20 -> 32 x 300; vector form 60 x 20 -> 32; 60 x 32 x 300     bitwise
  fill_pad_rows_kernel                            (296, 300), S 8: C, V, dst = columns [300, 600) of 900      bitwise
  fill_pad_rows: refusals                         lds / ldd 301, src / dst off 1, cols 50                     raises, nothing written
  relu_bwd_kernel (+ second sweep)                (296, 300) in place, scale 1 / 0.37, lddh / ldh 301; (7100, 300) bitwise
  gate_mul_kernel sigmoid / div 1 / div 4 + scale (130, 96), (8, 4); n_rows_dev none / 0 / half / beyond      1.4e-7 (5e-5) / bitwise / bitwise
  gate_mul: refusals                              x, g, out strided; x, g, out off 1                          raises, nothing written
  gather_rows_multi word / word + tail / byte     17 pairs (two launches), 130 rows: row bytes 50, 28, 24, 3, 1, 4 .. 36  bitwise, plan reused
  colsum, reduce_partials_vec4_kernel             N 300, M 1 / 255 / 257 / 70,000, x C / V / S / O, accumulate      8.6e-7 (5e-5)
  colsum, reduce_partials_kernel                  N 7 / 301; N 300 with out off 1                             1.1e-6 (5e-5)
  layernorm_bwd_vec_kernel<2 / 5 / 8>             E 100 / 300 / 400, 512, M 96, dy_div 1 / 16, C and ld E + 4       dz 2.1e-7, dgamma 3.9e-7, dbeta 2.5e-7, dzsum 4.4e-7 (2e-4)
  its second persistent sweep                     M 12309, E 100, dy_div 16                                   dz 2.2e-7, dgamma 6.2e-7, dzsum 4.2e-7 (2e-4)
  layernorm_bwd_kernel<2 / 5 / 8> by width        E 50 / 301 / 450 (ld E and E rounded up to 4)               dz 2.6e-7, dgamma 4.1e-7, dzsum 4.6e-7 (2e-4)
  layernorm_bwd_kernel<5> by one operand alone    E 300: lddy / ldy / lddz 301; dy / y / dz / gamma / beta off 1    dz 2.2e-7 (2e-4)
  layernorm_bwd: refusal                          E 516                                                       LIME_ERR_UNSUPPORTED, nothing written
  nll_softmax_kernel                              (37, 5), logits and dlogits C / V / S / O                   loss 5.0e-9, dlogits 1.5e-7 (5e-5)
  additive_pool_kernel                            (11, 32, 400, 200), ldh / ldx / ldo alone and together      7.3e-7 (5e-5)
  additive_pool_bwd_kernel                        (5, 100, 64, 50), each of five lds alone and together       d hidden 1.0e-6, d x 6.1e-7, d affine2 4.2e-7 (2e-4)
  intent_fuse_kernel (+ counted)                  (5, 2, 64, 48), content C / V / S / O / columns [100, 228) of 237   3.0e-7 (5e-5), rows behind the count untouched
  intent_fuse_bwd_kernel                          the same, dcontent                                          d intents 1.6e-7, d hidden 3.9e-7, d affine2 5.8e-7 (2e-4)
  embed_bwd sorted (+ pass H) / small             9000 (22,000) rows into 500 x 300; 1760 into 10 x 500; dx, dtable strided   7.2e-6 / 5.2e-6 / 1.6e-6 (2e-4)
  embed_bwd_kernel<5 / 8> (float atomics)         9000 x 300 with the sorted back end off; 1760 x 400         1.1e-5 / 4.8e-6 (2e-4)

Within one case and one body every layout gives the same bits (asserted), the atomic back end of embed_bwd excepted."""
import ctypes
import types

import pytest
import torch

import row_layout_cases as rc
from helpers import rel_err

pytestmark = pytest.mark.gpu

TIGHT, BWD, POOL = rc.TIGHT, rc.BWD, rc.POOL
LIME_ERR_UNSUPPORTED = -2
WORST = {}


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from lime_cikm25_amd import ops as _ops
    from lime_cikm25_amd import _lib
    _lib.load()
    assert _lib.MAX_GATHERS == rc.MAX_GATHERS
    yield _ops
    for k in sorted(WORST):
        print('WORST %-44s %s' % (k, 'bitwise' if WORST[k] is None else '%.1e' % WORST[k]))


def _lib_and_error():
    from lime_cikm25_amd import _lib
    return _lib.load(), _lib.LimeHipError


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def note(branch, err):
    if err is None:
        WORST.setdefault(branch, None)
    else:
        WORST[branch] = max(WORST.get(branch) or 0.0, err)


def close(got, want, tol, what, branch):
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape), (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what
    e = rel_err(got.numpy(), want.detach().numpy())
    print('PIN %s [%s]: rel err %.3e (bound %.1e)' % (what, branch, e, tol))
    note(branch, e)
    assert e <= tol, '%s: rel err %.3e > %.1e' % (what, e, tol)


def bitwise(got, want, what, branch):
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = int((got != want).sum())
    print('PIN %s [%s]: bitwise, %d of %d elements differ' % (what, branch, bad, got.numel()))
    note(branch, None)
    assert bad == 0, '%s: %d of %d elements differ from the host statement' % (what, bad, got.numel())


class Lay:
    """The operands of one call at one layout: inputs and outputs in guarded buffers, with what they held before the call."""

    def __init__(self, lds, offs):
        self.lds, self.offs, self.ins, self.outs = lds, offs, [], []

    def _place(self, name, t):
        cols = t[1] if isinstance(t, tuple) else t.shape[1]
        return rc.placed(t, self.lds.get(name, cols), self.offs.get(name, 0))

    def inp(self, name, t):
        v, buf = self._place(name, t)
        self.ins.append((name, buf, buf.clone()))
        return v

    def out(self, name, shape=None, init=None):
        """An output of ``shape`` that starts as the sentinel, or one that starts as ``init`` (in place, accumulate)."""
        v, buf = self._place(name, tuple(shape) if init is None else init)
        self.outs.append((name, buf, buf.clone(), v))
        return v

    def vec(self, name, n=None, init=None, output=False):
        """A contiguous vector, optionally ``offs[name]`` floats off the aligned base."""
        t = init.view(1, -1) if init is not None else None
        v = self.out(name, (1, n), t) if output else self.inp(name, t)
        return v[0]

    def check(self):
        for name, buf, before in self.ins:
            assert torch.equal(buf, before), 'input %s was written' % name
        for name, buf, before, v in self.outs:
            assert rc.outside_untouched(buf, v), 'wrote outside %s' % name

    def all_untouched(self):
        for name, buf, before in self.ins:
            assert torch.equal(buf, before), 'input %s was written by a refused call' % name
        for name, buf, before, v in self.outs:
            assert torch.equal(buf, before), '%s was written by a refused call' % name


def branch(case, lds, offs):
    body, sweep = rc.branch_of(case['entry'], case['dims'], lds, offs)
    return body, body + (' second sweep' if sweep else '')


def same_across(results, what):
    """results: [(layout name, order key, tensor)]: equal within an order key."""
    first = {}
    for name, key, t in results:
        if key in first:
            assert torch.equal(t, first[key][1]), '%s: layout %s differs from layout %s' % (what, name, first[key][0])
        else:
            first[key] = (name, t)


def par(entry):
    return pytest.mark.parametrize('case', rc.cases_of(entry), ids=rc.ids_of(entry))


# ---------------------------------------------------------------------------------------------------------------------
# embed_pe
# ---------------------------------------------------------------------------------------------------------------------
@par('embed_pe')
def test_embed_pe(ops, case):
    d = case['dims']
    rows, dim, period = d['rows'], d['dim'], d['period']
    ids = rc.ints(rows, d['V'], seed=11)
    table = rc.mag(d['V'], dim, seed=12)
    pe = rc.mag(period, dim, seed=13) * 0.1 if d['pe'] else None
    want = rc.embed_pe_ref(table, ids, pe, period)
    ids_d = ids.cuda()
    for name, lds, offs in case['layouts']:
        L = Lay(lds, offs)
        tv, pv, ov = L.inp('table', table), (L.inp('pe', pe) if pe is not None else None), L.out('out', (rows, dim))
        ops.embed_pe(ids_d, tv, pv, period, out=ov)
        bitwise(ov, want, 'embed_pe %s/%s' % (case['id'], name), branch(case, lds, offs)[1])
        L.check()


# ---------------------------------------------------------------------------------------------------------------------
# mean_pool and its counted form
# ---------------------------------------------------------------------------------------------------------------------
@par('mean_pool')
def test_mean_pool(ops, case):
    _, LimeHipError = _lib_and_error()
    d = case['dims']
    n_seq, S, dim, live = d['n_seq'], d['S'], d['dim'], d['live']
    x = rc.grid64(n_seq * S, dim, seed=S + dim)
    want = rc.mean_pool_ref(x, n_seq, S)
    count = None if live is None else torch.tensor([live], dtype=torch.int32, device='cuda')
    k = n_seq if live is None else min(live, n_seq)
    results = []
    for name, lds, offs in case['layouts']:
        body, br = branch(case, lds, offs)
        L = Lay(lds, offs)
        xv, ov = L.inp('x', x), L.out('out', (n_seq, dim))
        what = 'mean_pool %s/%s' % (case['id'], name)
        if body == 'refused':
            with pytest.raises(LimeHipError):
                ops.mean_pool(xv, n_seq, S, out=ov, n_seq_dev=count)
            torch.cuda.synchronize()
            L.all_untouched()
            note('mean_pool refused', None)
            continue
        ops.mean_pool(xv, n_seq, S, out=ov, n_seq_dev=count)
        close(ov[:k], want[:k], POOL, what, br + (' counted' if live is not None else ''))
        assert rc.is_sentinel(ov[k:]), what + ': wrote behind the count'
        L.check()
        results.append((name, 'rows in order' if body != 'mean_pool_vec4_kernel' else 'row groups', ov[:k].clone()))
    if results:
        same_across(results, 'mean_pool ' + case['id'])
    if live is not None and results:                       # the counted rows are the uncounted form's rows
        full = ops.mean_pool(x.cuda(), n_seq, S)
        assert torch.equal(results[0][2], full[:k])


# ---------------------------------------------------------------------------------------------------------------------
# news_xin
# ---------------------------------------------------------------------------------------------------------------------
@par('news_xin')
def test_news_xin(ops, case):
    _, LimeHipError = _lib_and_error()
    d = case['dims']
    cap, dim, nt, nb, live = d['cap'], d['dim'], d['nblk_t'], d['nblk_b'], d['live']
    tb, bb = rc.grid64(cap * nt, dim, seed=21), rc.grid64(cap * nb, dim, seed=22)
    title_row, body_row = rc.ints(cap, cap, seed=23), rc.ints(cap, cap, seed=24)
    want = rc.news_xin_ref(tb, nt, bb, nb, title_row, body_row, cap)
    news = types.SimpleNamespace(n=cap - 1, title_row=title_row.cuda(), body_row=body_row.cuda(),
                                 n_news=torch.tensor([live], dtype=torch.int32, device='cuda'))
    k = min(live, cap)
    results = []
    for name, lds, offs in case['layouts']:
        body, br = branch(case, lds, offs)
        L = Lay(lds, offs)
        tv, bv, xv = L.inp('title_blocks', tb), L.inp('body_blocks', bb), L.out('xin', (2 * cap, dim))
        what = 'news_xin %s/%s' % (case['id'], name)
        if body == 'refused':
            with pytest.raises(LimeHipError):
                ops.news_xin(tv, nt, bv, nb, news, xv, dim)
            torch.cuda.synchronize()
            L.all_untouched()
            note('news_xin refused', None)
            continue
        ops.news_xin(tv, nt, bv, nb, news, xv, dim)
        for half, nblk in ((0, nt), (1, nb)):
            got, ref = xv[half * cap:half * cap + k], want[half * cap:half * cap + k]
            if nblk == 1:
                bitwise(got, ref.float(), what + ' half %d' % half, 'news_xin_kernel one block row')
            else:
                close(got, ref, POOL, what + ' half %d' % half, 'news_xin_kernel %d block rows' % nblk)
            assert rc.is_sentinel(xv[half * cap + k:(half + 1) * cap]), what + ': wrote a row at or beyond the count'
        L.check()
        results.append((name, 'one order', xv[:k].clone()))
    same_across(results, 'news_xin ' + case['id'])


# ---------------------------------------------------------------------------------------------------------------------
# fuse_rows, gather_rows, row_scale, pad_heads, fill_pad_rows, relu_bwd_
# ---------------------------------------------------------------------------------------------------------------------
@par('fuse_rows')
def test_fuse_rows(ops, case):
    d = case['dims']
    rows, cols = d['rows'], d['cols']
    a, b = rc.mag(rows, cols, seed=31), rc.mag(rows, cols, seed=32)
    gate = torch.rand(rows, cols, generator=torch.Generator().manual_seed(33)) if d['gated'] else None
    want = rc.fuse_rows_gated_f32(a, b, gate) if d['gated'] else rc.fuse_rows_ref(a, b)
    for name, lds, offs in case['layouts']:
        L = Lay(lds, offs)
        av, bv, gv, ov = L.inp('a', a), L.inp('b', b), (L.inp('gate', gate) if d['gated'] else None), L.out('out', (rows, cols))
        ops.fuse_rows(av, bv, gv, out=ov)
        what, br = 'fuse_rows %s/%s' % (case['id'], name), branch(case, lds, offs)[1] + (' gated' if d['gated'] else ' add')
        bitwise(ov, want, what, br)
        if d['gated']:
            close(ov, rc.fuse_rows_ref(a, b, gate), TIGHT, what + ' against fp64', br + ' (fp64)')
        L.check()


@par('gather_rows')
def test_gather_rows(ops, case):
    d = case['dims']
    rows, cols, n = d['rows'], d['cols'], d['n']
    idx, table = rc.ints(rows, n, seed=41), rc.mag(n, cols, seed=42)
    assert idx.unique().numel() < rows and int(idx.min()) == 0 and int(idx.max()) == n - 1
    want = rc.gather_ref(table, idx)
    for name, lds, offs in case['layouts']:
        L = Lay(lds, offs)
        tv, ov = L.inp('table', table), L.out('out', (rows, cols))
        ops.gather_rows(idx.cuda(), tv, ov)
        bitwise(ov, want, 'gather_rows %s/%s' % (case['id'], name), branch(case, lds, offs)[1])
        L.check()


@par('row_scale')
def test_row_scale(ops, case):
    d = case['dims']
    rows, cols = d['rows'], d['cols']
    x, scale = rc.mag(rows, cols, seed=51), rc.mag(rows, seed=52)
    want = rc.row_scale_ref(x, scale)
    for name, lds, offs in case['layouts']:
        L = Lay(lds, offs)
        xv = L.inp('x', x)
        assert xv.is_contiguous()
        got = ops.row_scale(xv, scale.cuda())
        bitwise(got, want, 'row_scale %s/%s' % (case['id'], name), branch(case, lds, offs)[1])
        L.check()


@par('pad_heads')
def test_pad_heads(ops, case):
    lib, _ = _lib_and_error()
    d = case['dims']
    n_blk, hd, hs, cols = d['n_blk'], d['hd'], d['hs'], d['cols']
    src = rc.mag(n_blk * hd, cols, seed=61)
    want = rc.pad_heads_ref(src, n_blk, hd, hs)
    for name, lds, offs in case['layouts']:
        L = Lay(lds, offs)
        sv, dv = L.inp('src', src), L.out('dst', (n_blk * hs, cols))
        assert lib.lime_pad_heads_f32(ptr(sv), sv.stride(0), ptr(dv), dv.stride(0), n_blk, hd, hs, cols, stream()) == 0
        what, br = 'pad_heads %s/%s' % (case['id'], name), branch(case, lds, offs)[1]
        bitwise(dv, want, what, br)
        L.check()
        got = ops.pad_heads(sv.view(-1) if cols == 1 and sv.is_contiguous() else sv, n_blk, hd, hs)     # the wrapper's own dst
        bitwise(got.view(-1, cols), want, what + ' (ops)', br)
        L.check()


@par('fill_pad_rows')
def test_fill_pad_rows(ops, case):
    _, LimeHipError = _lib_and_error()
    d = case['dims']
    rows, cols, S = d['rows'], d['cols'], d['S']
    ids = rc.ints(rows, 3, seed=71, ends=False)
    assert 0 < int((ids == 0).sum()) < rows
    src, dst = rc.mag(S, cols, seed=72), rc.mag(rows, cols, seed=73)
    want = rc.fill_pad_rows_ref(ids, src, dst, S)
    for name, lds, offs in case['layouts']:
        body, br = branch(case, lds, offs)
        L = Lay(lds, offs)
        sv, dv = L.inp('src', src), L.out('dst', init=dst)
        if body == 'refused':
            with pytest.raises(LimeHipError):
                ops.fill_pad_rows(ids.cuda(), sv, dv, S)
            torch.cuda.synchronize()
            L.all_untouched()
            note('fill_pad_rows refused', None)
            continue
        ops.fill_pad_rows(ids.cuda(), sv, dv, S)
        bitwise(dv, want, 'fill_pad_rows %s/%s' % (case['id'], name), br)
        L.check()


@par('relu_bwd_')
def test_relu_bwd(ops, case):
    d = case['dims']
    rows, cols, scale = d['rows'], d['cols'], d['scale']
    dh, h = rc.mag(rows, cols, seed=81), rc.rnd(rows, cols, seed=82)
    h[0, :7] = 0.0                                                             # h == 0 is not h > 0
    want = rc.relu_bwd_ref(dh, h, scale)
    for name, lds, offs in case['layouts']:
        L = Lay(lds, offs)
        gv, hv = L.out('dh', init=dh), L.inp('h', h)
        assert ops.relu_bwd_(gv, hv, scale) is gv                              # in place, as training.py calls it
        bitwise(gv, want, 'relu_bwd_ %s/%s' % (case['id'], name), branch(case, lds, offs)[1])
        L.check()


# ---------------------------------------------------------------------------------------------------------------------
# gate_mul
# ---------------------------------------------------------------------------------------------------------------------
@par('gate_mul')
def test_gate_mul(ops, case):
    _, LimeHipError = _lib_and_error()
    d = case['dims']
    rows, cols, sig, div, scale, live = d['rows'], d['cols'], d['sigmoid'], d['div'], d['scale'], d['live']
    x = rc.mag(rows, cols, seed=91)
    g = rc.rnd(rows, cols, seed=92, scale=4.0) if sig else rc.mag((rows + div - 1) // div, cols, seed=93)
    want = rc.gate_mul_ref(x, g, div, scale, sig)
    count = None if live is None else torch.tensor([live], dtype=torch.int32, device='cuda')
    k = rows if live is None else min(live, rows)
    for name, lds, offs in case['layouts']:
        body, br = branch(case, lds, offs)
        L = Lay(lds, offs)
        xv, gv, ov = L.inp('x', x), L.inp('g', g), L.out('out', (rows, cols))
        what = 'gate_mul %s/%s' % (case['id'], name)
        if body == 'refused':
            with pytest.raises((ValueError, LimeHipError)):
                ops.gate_mul(xv, gv, div, scale, sig, out=ov, n_rows_dev=count)
            torch.cuda.synchronize()
            L.all_untouched()
            note('gate_mul refused', None)
            continue
        ops.gate_mul(xv, gv, div, scale, sig, out=ov, n_rows_dev=count)
        if sig:
            close(ov[:k], want[:k], TIGHT, what, br)
        else:
            bitwise(ov[:k], want[:k], what, br + ' div %d' % div)
        assert rc.is_sentinel(ov[k:]), what + ': wrote behind the count'
        L.check()


# ---------------------------------------------------------------------------------------------------------------------
# gather_rows_multi
# ---------------------------------------------------------------------------------------------------------------------
def _multi_operands(idx_len):
    """17 (table, out) pairs of rc.GATHER_MULTI_PAIRS; every out is rows [8, 8 + n) of a guard tensor filled with 0x5A bytes."""
    g = torch.Generator().manual_seed(7)
    tables, guards = [], []
    for dt, tail in rc.GATHER_MULTI_PAIRS:
        dtype = getattr(torch, dt)
        shape = (rc.GATHER_MULTI_TABLE,) + tuple(tail)
        t = rc.mag(*shape, seed=len(tables)) if dtype.is_floating_point else torch.randint(0, 100, shape, generator=g).to(dtype)
        tables.append(t.cuda())
        guard = torch.full((idx_len + 16,) + tuple(tail), 0x5A, dtype=torch.uint8, device='cuda').repeat_interleave(dtype.itemsize, dim=-1)
        guards.append(guard.view(dtype))
    return tables, guards


def test_gather_rows_multi(ops):
    from lime_cikm25_amd import _lib
    n = rc.GATHER_MULTI_ROWS
    idx = rc.ints(n, rc.GATHER_MULTI_TABLE, seed=5)                            # the rows rc.branch_of saw: repeats, 0 and 39
    tables, guards = _multi_operands(n)
    assert len(tables) == _lib.MAX_GATHERS + 1
    outs = [gd[8:8 + n] for gd in guards]
    before = [gd.clone() for gd in guards]
    plan = ops.gather_rows_multi_prepare(n, list(zip(tables, outs)))
    assert len(plan['tables']) == 2                                            # two launches
    for which, ix in (('first idx', idx), ('the plan again, second idx', idx.flip(0).contiguous())):
        ops.gather_rows_multi_run(ix.cuda(), plan)
        for (dt, tail), t, o, gd, b4 in zip(rc.GATHER_MULTI_PAIRS, tables, outs, guards, before):
            rb = t[0].numel() * t.element_size()
            body = rc.branch_of('gather_rows_multi', dict(row_bytes=rb, idx=ix.tolist()), {}, {})[0]
            bitwise(o, t.cpu()[ix.long()], 'gather_rows_multi %s %s row bytes %d, %s' % (dt, tail, rb, which), 'gather_rows_multi ' + body)
            assert torch.equal(gd[:8], b4[:8]) and torch.equal(gd[8 + n:], b4[8 + n:]), 'wrote outside the output'
    for t, was in zip(tables, _multi_operands(n)[0]):
        assert torch.equal(t, was), 'a table was written'


def test_gather_rows_multi_refuses_strided_operands(ops):
    n = 12
    idx = rc.ints(n, 9, seed=5).cuda()
    wide, out = rc.mag(9, 12, seed=1).cuda(), torch.full((n, 8), -7.0, device='cuda')
    wide_out = torch.full((n, 12), -7.0, device='cuda')
    with pytest.raises(ValueError):
        ops.gather_rows_multi(idx, [(wide[:, :8], out)])
    with pytest.raises(ValueError):
        ops.gather_rows_multi(idx, [(wide[:, :8].contiguous(), wide_out[:, :8])])
    with pytest.raises(ValueError):                                            # a good pair in front of the bad one is not run either
        ops.gather_rows_multi(idx, [(wide[:, :8].contiguous(), out), (wide[:, :8], out)])
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((wide_out == -7.0).all())
    note('gather_rows_multi refused', None)


# ---------------------------------------------------------------------------------------------------------------------
# colsum
# ---------------------------------------------------------------------------------------------------------------------
@par('colsum')
def test_colsum(ops, case):
    d = case['dims']
    M, N, acc = d['M'], d['N'], d['accumulate']
    x = rc.rnd(M, N, seed=M + N)
    base = rc.rnd(N, seed=3) if acc else None
    want = rc.colsum_ref(x, base)
    results = []
    for name, lds, offs in case['layouts']:
        L = Lay(lds, offs)
        xv = L.inp('x', x)
        ov = L.vec('out', N, init=base, output=True)
        assert ops.colsum(xv, out=ov, accumulate=acc) is ov
        close(ov, want, TIGHT, 'colsum %s/%s' % (case['id'], name), branch(case, lds, offs)[1] + (' accumulate' if acc else ''))
        L.check()
        results.append((name, branch(case, lds, offs)[0], ov.clone()))
    same_across(results, 'colsum ' + case['id'])                               # where x lies does not change a bit


# ---------------------------------------------------------------------------------------------------------------------
# layernorm_bwd (no dropout)
# ---------------------------------------------------------------------------------------------------------------------
@par('layernorm_bwd')
def test_layernorm_bwd(ops, case):
    lib, _ = _lib_and_error()
    d = case['dims']
    M, E, div = d['M'], d['E'], d['div']
    z, gamma, beta, dy = rc.layernorm_bwd_inputs(M, E, div)
    y, rstd, dz, dg, db, dzsum = rc.layernorm_bwd_ref(z, gamma, beta, dy, div)
    y32, rstd_d = y.float(), rstd.float().cuda()
    ws_floats = max(1, lib.lime_layernorm_bwd_workspace(M, min(E, 512)))
    results = []
    for name, lds, offs in case['layouts']:
        body, br = branch(case, lds, offs)
        L = Lay(lds, offs)
        dyv, yv, dzv = L.inp('dy', dy), L.inp('y', y32), L.out('dz', (M, E))
        gv, bv = L.vec('gamma', init=gamma), L.vec('beta', init=beta)
        dgv, dbv, dsv = (L.vec(nm, E, output=True) for nm in ('dgamma', 'dbeta', 'dzsum'))
        ws = torch.full((ws_floats,), float('nan'), device='cuda')
        st = lib.lime_layernorm_bwd_f32(ptr(dyv), dyv.stride(0), div, 1.0 / div, ptr(yv), yv.stride(0), ptr(gv), ptr(bv), ptr(rstd_d), ptr(dzv),
                                        dzv.stride(0), M, E, ptr(dgv), ptr(dbv), ptr(dsv), 0, ptr(ws), ws.numel(), stream())
        what = 'layernorm_bwd %s/%s' % (case['id'], name)
        if body == 'refused':
            torch.cuda.synchronize()
            assert st == LIME_ERR_UNSUPPORTED
            L.all_untouched()
            with pytest.raises(Exception):
                ops.layernorm_bwd(dyv, yv, gv, bv, rstd_d, dy_div=div, dy_scale=1.0 / div)
            note('layernorm_bwd refused', None)
            continue
        assert st == 0, what
        close(dzv, dz, BWD, what + ' dz', br + ' dz')
        close(dgv, dg, BWD, what + ' dgamma', br + ' dgamma')
        close(dbv, db, BWD, what + ' dbeta', br + ' dbeta')
        close(dsv, dzsum, BWD, what + ' dzsum', br + ' dzsum')
        L.check()
        results.append((name, body, torch.cat([dzv.reshape(-1), dgv, dbv, dsv])))
        if 'dz' not in lds and 'gamma' not in offs and 'beta' not in offs:     # the wrapper (its own contiguous dz): the same launch
            got = ops.layernorm_bwd(dyv, yv, gv, bv, rstd_d, dy_div=div, dy_scale=1.0 / div)
            for a, b in zip(got, (dzv, dgv, dbv, dsv)):
                assert torch.equal(a, b), what + ': ops.layernorm_bwd differs from the C entry'
            L.check()
    same_across(results, 'layernorm_bwd ' + case['id'])                        # one body, any layout: the same bits


# ---------------------------------------------------------------------------------------------------------------------
# nll_softmax, additive_pool (+ backward), intent_fuse (+ backward), embed_bwd: one scalar body each, leading dimensions only
# ---------------------------------------------------------------------------------------------------------------------
@par('nll_softmax')
def test_nll_softmax(ops, case):
    lib, _ = _lib_and_error()
    B, K = case['dims']['B'], case['dims']['K']
    logits = rc.rnd(B, K, seed=1, scale=4.0)
    want_loss, want_d = rc.nll_softmax_ref(logits)
    results = []
    for name, lds, offs in case['layouts']:
        L = Lay(lds, offs)
        lv, dv, loss = L.inp('logits', logits), L.out('dlogits', (B, K)), L.out('loss', (1, 1))
        assert lib.lime_nll_softmax_f32(ptr(lv), lv.stride(0), B, K, ptr(loss), ptr(dv), dv.stride(0), stream()) == 0
        what = 'nll_softmax %s/%s' % (case['id'], name)
        close(loss.view(1), want_loss, TIGHT, what + ' loss', 'nll_softmax_kernel loss')
        close(dv, want_d, TIGHT, what + ' dlogits', 'nll_softmax_kernel dlogits')
        L.check()
        results.append((name, 'one order', torch.cat([loss.view(1), dv.reshape(-1)])))
        if 'dlogits' not in lds or lds['dlogits'] == K and not offs['dlogits']:       # the wrapper (its own dlogits)
            got_loss, got_d = ops.nll_softmax(lv)
            assert torch.equal(got_loss, loss.view(1)) and torch.equal(got_d, dv)
            L.check()
    same_across(results, 'nll_softmax ' + case['id'])


def _pool_mask(n_seq, S):
    g = torch.Generator().manual_seed(4)
    mask = (torch.rand(n_seq, S, generator=g) > 0.3).to(torch.uint8)
    mask[:, 0] = 1
    mask[n_seq // 2] = 0                                                       # a sequence with every token masked
    return mask


@par('additive_pool')
def test_additive_pool(ops, case):
    d = case['dims']
    n_seq, S, A, D = d['n_seq'], d['S'], d['A'], d['D']
    hidden, x, a2 = torch.tanh(rc.rnd(n_seq * S, A, seed=1, scale=2)), rc.rnd(n_seq * S, D, seed=2), rc.rnd(A, seed=3, scale=0.3)
    mask = _pool_mask(n_seq, S)
    want = rc.additive_pool_ref(hidden, a2, x, mask, n_seq, S)
    results = []
    for name, lds, offs in case['layouts']:
        L = Lay(lds, offs)
        hv, xv, ov = L.inp('hidden', hidden), L.inp('x', x), L.out('out', (n_seq, D))
        ops.additive_pool(hv, a2.cuda(), xv, n_seq, S, mask=mask.cuda(), out=ov)
        close(ov, want, TIGHT, 'additive_pool %s/%s' % (case['id'], name), 'additive_pool_kernel')
        L.check()
        results.append((name, 'one order', ov.clone()))
    same_across(results, 'additive_pool ' + case['id'])


@par('additive_pool_bwd')
def test_additive_pool_bwd(ops, case):
    lib, _ = _lib_and_error()
    d = case['dims']
    n_seq, S, A, D = d['n_seq'], d['S'], d['A'], d['D']
    hidden, a2, x, dout = rc.rnd(n_seq * S, A, seed=1), rc.rnd(A, seed=2), rc.rnd(n_seq * S, D, seed=3), rc.rnd(n_seq, D, seed=5)
    mask = _pool_mask(n_seq, S)
    _, want_dh, want_da2, want_dx = rc.additive_pool_ref(hidden, a2, x, mask, n_seq, S, dout)
    a2_d, mask_d = a2.cuda(), mask.cuda()
    results = []
    for name, lds, offs in case['layouts']:
        L = Lay(lds, offs)
        hv, xv, dv = L.inp('hidden', hidden), L.inp('x', x), L.inp('dout', dout)
        dh, dx, part = L.out('dhidden', (n_seq * S, A)), L.out('dx', (n_seq * S, D)), L.out('part', (n_seq, A))
        st = lib.lime_additive_pool_bwd_f32(ptr(hv), hv.stride(0), ptr(a2_d), A, ptr(xv), xv.stride(0), D, ptr(mask_d), ptr(dv), dv.stride(0),
                                            ptr(dh), dh.stride(0), ptr(dx), dx.stride(0), ptr(part), n_seq, S, stream())
        assert st == 0
        what = 'additive_pool_bwd %s/%s' % (case['id'], name)
        close(dh, want_dh, BWD, what + ' d hidden', 'additive_pool_bwd_kernel d hidden')
        close(dx, want_dx, BWD, what + ' d x', 'additive_pool_bwd_kernel d x')
        close(ops.colsum(part), want_da2, BWD, what + ' d affine2', 'additive_pool_bwd_kernel d affine2')
        assert bool((dh.cpu().view(n_seq, S, A)[mask == 0] == 0).all())          # a masked token's score is a constant
        L.check()
        results.append((name, 'one order', torch.cat([dh.reshape(-1), dx.reshape(-1), part.reshape(-1)])))
        if all(lds[n] == w and not offs[n] for n, w in (('dhidden', A), ('dx', D))):     # the wrapper (its own dhidden, dx)
            g_dh, g_da2, g_dx = ops.additive_pool_bwd(hv, a2_d, xv, dv, n_seq, S, mask=mask_d)
            assert torch.equal(g_dh, dh) and torch.equal(g_dx, dx) and torch.equal(g_da2, ops.colsum(part))
            L.check()
    same_across(results, 'additive_pool_bwd ' + case['id'])


def _intent_operands(M, k, D, A):
    return (rc.rnd(2 * M * k, D, seed=1), torch.tanh(rc.rnd(2 * M * k, A, seed=2)), rc.rnd(A, seed=3, scale=0.2), rc.rnd(A, seed=4, scale=0.2))


@par('intent_fuse')
def test_intent_fuse(ops, case):
    d = case['dims']
    M, k, D, A, live = d['M'], d['k'], d['D'], d['A'], d['live']
    iv, hid, a2t, a2b = _intent_operands(M, k, D, A)
    want = rc.intent_fuse_ref(iv, hid, a2t, a2b, M, k)
    count = None if live is None else torch.tensor([live], dtype=torch.int32, device='cuda')
    n = M if live is None else min(live, M)
    ivd, hidd = iv.cuda(), hid.cuda()
    results = []
    for name, lds, offs in case['layouts']:
        L = Lay(lds, offs)
        cv = L.out('content', (M, 2 * D))
        ops.intent_fuse(ivd, hidd, a2t.cuda(), a2b.cuda(), cv, M, k, D, A, m_dev=count)
        what = 'intent_fuse %s/%s' % (case['id'], name)
        close(cv[:n], want[:n], TIGHT, what, 'intent_fuse_kernel' + (' counted' if live is not None else ''))
        assert rc.is_sentinel(cv[n:]), what + ': wrote a row at or beyond the count'
        L.check()
        results.append((name, 'one order', cv[:n].clone()))
    same_across(results, 'intent_fuse ' + case['id'])
    assert torch.equal(ivd.cpu(), iv) and torch.equal(hidd.cpu(), hid)


@par('intent_fuse_bwd')
def test_intent_fuse_bwd(ops, case):
    d = case['dims']
    M, k, D, A = d['M'], d['k'], d['D'], d['A']
    iv, hid, a2t, a2b = _intent_operands(M, k, D, A)
    dcontent = rc.rnd(M, 2 * D, seed=5)
    wants = rc.intent_fuse_ref(iv, hid, a2t, a2b, M, k, dcontent)[1:]
    results = []
    for name, lds, offs in case['layouts']:
        L = Lay(lds, offs)
        dv = L.inp('dcontent', dcontent)
        got = ops.intent_fuse_bwd(iv.cuda(), hid.cuda(), a2t.cuda(), a2b.cuda(), dv, M, k, D, A)
        for g, w, nm in zip(got, wants, ('d intents', 'd hidden', 'd affine2 title', 'd affine2 body')):
            close(g, w, BWD, 'intent_fuse_bwd %s/%s %s' % (case['id'], name, nm), 'intent_fuse_bwd_kernel ' + nm)
        L.check()
        results.append((name, 'one order', torch.cat([g.reshape(-1) for g in got])))
    same_across(results, 'intent_fuse_bwd ' + case['id'])


@par('embed_bwd')
def test_embed_bwd(ops, case):
    d = case['dims']
    rows, V, D = d['rows'], d['V'], d['D']
    ids = rc.embed_bwd_ids(rows, V, d['hot_share'])
    dx = rc.rnd(rows, D, seed=4)
    small = V <= 32
    base = rc.rnd(V, D, seed=7) if small else torch.zeros(V, D)                  # the small-table back end adds into what is there
    want = rc.embed_bwd_ref(ids, dx, V, base)
    body = None
    results = []
    ops.DETERMINISTIC_EMBED_BWD = d['deterministic']
    try:
        for name, lds, offs in case['layouts']:
            body = branch(case, lds, offs)[0]
            L = Lay(lds, offs)
            xv, tv = L.inp('dx', dx), L.out('dtable', init=base)
            assert ops.embed_bwd(ids.cuda(), xv, tv, hot_id=0) is tv
            close(tv, want, BWD, 'embed_bwd %s/%s' % (case['id'], name), body)
            L.check()
            results.append((name, 'fixed order', tv.clone()))
    finally:
        ops.DETERMINISTIC_EMBED_BWD = True
    if not body.startswith('embed_bwd_kernel'):                                 # float atomics: the order varies from run to run
        same_across(results, 'embed_bwd ' + case['id'])


# ---------------------------------------------------------------------------------------------------------------------
# one-row views: ops._ld() hands max(stride(0), cols) to the entry, right as long as no kernel looks for a row 1
# ---------------------------------------------------------------------------------------------------------------------
def test_one_row_views_with_any_row_stride(ops):
    cols = 300
    a, b = rc.mag(1, cols, seed=1), rc.mag(1, cols, seed=2)
    one = lambda t: (lambda v, buf: (v.as_strided((1, cols), (1, 1), v.storage_offset()), buf))(*rc.placed(t))   # stride(0) = 1 < cols
    (av, abuf), (bv, bbuf), (ov, obuf) = one(a), one(b), one((1, cols))
    assert av.stride(0) == 1 and ops._ld(av) == cols
    ops.fuse_rows(av, bv, out=ov)
    bitwise(ov, rc.fuse_rows_ref(a, b), 'fuse_rows one row', 'one-row views')
    assert rc.outside_untouched(obuf, ov)
    (ov, obuf) = one((1, cols))
    ops.mean_pool(av, 1, 1, out=ov)
    bitwise(ov, a, 'mean_pool one row of one token', 'one-row views')
    assert rc.outside_untouched(obuf, ov)
    (ov, obuf) = one((1, cols))
    ops.embed_pe(torch.zeros(1, dtype=torch.int32, device='cuda'), av, bv, 1, out=ov)
    bitwise(ov, rc.embed_pe_ref(a, torch.zeros(1, dtype=torch.int32), b, 1), 'embed_pe one row', 'one-row views')
    assert rc.outside_untouched(obuf, ov)
    got = ops.colsum(av)
    bitwise(got, a[0], 'colsum one row', 'one-row views')
    assert torch.equal(abuf.cpu(), rc.placed(a, device='cpu')[1]) and torch.equal(bbuf.cpu(), rc.placed(b, device='cpu')[1])
