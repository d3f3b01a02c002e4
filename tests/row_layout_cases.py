"""The layout contract of the HBM-bound row kernels, stated on the host: the case table of tests/test_row_layout_gpu.py, a restatement
of every entry's host dispatch (which body a call takes, whether it reaches a second grid-stride sweep) and the fp64 / exact statement
of every operation.  Nothing here reads a result back from the GPU; tests/test_row_layout_cpu.py proves on the CPU that the table
selects every body and sweep it claims and violates every alignment condition of a vector body alone.

A case is one set of logical operands (``dims``, the same values for every layout) and a list of layouts: per operand a leading
dimension and an offset in floats from a 16-byte aligned base.  The four placements of an operand of ``cols`` columns are
``C`` contiguous and aligned, ``V`` ld = cols + 4 (vector body, strided), ``S`` ld = cols + 1 (scalar body by leading dimension) and
``O`` ld = cols + 4 at offset 1 (scalar body by base alignment); ``W`` is ld = cols rounded up to 4 (the width alone is odd)."""
import math

import torch

import dropout_cases as dc

SENTINEL = 0x5A5AA5A5           # as tests/test_workspace_contract_gpu.py: a finite float (1.5e16), compared as int32
TIGHT = 5e-5                    # test_backward_gpu.py: exact-fp32 kernels against fp64
BWD = 2e-4                      # test_backward_gpu.py: gradients against fp64 autograd
POOL = 1e-6                     # test_kernels_gpu.py::test_mean_pool_counted
MAX_GATHERS = 16                # LIME_MAX_GATHERS of include/lime_hip.h (asserted against the binding on the GPU)
LN_BLOCKS = 768                 # ln_blocks() of csrc/layernorm_bwd_f32.hip: persistent workgroups of 16 (vec) / 4 (scalar) rows a sweep


# ---------------------------------------------------------------------------------------------------------------------
# placements and guarded buffers
# ---------------------------------------------------------------------------------------------------------------------
def C(cols): return (cols, 0)
def V(cols): return (cols + 4, 0)
def S(cols): return (cols + 1, 0)
def O(cols): return (cols + 4, 1)
def W(cols): return ((cols + 3) // 4 * 4, 0)


def layout(cols, **kinds):
    """{'operand': placement function} -> (lds, offs), e.g. layout(300, table=V, out=S)."""
    lds, offs = {}, {}
    for name, kind in kinds.items():
        lds[name], offs[name] = kind(cols) if callable(kind) else kind
    return lds, offs


def placed(t, ld=None, off=0, fill=SENTINEL, device='cuda'):
    """t [rows, cols] (4-byte elements; None-valued: pass a shape tuple for an output that starts as the sentinel) in a 16-byte aligned
    buffer as as_strided((rows, cols), (ld, 1), off); every other word holds ``fill`` -> (view, int32 buffer)."""
    shape = tuple(t) if isinstance(t, (tuple, list)) else tuple(t.shape)
    dtype = torch.float32 if isinstance(t, (tuple, list)) else t.dtype
    rows, cols = shape
    ld = cols if ld is None else ld
    assert ld >= cols and dtype.itemsize == 4
    buf = torch.full((rows * ld + off + 8,), fill, dtype=torch.int32, device=device)
    assert buf.data_ptr() % 16 == 0
    v = buf.view(dtype).as_strided((rows, cols), (ld, 1), off)
    if not isinstance(t, (tuple, list)):
        v.copy_(t)
    return v, buf


def outside_untouched(buf, view, fill=SENTINEL):
    """Every word of ``buf`` that ``view`` does not cover still holds the sentinel (compared as int32)."""
    off = (view.data_ptr() - buf.data_ptr()) // 4
    covered = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    covered.as_strided(tuple(view.shape), tuple(view.stride()), off).fill_(True)
    return bool((buf[~covered] == fill).all())


def is_sentinel(view):
    return bool((view.contiguous().view(torch.int32) == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------
# the host dispatch of every entry, from the conditions in the .hip files
# ---------------------------------------------------------------------------------------------------------------------
# operands whose leading dimension AND base the vector condition looks at / whose base alone it looks at
_VEC_LD = {'embed_pe': ('table', 'pe', 'out'), 'mean_pool': ('x',), 'news_xin': ('title_blocks', 'body_blocks', 'xin'),
           'fill_pad_rows': ('src', 'dst'), 'layernorm_bwd': ('dy', 'y', 'dz'), 'colsum': (), 'gate_mul': ()}
_VEC_BASE = {'layernorm_bwd': ('gamma', 'beta'), 'colsum': ('out',), 'gate_mul': ('x', 'g', 'out')}
_WIDTH = {'embed_pe': 'dim', 'mean_pool': 'dim', 'news_xin': 'dim', 'fill_pad_rows': 'cols', 'layernorm_bwd': 'E', 'colsum': 'N',
          'gate_mul': 'cols'}


def violations(entry, dims, lds, offs):
    """The alignment conditions of ``entry``'s 16-byte body that the layout violates: 'width', 'ld:<operand>', 'off:<operand>'."""
    w = dims[_WIDTH[entry]]
    bad = set()
    if w % 4:
        bad.add('width')
    for name in _VEC_LD[entry]:
        if name == 'pe' and not dims.get('pe', True):
            continue
        if lds.get(name, w) % 4:
            bad.add('ld:' + name)
        if offs.get(name, 0) % 4:
            bad.add('off:' + name)
    for name in _VEC_BASE.get(entry, ()):
        if offs.get(name, 0) % 4:
            bad.add('off:' + name)
    return bad


def _blocks(total, per=256):
    return (total + per - 1) // per


def _cpl(E):
    c = (E + 63) // 64
    return 2 if c <= 2 else (5 if c <= 5 else 8)


def branch_of(entry, dims, lds, offs):
    """-> (name of the body the host picks, or 'refused'; whether some workgroup runs a second grid-stride sweep)."""
    if entry == 'embed_pe':
        vec = not violations(entry, dims, lds, offs)
        total = dims['rows'] * (dims['dim'] // 4 if vec else dims['dim'])
        return ('embed_pe_kernel<4>' if vec else 'embed_pe_scalar_kernel'), _blocks(total) > 8192
    if entry == 'mean_pool':
        vec = not violations(entry, dims, lds, offs) and dims['dim'] <= 1024
        counted = dims.get('live') is not None
        if counted and not (vec and dims['S'] <= 16):
            return 'refused', False
        if vec and dims['S'] <= 16 and (dims['n_seq'] >= 512 or counted):
            return 'mean_pool_flat_kernel', False
        return ('mean_pool_vec4_kernel' if vec else 'mean_pool_kernel'), False
    if entry == 'news_xin':
        ok = not violations(entry, dims, lds, offs) and 1 <= dims['nblk_t'] <= 16 and 1 <= dims['nblk_b'] <= 16
        return ('news_xin_kernel' if ok else 'refused'), False
    if entry == 'fill_pad_rows':
        if violations(entry, dims, lds, offs):
            return 'refused', False
        return 'fill_pad_rows_kernel', _blocks(dims['rows'] * (dims['cols'] // 4)) > 16384
    if entry in ('fuse_rows', 'gather_rows', 'row_scale'):
        return entry + '_kernel', _blocks(dims['rows'] * dims['cols']) > 2048
    if entry in ('nll_softmax', 'additive_pool', 'additive_pool_bwd', 'intent_fuse', 'intent_fuse_bwd'):
        return entry + '_kernel', False                   # one scalar body, leading dimensions only
    if entry == 'embed_bwd':                              # ops.embed_bwd's choice of back end
        if dims['V'] <= 32:
            return 'embed_bwd_small_kernel', False
        if dims['deterministic'] and dims['D'] <= 320:
            first = max(dims['hot_share'] * dims['rows'], 0)
            return 'embed_bwd_sorted' + (' + pass H' if first >= 8192 else ''), False
        return 'embed_bwd_kernel<%d>' % (5 if dims['D'] <= 320 else 8), False
    if entry == 'pad_heads':
        return 'pad_heads_kernel', _blocks(dims['n_blk'] * dims['hs'] * dims['cols']) > 2048
    if entry == 'relu_bwd_':
        return 'relu_bwd_kernel', _blocks(dims['rows'] * dims['cols']) > 8192
    if entry == 'gate_mul':
        cols = dims['cols']
        if any(lds.get(n, cols) != cols for n in ('x', 'g', 'out')) or violations(entry, dims, lds, offs):
            return 'refused', False                       # the wrapper wants contiguous operands, the entry 16-byte aligned ones
        return 'gate_mul_kernel:' + ('sigmoid' if dims['sigmoid'] else 'scale'), False
    if entry == 'gather_rows_multi':
        # per (pair, output row): words when source row and destination row are both 4-byte aligned (+ a byte tail when the row is no
        # whole number of words), bytes otherwise; contiguous tables, so row r starts r * row_bytes behind an aligned base
        bodies = set()
        rb = dims['row_bytes']
        for r, i in enumerate(dims['idx']):
            if (r * rb) % 4 == 0 and (i * rb) % 4 == 0:
                bodies.add('word' if rb % 4 == 0 else ('word+tail' if rb >= 4 else 'tail'))
            else:
                bodies.add('byte')
        return '/'.join(sorted(bodies)), dims.get('n_pairs', 1) > MAX_GATHERS      # "second sweep": a second launch
    if entry == 'colsum':
        nblk = min(256, max(1, _blocks(dims['M'])))
        vec = not violations(entry, dims, lds, offs)
        return ('reduce_partials_vec4_kernel' if vec else 'reduce_partials_kernel') + (':several' if nblk > 1 else ':one'), False
    if entry == 'layernorm_bwd':
        M, E = dims['M'], dims['E']
        if E > 512:
            return 'refused', False
        nblk = min(LN_BLOCKS, (M + 15) // 16)
        if not violations(entry, dims, lds, offs):
            return 'layernorm_bwd_vec_kernel<%d>' % _cpl(E), M > nblk * 16
        return 'layernorm_bwd_kernel<%d>' % _cpl(E), M > nblk * 4
    raise KeyError(entry)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def mag(*shape, seed=0):
    """|x| in [0.5, 1.5], random sign: never zero, one multiplication never denormal."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) + 0.5) * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def grid64(*shape, seed=0):
    """Multiples of 1 / 64 in [-1, 1]: every partial sum of up to 2^17 of them is exact in fp32, in any order -- what is left of a
    mean is the rounding of 1 / S and of the product with it, 1.2e-7, whichever way a kernel associates."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-64, 65, shape, generator=g).float() / 64


def ints(n, hi, seed=0, ends=True):
    """n int32 in [0, hi) with repeats; the first two are 0 and hi - 1."""
    g = torch.Generator().manual_seed(seed)
    i = torch.randint(0, hi, (n,), generator=g, dtype=torch.int32)
    if ends and n >= 2:
        i[0], i[1] = 0, hi - 1
    return i


# ---------------------------------------------------------------------------------------------------------------------
# host statements (fp64, or exact where the kernel moves / combines elements without a reduction)
# ---------------------------------------------------------------------------------------------------------------------
def embed_pe_ref(table, ids, pe, period):
    out = table[ids.long()].double()
    if pe is not None:
        out = out + pe[torch.arange(ids.numel()) % period].double()
    return out.float()                                   # one addition of two fp32 values of like magnitude: exact in fp64


def mean_pool_ref(x, n_seq, S_):
    return x.double().view(n_seq, S_, x.shape[1]).mean(dim=1)


def news_xin_ref(tb, nblk_t, bb, nblk_b, title_row, body_row, cap):
    """-> [2 cap, dim] fp64: row j the mean of the nblk_t block rows of pooled sequence title_row[j], row cap + j the same of the body."""
    dim = tb.shape[1]
    t = tb.double().view(cap, nblk_t, dim).mean(dim=1)[title_row.long()]
    b = bb.double().view(cap, nblk_b, dim).mean(dim=1)[body_row.long()]
    return torch.cat([t, b])


def fuse_rows_ref(a, b, gate=None):
    if gate is None:
        return (a.double() + b.double()).float()
    ad, bd, gd = a.double(), b.double(), gate.double()
    return gd * ad + (1.0 - gd) * bd


def fuse_rows_gated_f32(a, b, gate):
    """The kernel's expression with its association, every operation rounded to fp32 (no contraction)."""
    return gate * a + (1.0 - gate) * b


def gather_ref(table, idx):
    return table[idx.long()]


def row_scale_ref(x, scale):
    return (x.double() * scale.double()[:, None]).float()


def pad_heads_ref(src, n_blk, hd, hs):
    cols = src.shape[1]
    out = torch.zeros(n_blk, hs, cols)
    out[:, :hd] = src.view(n_blk, hd, cols)
    return out.view(n_blk * hs, cols)


def gate_mul_ref(x, g, div=1, scale=1.0, sigmoid=True):
    """sigmoid: fp64; otherwise the two multiplications in fp32, in the kernel's order (nothing to contract)."""
    if sigmoid:
        return x.double() * torch.sigmoid(g.double())
    return x * g.repeat_interleave(div, dim=0)[:x.shape[0]] * torch.tensor(scale, dtype=torch.float32)


def fill_pad_rows_ref(ids, src, dst, S_):
    out = dst.clone()
    r = torch.nonzero(ids == 0).view(-1)
    out[r] = src[r % S_]
    return out


def relu_bwd_ref(dh, h, scale):
    return torch.where(h > 0, (dh.double() * float(torch.tensor(scale, dtype=torch.float32))).float(), torch.zeros(()))


def colsum_ref(x, base=None):
    s = x.double().sum(0)
    return s if base is None else s + base.double()


def layernorm_bwd_inputs(M, E, div):
    z, gamma, beta = rnd(M, E, seed=31), rnd(E, seed=32) * 0.5 + 1.0, rnd(E, seed=33)
    dy = rnd((M + div - 1) // div, E, seed=34)
    return z, gamma, beta, dy


def nll_softmax_ref(logits):
    """-> (loss [1], dlogits) of mean_b -log_softmax(logits[b])[0], fp64 autograd."""
    x = logits.double().requires_grad_()
    loss = (-torch.log_softmax(x, dim=1)[:, 0]).mean()
    loss.backward()
    return loss.detach().reshape(1), x.grad


def additive_pool_ref(hidden, a2, x, mask, n_seq, S_, dout=None):
    """layers.Attention over the tokens of each sequence, masked with -1e9 -> rep, or (rep, dhidden, da2, dx) under ``dout``."""
    h, a, xx = (t.double().requires_grad_() for t in (hidden, a2, x))
    score = (h @ a).view(n_seq, S_).masked_fill(mask == 0, -1e9)
    rep = (torch.softmax(score, dim=1).unsqueeze(-1) * xx.view(n_seq, S_, -1)).sum(dim=1)
    if dout is None:
        return rep.detach()
    rep.backward(dout.double())
    return rep.detach(), h.grad, a.grad, xx.grad


def intent_fuse_ref(intents, hidden, a2t, a2b, M, k, dcontent=None):
    """[title pool, (cos + 1) / 2 * body pool] per news -> content [M, 2 D], or (content, d intents, d hidden, d a2t, d a2b)."""
    x, h, wt, wb = (t.double().requires_grad_() for t in (intents, hidden, a2t, a2b))
    D, A = intents.shape[1], hidden.shape[1]

    def pool(xx, hh, w):
        alpha = torch.softmax((hh.view(M, k, A) * w).sum(-1), dim=1)
        return (alpha.unsqueeze(-1) * xx.view(M, k, D)).sum(1)
    t, b = pool(x[:M * k], h[:M * k], wt), pool(x[M * k:], h[M * k:], wb)
    sim = (torch.nn.functional.cosine_similarity(t, b, dim=1) + 1) / 2
    content = torch.cat([t, sim.unsqueeze(1) * b], dim=1)
    if dcontent is None:
        return content.detach()
    content.backward(dcontent.double())
    return content.detach(), x.grad, h.grad, wt.grad, wb.grad


def embed_bwd_ref(ids, dx, V, base=None):
    t = torch.zeros(V, dx.shape[1], dtype=torch.float64) if base is None else base.double().clone()
    return t.index_add_(0, ids.long(), dx.double())


def embed_bwd_ids(rows, V, hot_share, seed=3):
    """ids in [1, V) with ``hot_share`` of the positions on the padding word 0."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, V, (rows,), generator=g, dtype=torch.int32)
    ids[torch.randperm(rows, generator=g)[:int(hot_share * rows)]] = 0
    return ids


layernorm_bwd_ref = dc.layernorm_bwd_ref                  # fp64 autograd of F.layer_norm; dy spread as dy / div


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
def _case(entry, cid, dims, layouts, **kw):
    d = dict(entry=entry, id=cid, dims=dims, layouts=[(n, l[0], l[1]) for n, l in layouts])
    d.update(kw)
    return d


def _embed_cases():
    rows, period = 41 * 32, 32
    both = lambda cols, k: layout(cols, table=k, pe=k, out=k)
    out = []
    for pe in (True, False):
        tag = 'pe' if pe else 'nope'
        out.append(_case('embed_pe', 'dim300-' + tag, dict(rows=rows, dim=300, period=period, pe=pe, V=50), [
            ('C', both(300, C)), ('V', both(300, V)),
            ('ld_table', layout(300, table=S)), ('ld_pe', layout(300, pe=S)), ('ldo', layout(300, out=S)),
            ('off_table', layout(300, table=O)), ('off_pe', layout(300, pe=O)), ('off_out', layout(300, out=O)),
            ('O', both(300, O))]))
        out.append(_case('embed_pe', 'dim50-' + tag, dict(rows=rows, dim=50, period=period, pe=pe, V=50), [
            ('C', both(50, C)), ('W', both(50, W)), ('S', both(50, S))]))
    # 28,000 * 75 float4 and 7,100 * 301 floats: 8204 and 8348 workgroups' worth > 8192
    out.append(_case('embed_pe', 'sweep-vec', dict(rows=28000, dim=300, period=period, pe=True, V=50), [('C', both(300, C))]))
    out.append(_case('embed_pe', 'sweep-scalar', dict(rows=7100, dim=301, period=period, pe=True, V=50), [('C', both(301, C))]))
    return out


def _mean_pool_cases():
    x4 = lambda dim: [('C', layout(dim, x=C, out=C)), ('V', layout(dim, x=V, out=V)), ('S', layout(dim, x=S, out=C)),
                      ('O', layout(dim, x=O, out=C)), ('out-O', layout(dim, x=C, out=O))]
    out = []
    for n_seq, S_ in ((700, 1), (700, 3), (700, 16)):                        # flat: n_seq >= 512, S <= 16; S / O: the scalar body, same order
        out.append(_case('mean_pool', 'n%d-S%d-dim300' % (n_seq, S_), dict(n_seq=n_seq, S=S_, dim=300, live=None), x4(300)))
    for S_, dim, n_seq in ((1, 4, 37), (3, 4, 37), (300, 4, 3), (1, 300, 37), (32, 300, 37), (300, 300, 3), (3, 1024, 37), (32, 1024, 3)):
        out.append(_case('mean_pool', 'n%d-S%d-dim%d' % (n_seq, S_, dim), dict(n_seq=n_seq, S=S_, dim=dim, live=None), x4(dim)))
    out.append(_case('mean_pool', 'n37-S32-dim50', dict(n_seq=37, S=32, dim=50, live=None),
                     [('C', layout(50, x=C, out=C)), ('W', layout(50, x=W, out=W))]))
    out.append(_case('mean_pool', 'n3-S32-dim1028', dict(n_seq=3, S=32, dim=1028, live=None), [('C', layout(1028, x=C, out=C))]))
    for live in (0, 333, 700, 900):                                          # counted, against the uncounted rows
        out.append(_case('mean_pool', 'n700-S3-dim300-live%d' % live, dict(n_seq=700, S=3, dim=300, live=live),
                         [('C', layout(300, x=C, out=C)), ('V', layout(300, x=V, out=V)), ('out-O', layout(300, x=C, out=O))]))
    out.append(_case('mean_pool', 'n37-S16-dim300-live20', dict(n_seq=37, S=16, dim=300, live=20),      # counted below 512 sequences: flat
                     [('C', layout(300, x=C, out=C)), ('V', layout(300, x=V, out=V))]))
    # refusals of the counted form: S > 16, and each way out of the vector layout
    out.append(_case('mean_pool', 'refused-S17', dict(n_seq=37, S=17, dim=300, live=20), [('C', layout(300, x=C, out=C))]))
    out.append(_case('mean_pool', 'refused-layout', dict(n_seq=37, S=3, dim=300, live=20),
                     [('S', layout(300, x=S, out=C)), ('O', layout(300, x=O, out=C))]))
    out.append(_case('mean_pool', 'refused-dim50', dict(n_seq=37, S=3, dim=50, live=20), [('W', layout(50, x=W, out=W))]))
    return out


def _news_xin_cases():
    out = []
    ok = [('C', layout(300, title_blocks=C, body_blocks=C, xin=C)), ('V', layout(300, title_blocks=V, body_blocks=V, xin=V)),
          ('xin-wide', layout(300, title_blocks=C, body_blocks=V, xin=(400, 0)))]
    for nt, nb in ((1, 1), (4, 16), (16, 1)):
        for live in (0, 5, 9, 12):
            out.append(_case('news_xin', 'nblk%d-%d-live%d' % (nt, nb, live), dict(cap=9, dim=300, nblk_t=nt, nblk_b=nb, live=live), ok))
    out.append(_case('news_xin', 'refused', dict(cap=9, dim=300, nblk_t=4, nblk_b=4, live=5), [
        ('ld_t', layout(300, title_blocks=S)), ('ld_b', layout(300, body_blocks=S)), ('ldx', layout(300, xin=S)),
        ('off_t', layout(300, title_blocks=O)), ('off_b', layout(300, body_blocks=O)), ('off_x', layout(300, xin=O))]))
    out.append(_case('news_xin', 'refused-dim50', dict(cap=9, dim=50, nblk_t=4, nblk_b=4, live=5),
                     [('W', layout(50, title_blocks=W, body_blocks=W, xin=W))]))
    return out


def _elementwise_cases():
    out = []
    for gated in (False, True):
        tag = 'gated' if gated else 'add'
        all_ = lambda cols, k: layout(cols, a=k, b=k, gate=k, out=k)
        for rows, cols in ((37, 300), (33, 33)):
            out.append(_case('fuse_rows', '%s-%dx%d' % (tag, rows, cols), dict(rows=rows, cols=cols, gated=gated), [
                ('C', all_(cols, C)), ('V', all_(cols, V)), ('lda', layout(cols, a=S)), ('ldb', layout(cols, b=S)),
                ('ldg', layout(cols, gate=S)), ('ldo', layout(cols, out=S)), ('O', all_(cols, O))]))
        out.append(_case('fuse_rows', tag + '-sweep', dict(rows=1800, cols=300, gated=gated), [('S', all_(300, S))]))   # 540,000 > 524,288
    g4 = [('C', layout(300, table=C, out=C)), ('V', layout(300, table=V, out=V)), ('S', layout(300, table=S, out=C)),
          ('O', layout(300, table=C, out=O))]
    out.append(_case('gather_rows', '700-from-50', dict(rows=700, cols=300, n=50), g4))
    out.append(_case('gather_rows', 'sweep', dict(rows=1800, cols=300, n=50), [('S', layout(300, table=S, out=V))]))
    out.append(_case('row_scale', '700x300', dict(rows=700, cols=300), [('C', layout(300, x=C)), ('off1', layout(300, x=(300, 1)))]))
    out.append(_case('row_scale', 'sweep', dict(rows=1800, cols=300), [('C', layout(300, x=C))]))
    p4 = lambda cols: [('C', layout(cols, src=C, dst=C)), ('V', layout(cols, src=V, dst=V)), ('S', layout(cols, src=S, dst=C)),
                       ('O', layout(cols, src=C, dst=O))]
    out.append(_case('pad_heads', 'matrix', dict(n_blk=6, hd=20, hs=32, cols=300), p4(300)))
    out.append(_case('pad_heads', 'vector', dict(n_blk=60, hd=20, hs=32, cols=1), p4(1)))
    out.append(_case('pad_heads', 'sweep', dict(n_blk=60, hd=20, hs=32, cols=300), [('S', layout(300, src=S, dst=V))]))   # 576,000 > 524,288
    rows = 37 * 8
    out.append(_case('fill_pad_rows', '296x300', dict(rows=rows, cols=300, S=8), [
        ('C', layout(300, src=C, dst=C)), ('V', layout(300, src=V, dst=V)), ('dst-wide', layout(300, src=C, dst=(900, 300)))]))
    out.append(_case('fill_pad_rows', 'refused', dict(rows=rows, cols=300, S=8), [
        ('lds', layout(300, src=S)), ('ldd', layout(300, dst=S)), ('off_src', layout(300, src=O)), ('off_dst', layout(300, dst=O))]))
    out.append(_case('fill_pad_rows', 'refused-cols50', dict(rows=rows, cols=50, S=8), [('W', layout(50, src=W, dst=W))]))
    r4 = [('C', layout(300, dh=C, h=C)), ('V', layout(300, dh=V, h=V)), ('lddh', layout(300, dh=S)), ('ldh', layout(300, h=S)),
          ('O', layout(300, dh=O, h=O))]
    for scale in (1.0, 0.37):
        out.append(_case('relu_bwd_', '296x300-scale%g' % scale, dict(rows=rows, cols=300, scale=scale), r4))
    out.append(_case('relu_bwd_', 'sweep', dict(rows=7100, cols=300, scale=0.37), [('S', layout(300, dh=S, h=V))]))     # 2,130,000 > 2,097,152
    return out


def _gate_mul_cases():
    out = []
    ok = lambda cols: [('C', layout(cols, x=C, g=C, out=C))]
    for rows, cols in ((130, 96), (8, 4)):
        for live in (None, 0, rows // 2, rows + 7):
            tag = '%dx%d-live%s' % (rows, cols, live)
            out.append(_case('gate_mul', 'sigmoid-' + tag, dict(rows=rows, cols=cols, sigmoid=True, div=1, scale=1.0, live=live), ok(cols)))
            out.append(_case('gate_mul', 'div4-' + tag, dict(rows=rows, cols=cols, sigmoid=False, div=4, scale=0.37, live=live), ok(cols)))
        out.append(_case('gate_mul', 'div1-%dx%d' % (rows, cols), dict(rows=rows, cols=cols, sigmoid=False, div=1, scale=1.0, live=None), ok(cols)))
    out.append(_case('gate_mul', 'refused', dict(rows=130, cols=96, sigmoid=True, div=1, scale=1.0, live=None), [
        ('ldx', layout(96, x=V)), ('ldg', layout(96, g=V)), ('ldo', layout(96, out=V)),
        ('off_x', layout(96, x=(96, 1))), ('off_g', layout(96, g=(96, 1))), ('off_out', layout(96, out=(96, 1)))]))
    return out


# (dtype name, trailing shape) of the 17 (table, out) pairs: row bytes 50 as 50 x 1, 25 x 2; 28 and 24 bytes as words; 3 bytes on a tail alone
GATHER_MULTI_PAIRS = [('uint8', (50,)), ('int16', (25,)), ('float32', (7,)), ('int64', (3,)), ('uint8', (3,)), ('float32', (5, 3)),
                      ('int16', (4,)), ('uint8', (1,))] + [('int32', (k + 1,)) for k in range(9)]
GATHER_MULTI_ROWS, GATHER_MULTI_TABLE = 130, 40


def _gather_multi_cases():
    esize = {'uint8': 1, 'int16': 2, 'int32': 4, 'float32': 4, 'int64': 8}
    idx = ints(GATHER_MULTI_ROWS, GATHER_MULTI_TABLE, seed=5).tolist()
    out = []
    for k, (dt, tail) in enumerate(GATHER_MULTI_PAIRS):
        out.append(_case('gather_rows_multi', 'pair%d-%s-%s' % (k, dt, 'x'.join(map(str, tail))),
                         dict(row_bytes=esize[dt] * math.prod(tail), idx=idx, n_pairs=len(GATHER_MULTI_PAIRS), pair=k), [('C', ({}, {}))]))
    return out


def _colsum_cases():
    out = []
    for N in (7, 300, 301):
        for M in (1, 255, 257):
            out.append(_case('colsum', 'M%d-N%d' % (M, N), dict(M=M, N=N, accumulate=False),
                             [('C', layout(N, x=C, out=C)), ('V', layout(N, x=V, out=C)), ('S', layout(N, x=S, out=C)), ('O', layout(N, x=O, out=C))]))
        out.append(_case('colsum', 'M70000-N%d' % N, dict(M=70000, N=N, accumulate=False), [('C', layout(N, x=C, out=C))]))
        out.append(_case('colsum', 'accumulate-M257-N%d' % N, dict(M=257, N=N, accumulate=True),
                         [('V', layout(N, x=V, out=C)), ('out-off1', layout(N, x=C, out=(N, 1)))]))
    return out


def _layernorm_bwd_cases():
    out = []
    trio = lambda E, k: layout(E, dy=k, y=k, dz=k)
    for div in (1, 16):
        for E in (100, 300, 400, 512):
            lay = [('C', trio(E, C)), ('V', trio(E, V))]
            if E == 300:
                lay += [('lddy', layout(E, dy=S)), ('ldy', layout(E, y=S)), ('lddz', layout(E, dz=S)), ('off_dy', layout(E, dy=O)),
                        ('off_y', layout(E, y=O)), ('off_dz', layout(E, dz=O)), ('off_gamma', layout(E, gamma=(E, 1))),
                        ('off_beta', layout(E, beta=(E, 1))), ('S', trio(E, S))]
            out.append(_case('layernorm_bwd', 'E%d-div%d' % (E, div), dict(M=96, E=E, div=div), lay))
        for E in (50, 301, 450):
            out.append(_case('layernorm_bwd', 'E%d-div%d' % (E, div), dict(M=96, E=E, div=div), [('C', trio(E, C)), ('W', trio(E, W))]))
    out.append(_case('layernorm_bwd', 'sweep-E100-div16', dict(M=12309, E=100, div=16), [('V', trio(100, V))]))           # 12309 > 768 * 16 rows
    out.append(_case('layernorm_bwd', 'refused-E516', dict(M=96, E=516, div=1), [('C', trio(516, C))]))
    return out


def _tail_cases():
    out = []
    out.append(_case('nll_softmax', '37x5', dict(B=37, K=5), [
        ('C', layout(5, logits=C, dlogits=C)), ('V', layout(5, logits=V, dlogits=V)), ('S', layout(5, logits=S, dlogits=C)),
        ('O', layout(5, logits=O, dlogits=C)), ('dlogits-S', layout(5, logits=C, dlogits=S)), ('dlogits-O', layout(5, logits=C, dlogits=O))]))
    # additive_pool: test_kernels_gpu.py's (11, 32, 400, 200) with its lengths (an empty sequence among them)
    mix = lambda A, D, k1, k2, k3: (dict(hidden=k1(A)[0], x=k2(D)[0], out=k3(D)[0]), dict(hidden=k1(A)[1], x=k2(D)[1], out=k3(D)[1]))
    out.append(_case('additive_pool', '11x32-A400-D200', dict(n_seq=11, S=32, A=400, D=200), [
        ('C', mix(400, 200, C, C, C)), ('V', mix(400, 200, V, V, V)), ('S', mix(400, 200, S, S, S)), ('O', mix(400, 200, O, O, O)),
        ('ldh', mix(400, 200, S, C, C)), ('ldx', mix(400, 200, C, S, C)), ('ldo', mix(400, 200, C, C, S))]))
    # additive_pool_bwd: test_backward_gpu.py's (5, 100, 64, 50); its (1, 1, 200, 400) has no second row for a leading dimension to find
    def bmix(A, D, kh, kx, kd, kdh, kdx):
        names = (('hidden', kh, A), ('x', kx, D), ('dout', kd, D), ('dhidden', kdh, A), ('dx', kdx, D))
        return ({n: k(w)[0] for n, k, w in names}, {n: k(w)[1] for n, k, w in names})
    out.append(_case('additive_pool_bwd', '5x100-A64-D50', dict(n_seq=5, S=100, A=64, D=50), [
        ('C', bmix(64, 50, C, C, C, C, C)), ('V', bmix(64, 50, V, V, V, V, V)), ('S', bmix(64, 50, S, S, S, S, S)), ('O', bmix(64, 50, O, O, O, O, O)),
        ('ldh', bmix(64, 50, S, C, C, C, C)), ('ldx', bmix(64, 50, C, S, C, C, C)), ('ldo', bmix(64, 50, C, C, S, C, C)),
        ('lddh', bmix(64, 50, C, C, C, S, C)), ('lddx', bmix(64, 50, C, C, C, C, S))]))
    # intent_fuse / intent_fuse_bwd: test_backward_gpu.py's (5, 2, 64, 48); content / dcontent are [M, 2 D] windows: also inside a wider
    # row at a column offset, as the model's `fused[:, 900:]`
    win = lambda name: [('C', layout(128, **{name: C})), ('V', layout(128, **{name: V})), ('S', layout(128, **{name: S})),
                        ('O', layout(128, **{name: O})), ('column-offset', layout(128, **{name: (237, 100)}))]
    for live in (None, 0, 3, 9):
        out.append(_case('intent_fuse', '5x2-D64-A48-live%s' % live, dict(M=5, k=2, D=64, A=48, live=live), win('content')))
    out.append(_case('intent_fuse_bwd', '5x2-D64-A48', dict(M=5, k=2, D=64, A=48), win('dcontent')))
    # embed_bwd: strided dx, a table wider than D, the three back ends; 0.4 * 22,000 >= 8192 positions of the padding word: pass H
    e3 = lambda D: [('C', layout(D, dx=C, dtable=C)), ('V', layout(D, dx=V, dtable=V)), ('S', layout(D, dx=S, dtable=S)),
                    ('O', layout(D, dx=O, dtable=O)), ('lddx', layout(D, dx=S, dtable=C)), ('ld_table', layout(D, dx=C, dtable=(D + 37, 20)))]
    out.append(_case('embed_bwd', 'sorted-9000', dict(rows=9000, V=500, D=300, deterministic=True, hot_share=0.4), e3(300)))
    out.append(_case('embed_bwd', 'sorted-22000', dict(rows=22000, V=500, D=300, deterministic=True, hot_share=0.4), [('S', layout(300, dx=S, dtable=S))]))
    out.append(_case('embed_bwd', 'atomics-9000', dict(rows=9000, V=500, D=300, deterministic=False, hot_share=0.4), e3(300)))
    out.append(_case('embed_bwd', 'atomics-D400', dict(rows=1760, V=500, D=400, deterministic=True, hot_share=0.4), e3(400)[:3]))
    out.append(_case('embed_bwd', 'small-1760', dict(rows=1760, V=10, D=500, deterministic=True, hot_share=0.4), e3(500)))
    return out


CASES = (_tail_cases() + _embed_cases() + _mean_pool_cases() + _news_xin_cases() + _elementwise_cases() + _gate_mul_cases() + _gather_multi_cases() +
         _colsum_cases() + _layernorm_bwd_cases())


def cases_of(entry):
    return [c for c in CASES if c['entry'] == entry]


def ids_of(entry):
    return [c['id'] for c in cases_of(entry)]


def flat():
    """Every (case, layout) of the table -> (entry, 'case/layout', dims, lds, offs)."""
    for c in CASES:
        for name, lds, offs in c['layouts']:
            yield c['entry'], '%s/%s' % (c['id'], name), c['dims'], lds, offs


# what the table must select: (entry, body, second sweep)
REQUIRED = [
    ('embed_pe', 'embed_pe_kernel<4>', False), ('embed_pe', 'embed_pe_scalar_kernel', False),
    ('embed_pe', 'embed_pe_kernel<4>', True), ('embed_pe', 'embed_pe_scalar_kernel', True),
    ('mean_pool', 'mean_pool_flat_kernel', False), ('mean_pool', 'mean_pool_vec4_kernel', False), ('mean_pool', 'mean_pool_kernel', False),
    ('mean_pool', 'refused', False),
    ('news_xin', 'news_xin_kernel', False), ('news_xin', 'refused', False),
    ('fuse_rows', 'fuse_rows_kernel', False), ('fuse_rows', 'fuse_rows_kernel', True),
    ('gather_rows', 'gather_rows_kernel', False), ('gather_rows', 'gather_rows_kernel', True),
    ('row_scale', 'row_scale_kernel', False), ('row_scale', 'row_scale_kernel', True),
    ('pad_heads', 'pad_heads_kernel', False), ('pad_heads', 'pad_heads_kernel', True),
    ('fill_pad_rows', 'fill_pad_rows_kernel', False), ('fill_pad_rows', 'refused', False),
    ('relu_bwd_', 'relu_bwd_kernel', False), ('relu_bwd_', 'relu_bwd_kernel', True),
    ('gate_mul', 'gate_mul_kernel:sigmoid', False), ('gate_mul', 'gate_mul_kernel:scale', False), ('gate_mul', 'refused', False),
    ('gather_rows_multi', 'word', True), ('gather_rows_multi', 'byte/word+tail', True), ('gather_rows_multi', 'byte/tail', True),
    ('colsum', 'reduce_partials_vec4_kernel:one', False), ('colsum', 'reduce_partials_vec4_kernel:several', False),
    ('colsum', 'reduce_partials_kernel:one', False), ('colsum', 'reduce_partials_kernel:several', False),
    ('layernorm_bwd', 'layernorm_bwd_vec_kernel<2>', False), ('layernorm_bwd', 'layernorm_bwd_vec_kernel<5>', False),
    ('layernorm_bwd', 'layernorm_bwd_vec_kernel<8>', False), ('layernorm_bwd', 'layernorm_bwd_vec_kernel<2>', True),
    ('layernorm_bwd', 'layernorm_bwd_kernel<2>', True), ('layernorm_bwd', 'layernorm_bwd_kernel<5>', True),
    ('layernorm_bwd', 'layernorm_bwd_kernel<8>', True), ('layernorm_bwd', 'refused', False),
    ('nll_softmax', 'nll_softmax_kernel', False), ('additive_pool', 'additive_pool_kernel', False),
    ('additive_pool_bwd', 'additive_pool_bwd_kernel', False), ('intent_fuse', 'intent_fuse_kernel', False),
    ('intent_fuse_bwd', 'intent_fuse_bwd_kernel', False),
    ('embed_bwd', 'embed_bwd_small_kernel', False), ('embed_bwd', 'embed_bwd_sorted', False), ('embed_bwd', 'embed_bwd_sorted + pass H', False),
    ('embed_bwd', 'embed_bwd_kernel<5>', False), ('embed_bwd', 'embed_bwd_kernel<8>', False),
]

# the conditions of each 16-byte body that some layout must violate with every other condition met
ALONE = {
    'embed_pe': ['width', 'ld:table', 'ld:pe', 'ld:out', 'off:table', 'off:pe', 'off:out'],
    'mean_pool': ['width', 'ld:x', 'off:x'],
    'news_xin': ['width', 'ld:title_blocks', 'ld:body_blocks', 'ld:xin', 'off:title_blocks', 'off:body_blocks', 'off:xin'],
    'fill_pad_rows': ['width', 'ld:src', 'ld:dst', 'off:src', 'off:dst'],
    'gate_mul': ['off:x', 'off:g', 'off:out'],
    'colsum': ['width', 'off:out'],
    'layernorm_bwd': ['width', 'ld:dy', 'ld:y', 'ld:dz', 'off:dy', 'off:y', 'off:dz', 'off:gamma', 'off:beta'],
}
