"""The bf16 token-encoder kernels (csrc/token_attn_bf16.hip, inproj_bf16.hip, ffn_bf16.hip, lime_linear_bf16, lime_mean_pool_bf16)
against their fp64 statements (tests/bf16_cases.py: the arithmetic of each kernel's header comment, bf16 roundings where the kernel
rounds, fp64 everywhere else), judged by ``bf16_cases.assert_bf16_matches``: a derived hard bound per element and at most 1 % of the
elements off bf16(fp64) -- a kernel that is an ulp off in one lane, column or row class fails.  The shapes are the smallest that reach
each branch: every S, head_dim / n_head edges, output padding and leading dimensions, the compacted (row_map, n_seq_dev) attention, the
dense / gathered / scattered in_proj with junk behind K, every accepted E class of the fused ffn / block, device row counts, and -- sized
from the CU count -- a second iteration of each persistent loop.  Inputs and references come from bf16_cases (seeded CPU generators,
cached per case); tests/test_bf16_reference_cpu.py shows that fp32 CPU evaluations of the same statements pass the same criterion."""
import math

import numpy as np
import pytest
import torch

import bf16_cases as C
from bf16_cases import SENTINEL, EP, assert_bf16_matches
from helpers import rel_err

pytestmark = pytest.mark.gpu

OBSERVED = {}           # kernel -> [worst share, worst distance] over this module's run (printed at the end: pytest -s)


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from lime_cikm25_amd import ops as _ops
    from lime_cikm25_amd import _lib
    _lib.load()
    yield _ops
    for k, (share, worst) in sorted(OBSERVED.items()):
        print('\nobserved, %s: at most %.4f %% of a case\'s elements differ from bf16(fp64), worst %.3f ulp' % (k, 100 * share, worst))


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def dev(t):
    return None if t is None else t.cuda()


def matches(kernel, got, want64, single_rounding, what):
    share, worst = assert_bf16_matches(got, want64.to(got.device), single_rounding, what)
    o = OBSERVED.setdefault(kernel, [0.0, 0.0])
    o[0], o[1] = max(o[0], share), max(o[1], worst)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def sentinel(rows, cols, dtype=torch.bfloat16):
    return torch.full((rows, cols), SENTINEL, dtype=dtype, device='cuda')


def refused():
    from lime_cikm25_amd._lib import LimeHipError
    return pytest.raises(LimeHipError)


# ---------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------
def run_attn_dense(ops, S, n_seq, h, hd, out_cols, ldo, kernel='attention'):
    qkv, scale, want = C.attn_inputs(S, n_seq, h, hd)
    d, W, real = dev(qkv), h * 32, h * hd
    oc = real if out_cols is None else out_cols
    buf = sentinel(n_seq * S, oc if ldo is None else ldo)
    ops.token_attention_bf16(d[:, :W], d[:, W:2 * W], d[:, 2 * W:], n_seq, S, h, hd, scale, out_cols=oc, out=buf[:, :oc])
    matches(kernel, buf[:, :real], want, None, 'attention S=%d n_seq=%d h=%d hd=%d' % (S, n_seq, h, hd))
    assert (buf[:, real:oc] == 0).all(), 'the columns behind the last head are zero'
    assert (buf[:, oc:] == SENTINEL).all(), 'nothing is written behind out_cols'


@pytest.mark.parametrize('S,n_seq,h,hd,out_cols,ldo', C.ATTN_DENSE_PARAMS)
def test_token_attention_bf16_shapes(ops, S, n_seq, h, hd, out_cols, ldo):
    run_attn_dense(ops, S, n_seq, h, hd, out_cols, ldo, 'attention' if C.attn_rounds_p(S, hd) else 'attention (fp32 core)')


@pytest.mark.parametrize('which', [0, 1], ids=['S128', 'S32'])
def test_token_attention_bf16_second_iteration_of_the_persistent_loop(ops, which):
    """More groups than the grid holds workgroups: the prefetch under a group's work, the second stash, and (S = 32) a last group with
    two of its four pairs invalid."""
    S, n_seq, h, hd = C.attn_loop_cases(n_cu())[which]
    G, per_cu = (1, 3) if S == 128 else (4, 4)
    groups = -(-n_seq * h // G)
    assert n_cu() * per_cu < groups < 2 * n_cu() * per_cu and (S == 128 or (n_seq * h) % 4 == 2)
    run_attn_dense(ops, S, n_seq, h, hd, None, None)


def random_ids(n_seq, S, seed, p_empty, vocab):
    """Padded id sequences: random lengths, all-padding sequences, padding words inside a text (as tests/test_compact_gpu.py)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, S + 1, size=n_seq)
    lens[rng.random(n_seq) < p_empty] = 0
    ids = rng.integers(1, vocab, size=(n_seq, S))
    ids[np.arange(S)[None, :] >= lens[:, None]] = 0
    ids[rng.random((n_seq, S)) < 0.02] = 0
    return torch.from_numpy(ids.astype(np.int32))


@pytest.mark.parametrize('S', [32, 128])
def test_compacted_attention_equals_the_dense_kernel_on_the_gathered_rows(ops, S):
    """ids with live sequences, padding tails and all-padding sequences through compact_sequences; q / k / v from the bf16 in_proj over
    the live tokens and the S padding rows (rows it does not write stay NaN: nothing may read them); attention through row_map equals
    the dense kernel on the materialised rows bit for bit, and the fp64 statement."""
    n_seq, h, hd, V, E, K, N = 70, 10, 30, 400, 300, 304, 960
    W, scale = h * 32, 1.0 / math.sqrt(hd)
    ids = random_ids(n_seq, S, seed=S, p_empty=0.3, vocab=V).cuda()
    c = ops.compact_sequences(ids)
    n_c = int(c.counts[0])
    assert 1 < n_c < n_seq + 1
    table = C.padded_bf16(C.rnd(V, E, seed=S + 1, scale=2.0), K)
    w = torch.zeros(3 * h, 32, E)
    w[:, :hd] = C.rnd(3 * h, hd, E, seed=S + 2, scale=0.1)                  # heads padded to 32 columns: zero weights, zero add rows
    add = torch.zeros(S, 3 * h, 32)
    add[:, :, :hd] = C.rnd(S, 3 * h, hd, seed=S + 3)
    qkv = torch.full((c.cap + S, N), float('nan'), dtype=torch.bfloat16, device='cuda')
    ops.inproj_bf16(dev(table), ops.inproj_pack_bf16(dev(w.view(N, E)), K), dev(add.view(S, N)), N, qkv, a_ids=c.tok_ids, c_ids=c.tok_rows,
                    m_dev=c.n_tokens_and_pad_rows)
    full = qkv[c.row_map[:n_c * S].long()]                                   # the materialised rows of the n_c compact sequences
    assert torch.isfinite(full).all() and torch.isnan(qkv).any()
    want_bits = ops.token_attention_bf16(full[:, :W], full[:, W:2 * W], full[:, 2 * W:], n_c, S, h, hd, scale, out_cols=EP)
    out = sentinel((n_seq + 1) * S, EP)
    ops.token_attention_rows_bf16(qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:], c.row_map, c.n_compact, n_seq + 1, S, h, hd, scale, out_cols=EP,
                                  out=out)
    assert same_bits(out[:n_c * S], want_bits) and (out[n_c * S:] == SENTINEL).all()
    f = full.cpu()
    matches('attention (row_map)', out[:n_c * S, :h * hd], C.attn64(f[:, :W], f[:, W:2 * W], f[:, 2 * W:], n_c, S, h, hd, scale), None,
            'compacted attention S=%d' % S)
    assert (out[:n_c * S, h * hd:] == 0).all()


def rowmap_case(S, n_seq, h, hd, seed):
    """A q/k/v buffer larger than the batch whose rows are a random permutation of the dense case's; every other row is NaN."""
    qkv, scale, want = C.attn_inputs(S, n_seq, h, hd)
    rows = n_seq * S + 77
    row_map = torch.randperm(rows, generator=C.gen(seed))[:n_seq * S].to(torch.int32)
    buf = torch.full((rows, qkv.shape[1]), float('nan'), dtype=torch.bfloat16)
    buf[row_map.long()] = qkv
    return dev(buf), dev(row_map), scale, want


@pytest.mark.parametrize('S,hd', C.ATTN_ROWMAP)
def test_token_attention_rows_bf16_reads_through_the_row_map(ops, S, hd):
    n_seq, h = 5, 10
    buf, row_map, scale, want = rowmap_case(S, n_seq, h, hd, seed=S + hd)
    W, real = h * 32, h * hd
    oc = max(real, EP)                              # head_dim 30: four zero columns behind the heads; 32: out_pad = 0
    out = sentinel(n_seq * S, oc + 8)
    ops.token_attention_rows_bf16(buf[:, :W], buf[:, W:2 * W], buf[:, 2 * W:], row_map, None, n_seq, S, h, hd, scale, out_cols=oc, out=out[:, :oc])
    matches('attention (row_map)', out[:, :real], want, None, 'row_map attention S=%d hd=%d' % (S, hd))
    assert (out[:, real:oc] == 0).all() and (out[:, oc:] == SENTINEL).all()


def test_token_attention_rows_bf16_device_sequence_count(ops):
    """n_seq_dev clamps to [0, n_seq]: the counted sequences equal the uncounted run bit for bit, the others are not written."""
    S, n_seq, h, hd = 64, 6, 10, 30
    buf, row_map, scale, _ = rowmap_case(S, n_seq, h, hd, seed=3)
    W = h * 32
    run = lambda cnt, out: ops.token_attention_rows_bf16(buf[:, :W], buf[:, W:2 * W], buf[:, 2 * W:], row_map, cnt, n_seq, S, h, hd, scale,
                                                         out_cols=EP, out=out)
    ref = run(None, sentinel(n_seq * S, EP))
    assert not (ref == SENTINEL).any()
    for cnt in (0, 1, n_seq // 2, n_seq, n_seq + 5, -3):
        out = run(torch.tensor([cnt], dtype=torch.int32, device='cuda'), sentinel(n_seq * S, EP))
        k = min(max(cnt, 0), n_seq) * S
        assert same_bits(out[:k], ref[:k]) and (out[k:] == SENTINEL).all(), 'n_seq_dev = %d' % cnt


def test_token_attention_rows_bf16_refusals(ops):
    """The shapes the entry point states it does not take (argument checks: nothing is launched)."""
    h, hd, n_seq = 2, 30, 2
    q = torch.zeros(n_seq * 128, h * 32, dtype=torch.bfloat16, device='cuda')
    rm = torch.arange(n_seq * 256, dtype=torch.int32, device='cuda') % (n_seq * 128)
    call = lambda S, hd_, **kw: ops.token_attention_rows_bf16(q, q, q, rm, None, n_seq, S, h, hd_, 0.2, **kw)
    assert call(32, hd).shape == (n_seq * 32, h * hd)                          # the same arguments with an accepted shape
    for S, hd_, kw in ((96, hd, {}), (256, hd, {}), (32, 15, {}), (32, 34, {}), (32, hd, dict(out_cols=h * hd - 2)),
                       (32, hd, dict(out_cols=h * hd + 34))):
        with refused():
            call(S, hd_, **kw)
    with refused():                                                             # ldo < out_cols
        ops.token_attention_rows_bf16(q, q, q, rm, None, n_seq, 32, h, hd, 0.2, out_cols=h * hd + 4, out=sentinel(n_seq * 32, h * hd))
    with refused():
        ops.token_attention_bf16(q[:192], q[:192], q[:192], 2, 96, h, hd, 0.2)


# ---------------------------------------------------------------------------------------------------
# in_proj
# ---------------------------------------------------------------------------------------------------
def inproj_operands(d, M, K):
    """The three forms of the A operand: (a, a_ids) gathered from the table; dense rows; dense rows as the [:, :K] view of a buffer whose
    columns behind K hold NaN and 3e38 (legal: lda > K)."""
    table, ids = dev(d['table']), dev(d['ids'])
    rows = table[ids.long()].contiguous()
    junk = torch.empty((M, K + 32), dtype=torch.bfloat16, device='cuda')
    junk[:, K::2], junk[:, K + 1::2] = float('nan'), 3e38
    junk[:, :K] = rows
    return (('gathered', table, ids), ('dense', rows, None), ('dense, junk behind K', junk[:, :K], None))


@pytest.mark.parametrize('period', ['1', 'S'])
@pytest.mark.parametrize('M,K,N,S', C.INPROJ_PARAMS)
def test_inproj_bf16_forms(ops, M, K, N, S, period):
    """Gathered / dense / dense-with-junk operand rows, results in place and scattered by c_ids into a larger sentinel-filled buffer with
    ldo > N; the periodic fp32 row is that of the OUTPUT row.  The first form is held to the fp64 statement, the others to its bits."""
    M = C.inproj_m(M, n_cu())
    period = 1 if period == '1' else S
    d = C.inproj_inputs(M, K, N, S)
    wp, add = ops.inproj_pack_bf16(dev(d['w']), K), dev(d['adds'][period])
    forms = inproj_operands(d, M, K)
    for scattered in (False, True):
        want, bound = C.inproj_want(M, K, N, S, period, scattered)
        c_ids = dev(d['c_ids']) if scattered else None
        first = None
        for name, a, a_ids in forms:
            what = 'in_proj M=%d K=%d N=%d period=%d %s%s' % (M, K, N, period, name, ', scattered' if scattered else '')
            buf = sentinel(d['cap'], N + 4) if scattered else sentinel(M, N)
            out = buf[:, :N]
            ops.inproj_bf16(a, wp, add, N, out, a_ids=a_ids, c_ids=c_ids)
            got = out[c_ids.long()] if scattered else out
            assert torch.isfinite(got).all(), what
            if first is None:
                first = got
                matches('in_proj', got, want, bound, what)
            else:
                assert same_bits(got, first), what
            if scattered:
                rest = torch.ones(d['cap'], dtype=torch.bool, device='cuda')
                rest[c_ids.long()] = False
                assert (buf[rest] == SENTINEL).all() and (buf[:, N:] == SENTINEL).all(), what


@pytest.mark.parametrize('M,K,N,S', C.INPROJ_PARAMS)
def test_inproj_bf16_device_row_count(ops, M, K, N, S):
    M = C.inproj_m(M, n_cu())
    d = C.inproj_inputs(M, K, N, S)
    wp, add, table, ids, c_ids = ops.inproj_pack_bf16(dev(d['w']), K), dev(d['adds'][S]), dev(d['table']), dev(d['ids']), dev(d['c_ids'])
    run = lambda m_dev: ops.inproj_bf16(table, wp, add, N, sentinel(d['cap'], N), a_ids=ids, c_ids=c_ids, m_dev=m_dev)[c_ids.long()]
    full = run(None)
    for m in C.INPROJ_M_DEV:
        m = M + 7 if m == 'over' else m
        got = run(torch.tensor([m], dtype=torch.int32, device='cuda'))
        k = min(m, M)
        assert same_bits(got[:k], full[:k]) and (got[k:] == SENTINEL).all(), 'm_dev = %d' % m


@pytest.mark.parametrize('K,N', [(64, 320), (320, 960)])
def test_inproj_pack_bf16_layout(ops, K, N):
    """packed [pass][chunk][320 rows][32 k]; row 16 t + 4 kg + q of a pass is output column 32 (t >> 1) + 8 kg + 4 (t & 1) + q; zero
    beyond the weight's columns."""
    E = C.INPROJ_E[K]
    w = C.rnd(N, E, seed=K, scale=0.06)
    wv = ops.inproj_pack_bf16(dev(w), K).cpu().view(N // 320, 10, 10, 2, 4, 4, 32).permute(0, 2, 4, 3, 5, 1, 6).reshape(N, 320)
    assert same_bits(wv[:, :E], C.bf(w)) and (wv[:, E:] == 0).all()


def test_inproj_bf16_rows_do_not_depend_on_their_position(ops):
    M, K, N, S = 385, 320, 960, 128
    d = C.inproj_inputs(M, K, N, S)
    wp, add, table, ids = ops.inproj_pack_bf16(dev(d['w']), K), dev(d['adds'][1]), dev(d['table']), dev(d['ids'])
    p = torch.randperm(M, generator=C.gen(9)).cuda()
    a = ops.inproj_bf16(table, wp, add, N, sentinel(M, N), a_ids=ids)
    b = ops.inproj_bf16(table, wp, add, N, sentinel(M, N), a_ids=ids[p].contiguous())
    assert same_bits(b, a[p])


# ---------------------------------------------------------------------------------------------------
# fused ffn and block
# ---------------------------------------------------------------------------------------------------
def wide(t, ld, rows=None):
    """t [M, C] as the [:, :C] view of a sentinel-filled [rows or M, ld] buffer -> (view, buffer)."""
    buf = sentinel(t.shape[0] if rows is None else rows, ld, t.dtype)
    buf[:t.shape[0], :t.shape[1]] = t
    return buf[:, :t.shape[1]], buf


def check_rows(kernel, got, want, E, what):
    assert got.dtype == torch.bfloat16 and got.shape == (want.shape[0], EP) and (got[:, E:] == 0).all(), what
    matches(kernel, got[:, :E], want, None, what)


def check_pool(got, want, E, tol, what):
    mb = want.shape[0] // 32 * 32
    assert got.dtype == torch.float32 and got.shape == (mb // 32, EP) and (got[:, E:] == 0).all(), what
    e = rel_err(got[:, :E].cpu().numpy(), C.pool32_64(want[:mb]).numpy())
    print('%s: block means rel err %.2e' % (what, e))
    assert e < tol, '%s: block means rel err %.3e' % (what, e)


def run_ffn(ops, E, F, M, views=True):
    x, w, want = C.ffn_inputs(E, F, M)
    what = 'ffn E=%d F=%d M=%d' % (E, F, M)
    xd = dev(x)
    w1p, w2p = ops.ffn_pack_bf16(dev(w['w1']), dev(w['b1']), dev(w['w2']))
    args = (w1p, w2p, dev(w['b2']), (dev(w['g']), dev(w['beta'])), w['eps'], E)
    got = ops.encoder_ffn_bf16(xd, *args)
    check_rows('ffn', got, want, E, what)
    mb = M // 32 * 32
    if mb:
        blocks = ops.encoder_ffn_bf16(xd[:mb], *args, pool32=True)
        check_pool(blocks, want, E, C.POOL_TOL_FFN, what)
    if views:                                        # x / out as views of wider sentinel-filled buffers: same bits, nothing else written
        xv, _ = wide(xd, 320)
        ov, obuf = wide(sentinel(M, EP), 352)
        ops.encoder_ffn_bf16(xv, *args, out=ov)
        assert same_bits(ov, got) and (obuf[:, EP:] == SENTINEL).all(), what
        if mb:
            pv, pbuf = wide(sentinel(mb // 32, EP, torch.float32), 320)
            ops.encoder_ffn_bf16(xv[:mb], *args, pool32=True, out=pv)
            assert same_bits(pv, blocks) and (pbuf[:, EP:] == SENTINEL).all(), what


@pytest.mark.parametrize('E,F', C.FFN_PARAMS)
def test_encoder_ffn_bf16_model_widths(ops, E, F):
    """Every class of E the host accepts (where the bias column sits in the last k chunk, the LayerNorm count) x the pass counts,
    at one row, a row count that ends inside a wave and one that ends inside a tile."""
    for M in C.FFN_M:
        run_ffn(ops, E, F, M)


def test_encoder_ffn_bf16_several_tiles_per_workgroup(ops):
    E, F = C.FFN_BIG
    run_ffn(ops, E, F, C.big_m(n_cu()), views=False)


def block_args(ops, d, E, kind, rows=None):
    """-> (positional + keyword arguments of ops.encoder_block_bf16 for the first ``rows`` tokens)."""
    sl = slice(None, rows)
    kw = dict(res_kind=kind, w1p=None, w2p=None, b2=dev(d['b2']), ln2=(dev(d['g']), dev(d['beta'])), ln2_eps=d['eps'], E=E)
    kw['w1p'], kw['w2p'] = ops.ffn_pack_bf16(dev(d['w1']), dev(d['b1']), dev(d['w2']))
    if kind == 2:
        kw.update(res=dev(d['table']), res_ids=dev(d['res_ids'][sl]))
    else:
        kw.update(res=dev(d['res_rows'][sl]))
    return [dev(d['attn'][sl]), ops.oproj_pack_bf16(dev(d['w0'])), dev(d['add_rows']), (dev(d['g1']), dev(d['beta1'])), d['eps1']], kw


def run_block(ops, E, kind, period, M, views=True):
    d = C.block_inputs(E, kind, period, M)
    what = 'block E=%d kind=%d period=%d M=%d' % (E, kind, period, M)
    pos, kw = block_args(ops, d, E, kind)
    got = ops.encoder_block_bf16(*pos, **kw)
    check_rows('block', got, d['want'], E, what)
    mb = M // 32 * 32
    ppos, pkw = block_args(ops, d, E, kind, rows=mb)
    blocks = ops.encoder_block_bf16(*ppos, pool32=True, **pkw)
    check_pool(blocks, d['want'], E, C.POOL_TOL_BLOCK, what)
    if views:                                        # attn / res / out as views of wider sentinel-filled buffers
        av, _ = wide(pos[0], 320)
        rv, _ = wide(kw['res'], 352)
        ov, obuf = wide(sentinel(M, EP), 320)
        ops.encoder_block_bf16(av, *pos[1:], **dict(kw, res=rv), out=ov)
        assert same_bits(ov, got) and (obuf[:, EP:] == SENTINEL).all(), what
        pv, pbuf = wide(sentinel(mb // 32, EP, torch.float32), 352)
        ops.encoder_block_bf16(av[:mb], *ppos[1:], **dict(pkw, res=rv if kind == 2 else rv[:mb]), pool32=True, out=pv)
        assert same_bits(pv, blocks) and (pbuf[:, EP:] == SENTINEL).all(), what


@pytest.mark.parametrize('E,kind,period', C.BLOCK_PARAMS)
def test_encoder_block_bf16_model_widths(ops, E, kind, period):
    """out_proj + residual + norm1 + the feed-forward half: the E classes the block accepts, the gathered and the dense residual, one
    shared add row and one per position with a row count that is no multiple of the period (nor of a tile)."""
    run_block(ops, E, kind, period, C.BLOCK_M)


def test_encoder_block_bf16_dense_residual_several_tiles_per_workgroup(ops):
    E, kind, period = C.BLOCK_BIG
    run_block(ops, E, kind, period, C.big_m(n_cu()), views=False)


@pytest.mark.parametrize('form', ['ffn', 'block', 'block pool32'])
def test_fused_encoder_device_row_count(ops, form):
    """m_dev: the first rows (block means) equal the uncounted run bit for bit, nothing behind them is written."""
    M, E, F = C.M_DEV_ROWS, 300, 512
    pool = form == 'block pool32'
    if form == 'ffn':
        x, w, _ = C.ffn_inputs(E, F, M)
        w1p, w2p = ops.ffn_pack_bf16(dev(w['w1']), dev(w['b1']), dev(w['w2']))
        xd, rest = dev(x), (w1p, w2p, dev(w['b2']), (dev(w['g']), dev(w['beta'])), w['eps'], E)
        run = lambda m_dev, out: ops.encoder_ffn_bf16(xd, *rest, m_dev=m_dev, out=out)
    else:
        pos, kw = block_args(ops, C.block_inputs(E, 2, C.BLOCK_S, M), E, 2)
        run = lambda m_dev, out: ops.encoder_block_bf16(*pos, pool32=pool, m_dev=m_dev, out=out, **kw)
    blank = lambda: sentinel(M // 32, EP, torch.float32) if pool else sentinel(M, EP)
    full = run(None, blank())
    assert (full == SENTINEL).float().mean() < 0.01                # (a result may BE 7.0; a region that was not written is all of them)
    for m in C.M_DEV:
        got = run(torch.tensor([m], dtype=torch.int32, device='cuda'), blank())
        k = m // 32 if pool else m
        assert same_bits(got[:k], full[:k]) and (got[k:] == SENTINEL).all(), '%s, m_dev = %d' % (form, m)


@pytest.mark.parametrize('form', ['ffn', 'block kind 2', 'block kind 3'])
def test_fused_encoder_rows_do_not_depend_on_their_position(ops, form):
    """Permuting the input rows permutes the bf16 output rows bit for bit: a row's arithmetic depends on neither its tile, wave nor lane."""
    M, E, F = 300, 300, 512
    p = torch.randperm(M, generator=C.gen(21))
    if form == 'ffn':
        x, w, _ = C.ffn_inputs(E, F, M)
        w1p, w2p = ops.ffn_pack_bf16(dev(w['w1']), dev(w['b1']), dev(w['w2']))
        rest = (w1p, w2p, dev(w['b2']), (dev(w['g']), dev(w['beta'])), w['eps'], E)
        a, b = ops.encoder_ffn_bf16(dev(x), *rest), ops.encoder_ffn_bf16(dev(x[p]), *rest)
    else:
        kind = int(form[-1])
        d = C.block_inputs(E, kind, 1, M)
        pos, kw = block_args(ops, d, E, kind)
        a = ops.encoder_block_bf16(*pos, **kw)
        moved = dict(kw, res_ids=dev(d['res_ids'][p])) if kind == 2 else dict(kw, res=dev(d['res_rows'][p]))
        b = ops.encoder_block_bf16(dev(d['attn'][p]), *pos[1:], **moved)
    assert same_bits(b, a[p.cuda()])


# ---------------------------------------------------------------------------------------------------
# lime_linear_bf16 as the compacted path launches it, the bf16 mean pool
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', C.LINEAR_M)
def test_linear_bf16_scatter_with_device_row_count(ops, M):
    """The two launches of the compacted in_proj when the activation-stationary kernel is not used: live tokens gathered by a_ids and
    scattered by c_ids under m_dev (fp32 periodic rows of the OUTPUT row), and the S padding rows (a_ids all zero)."""
    d = C.linear_inputs(M)
    E, S, cap = d['E'], d['S'], d['cap']
    table, w, res, ids, c_ids = dev(d['table']), dev(d['w']), dev(d['res']), dev(d['ids']), dev(d['c_ids'])
    a_rows = d['table'][d['ids'].long()]
    res_rows = d['res'][d['c_ids'].long() % S]

    def run(m):
        buf = sentinel(cap, EP)
        ops.linear_bf16(table, w, None, a_ids=ids, res=res, res_kind=1, res_mod=S, out=buf, c_ids=c_ids, n_alg=3 * E, k_alg=E,
                        m_dev=None if m is None else torch.tensor([m], dtype=torch.int32, device='cuda'))
        return buf
    full = run(None)
    got = full[c_ids.long()]
    matches('linear', got, C.linear64(a_rows, d['w'], res=res_rows), C.linear_acc_bound(a_rows, d['w'], res=res_rows), 'linear_bf16 scatter M=%d' % M)
    rest = torch.ones(cap, dtype=torch.bool, device='cuda')
    rest[c_ids.long()] = False
    assert (full[rest] == SENTINEL).all()
    for m in (0, 1, M // 2 + 1, M, M + 9):
        buf = run(m)
        k = min(m, M)
        rest[:] = True
        rest[c_ids[:k].long()] = False
        assert same_bits(buf[c_ids[:k].long()], got[:k]) and (buf[rest] == SENTINEL).all(), 'm_dev = %d' % m
    # the padding rows: S results from table row 0
    pad = ops.linear_bf16(table, w, None, a_ids=torch.zeros(S, dtype=torch.int32, device='cuda'), res=res, res_kind=1, res_mod=S)
    a0 = d['table'][:1].expand(S, EP)
    matches('linear', pad, C.linear64(a0, d['w'], res=d['res']), C.linear_acc_bound(a0, d['w'], res=d['res']), 'linear_bf16 padding rows')


@pytest.mark.parametrize('S', C.POOL_S)
def test_mean_pool_bf16(ops, S):
    n_seq, dim = 7, 300
    x = C.padded_bf16(C.rnd(n_seq * S, dim, seed=S, scale=2.0), EP)
    got = ops.mean_pool_bf16(dev(x), n_seq, S, dim).cpu().double()
    x64 = x[:, :dim].double().reshape(n_seq, S, dim)
    want = x64.mean(dim=1)
    bound = (S + 1) * 2.0 ** -24 * x64.abs().mean(dim=1)                      # an S-term fp32 sum in any order, and the division
    assert got.shape == (n_seq, dim) and bool(((got - want).abs() <= bound).all()), float(((got - want).abs() / bound).max())
