"""The proof, on the CPU, that tests/row_layout_cases.py covers what tests/test_row_layout_gpu.py claims: through ``branch_of`` (the host
dispatch of the .hip files restated in Python) every body, refusal and second sweep of the table is selected by some case, and every
alignment condition of a 16-byte body is violated alone by some case; the guarded-buffer helpers do what they say; and the host
statements agree with torch.nn.functional / autograd in fp64 where one exists."""
import pytest
import torch
import torch.nn.functional as F

import row_layout_cases as rc


def test_every_body_and_sweep_is_selected():
    seen = {}
    for entry, cid, dims, lds, offs in rc.flat():
        seen.setdefault((entry,) + rc.branch_of(entry, dims, lds, offs), []).append(cid)
    missing = [r for r in rc.REQUIRED if r not in seen]
    assert not missing, 'no case selects %s' % missing
    assert {e for e, _, _ in rc.REQUIRED} == {c['entry'] for c in rc.CASES}
    for key in sorted(seen):
        print('%-18s %-40s sweep %-5s %3d layouts, e.g. %s' % (key + (len(seen[key]), seen[key][0])))


def test_every_vector_condition_is_violated_alone():
    alone = {}
    for entry, cid, dims, lds, offs in rc.flat():
        if entry in rc.ALONE:
            bad = rc.violations(entry, dims, lds, offs)
            if len(bad) == 1:
                alone.setdefault((entry, next(iter(bad))), cid)
    missing = [(e, c) for e, conds in rc.ALONE.items() for c in conds if (e, c) not in alone]
    assert not missing, 'never violated alone: %s' % missing
    # ... and a violated condition never selects the vector body
    for entry, cid, dims, lds, offs in rc.flat():
        if entry in rc.ALONE and rc.violations(entry, dims, lds, offs):
            body = rc.branch_of(entry, dims, lds, offs)[0]
            assert 'vec' not in body and '<4>' not in body and body not in ('news_xin_kernel', 'fill_pad_rows_kernel', 'mean_pool_flat_kernel') \
                and not body.startswith('gate_mul_kernel'), (cid, body)


def test_the_four_placements_of_a_case_share_its_operands():
    """A case's layouts differ in leading dimensions and offsets only; ids are unique; every leading dimension holds its row."""
    ids = [(c['entry'], c['id']) for c in rc.CASES]
    assert len(ids) == len(set(ids))
    for c in rc.CASES:
        names = [n for n, _, _ in c['layouts']]
        assert len(names) == len(set(names)), c['id']
        w = c['dims'].get(rc._WIDTH.get(c['entry'], 'cols'), 0)
        for _, lds, offs in c['layouts']:
            assert all(ld >= w for ld in lds.values()) and all(o >= 0 for o in offs.values()), c['id']


@pytest.mark.parametrize('ld,off', [(None, 0), (9, 0), (6, 0), (9, 1)])
def test_placed_and_outside_untouched(ld, off):
    t = rc.rnd(7, 5, seed=1)
    v, buf = rc.placed(t, ld, off, device='cpu')
    assert buf.dtype == torch.int32 and torch.equal(v, t) and v.stride() == (5 if ld is None else ld, 1)
    assert (v.data_ptr() - buf.data_ptr()) == 4 * off
    assert rc.outside_untouched(buf, v)
    n_out = buf.numel() - t.numel()
    assert int((buf == rc.SENTINEL).sum()) == n_out                          # the view covers exactly rows * cols words
    v.mul_(2.0)
    assert rc.outside_untouched(buf, v)                                      # writes inside the view are not its business
    for word in ([off - 1] if off else []) + [off + 5 if (ld or 5) > 5 else buf.numel() - 1, buf.numel() - 1]:
        saved = int(buf[word])
        buf[word] = 0
        assert not rc.outside_untouched(buf, v), word                        # one word outside: seen
        buf[word] = saved
    o, obuf = rc.placed((7, 5), ld, off, device='cpu')
    assert rc.is_sentinel(o) and bool((obuf == rc.SENTINEL).all())


def test_host_statements_against_torch():
    g = torch.Generator().manual_seed(3)
    # embed_pe: F.embedding + the positional rows
    table, pe, ids = rc.mag(50, 12, seed=1), rc.mag(8, 12, seed=2) * 0.1, rc.ints(40, 50, seed=3)
    want = F.embedding(ids.long(), table.double()) + pe.double().repeat(5, 1)
    assert torch.equal(rc.embed_pe_ref(table, ids, pe, 8).double(), want.float().double())
    assert torch.equal(rc.embed_pe_ref(table, ids, None, 0), table[ids.long()])
    # mean_pool: F.avg_pool1d over the tokens
    x = rc.grid64(6 * 5, 12, seed=4)
    want = F.avg_pool1d(x.double().view(6, 5, 12).transpose(1, 2), 5).squeeze(-1)
    assert torch.allclose(rc.mean_pool_ref(x, 6, 5), want, rtol=0, atol=1e-15)
    # grid64: sums of 300 values are exact in fp32 in any order
    y = rc.grid64(300, 64, seed=5)
    assert torch.equal(y.sum(0).double(), y.double().sum(0)) and torch.equal(y.flip(0).cumsum(0)[-1].double(), y.double().sum(0))
    # news_xin against two mean_pools and two gathers
    cap, tb, bb = 5, rc.grid64(5 * 4, 8, seed=6), rc.grid64(5 * 2, 8, seed=7)
    tr, br = rc.ints(cap, cap, seed=8), rc.ints(cap, cap, seed=9)
    want = torch.cat([rc.mean_pool_ref(tb, cap, 4)[tr.long()], rc.mean_pool_ref(bb, cap, 2)[br.long()]])
    assert torch.equal(rc.news_xin_ref(tb, 4, bb, 2, tr, br, cap), want)
    # fuse_rows: torch.lerp states gate * a + (1 - gate) * b
    a, b, gate = rc.mag(9, 7, seed=10), rc.mag(9, 7, seed=11), torch.rand(9, 7, generator=g)
    assert torch.allclose(rc.fuse_rows_ref(a, b, gate), torch.lerp(b.double(), a.double(), gate.double()), rtol=1e-14, atol=0)
    assert torch.allclose(rc.fuse_rows_gated_f32(a, b, gate).double(), rc.fuse_rows_ref(a, b, gate), rtol=0, atol=4e-7)   # four roundings of terms <= 1.5
    assert torch.equal(rc.fuse_rows_ref(a, b), a + b)
    # pad_heads: F.pad of the head axis
    src = rc.mag(6 * 5, 7, seed=12)
    assert torch.equal(rc.pad_heads_ref(src, 6, 5, 8), F.pad(src.view(6, 5, 7), (0, 0, 0, 3)).reshape(48, 7))
    # gate_mul
    xg, gg = rc.mag(12, 8, seed=13), rc.rnd(12, 8, seed=14, scale=4.0)
    assert torch.allclose(rc.gate_mul_ref(xg, gg), xg.double() * F.sigmoid(gg.double()), rtol=1e-15, atol=0)
    g3 = rc.mag(3, 8, seed=15)
    want = xg.double() * g3.double()[torch.arange(12) // 4] * 0.37
    assert torch.allclose(rc.gate_mul_ref(xg, g3, div=4, scale=0.37, sigmoid=False).double(), want, rtol=2e-7, atol=0)
    # relu_bwd_: autograd of relu, times the scale
    h = rc.rnd(9, 7, seed=16).requires_grad_()
    dh = rc.mag(9, 7, seed=17)
    F.relu(h).backward(dh)
    assert torch.equal(rc.relu_bwd_ref(dh, h.detach(), 1.0), h.grad)
    assert torch.allclose(rc.relu_bwd_ref(dh, h.detach(), 0.37).double(), h.grad.double() * 0.37, rtol=2e-7, atol=0)
    # fill_pad_rows
    ids0 = torch.tensor([0, 3, 0, 0, 5, 0], dtype=torch.int32)
    srcf, dstf = rc.mag(2, 4, seed=18), rc.mag(6, 4, seed=19)
    got = rc.fill_pad_rows_ref(ids0, srcf, dstf, 2)
    assert torch.equal(got[[0, 2, 3, 5]], srcf[[0, 0, 1, 1]]) and torch.equal(got[[1, 4]], dstf[[1, 4]])
    # colsum, row_scale, gather
    assert torch.equal(rc.colsum_ref(a), a.double().sum(0)) and torch.equal(rc.colsum_ref(a, b[0]), a.double().sum(0) + b[0].double())
    assert torch.equal(rc.row_scale_ref(a, b[:, 0]), a * b[:, :1])
    assert torch.equal(rc.gather_ref(table, ids), F.embedding(ids.long(), table))


def test_layernorm_bwd_statement_spreads_dy_over_div_rows():
    M, E, div = 35, 12, 16
    z, gamma, beta, dy = rc.layernorm_bwd_inputs(M, E, div)
    y, rstd, dz, dg, db, dzsum = rc.layernorm_bwd_ref(z, gamma, beta, dy, div)
    zd = z.double().requires_grad_()
    out = F.layer_norm(zd, (E,), gamma.double(), beta.double(), 1e-5)
    full = torch.stack([dy[r // div].double() / div for r in range(M)])
    out.backward(full)
    assert torch.allclose(dz, zd.grad, rtol=1e-12, atol=1e-15) and torch.allclose(dzsum, zd.grad.sum(0), rtol=1e-12, atol=1e-15)
    assert torch.allclose(db, full.sum(0), rtol=1e-12, atol=1e-15)
    assert torch.allclose(y, out.detach(), rtol=0, atol=1e-15)


def test_branch_of_thresholds():
    """The caps, exactly at and one past the edge."""
    e = lambda rows, dim: rc.branch_of('embed_pe', dict(rows=rows, dim=dim, pe=True), {}, {})
    assert e(8192 * 256 // 75 + 0, 300) == ('embed_pe_kernel<4>', False) and e(8192 * 256 // 75 + 1, 300) == ('embed_pe_kernel<4>', True)
    f = lambda rows: rc.branch_of('fuse_rows', dict(rows=rows, cols=256), {}, {})[1]
    assert not f(2048) and f(2049)
    m = lambda n_seq, S, dim, live=None, **k: rc.branch_of('mean_pool', dict(n_seq=n_seq, S=S, dim=dim, live=live), k.get('lds', {}), k.get('offs', {}))[0]
    assert m(511, 16, 300) == 'mean_pool_vec4_kernel' and m(512, 16, 300) == 'mean_pool_flat_kernel' and m(512, 17, 300) == 'mean_pool_vec4_kernel'
    assert m(3, 2, 1024) == 'mean_pool_vec4_kernel' and m(3, 2, 1028) == 'mean_pool_kernel' and m(3, 2, 300, offs={'x': 1}) == 'mean_pool_kernel'
    assert m(3, 16, 300, live=2) == 'mean_pool_flat_kernel' and m(3, 17, 300, live=2) == 'refused'
    ln = lambda M, E, **k: rc.branch_of('layernorm_bwd', dict(M=M, E=E), k.get('lds', {}), {})
    assert ln(768 * 16, 128) == ('layernorm_bwd_vec_kernel<2>', False) and ln(768 * 16 + 1, 132) == ('layernorm_bwd_vec_kernel<5>', True)
    assert ln(96, 320)[0] == 'layernorm_bwd_vec_kernel<5>' and ln(96, 324)[0] == 'layernorm_bwd_vec_kernel<8>' and ln(96, 513)[0] == 'refused'
    assert ln(96, 300, lds={'dz': 301})[0] == 'layernorm_bwd_kernel<5>' and ln(96, 129)[0] == 'layernorm_bwd_kernel<5>'
