"""The fp32 token-attention backward on the GPU, one case of attn_bwd_route_cases.py per family and per pass of
lime_token_attention_bwd_plan_f32 and one on each side of each routing threshold: the plan names the expected family and pass,
ops.token_attention_bwd agrees with fp64 autograd of a plain softmax attention on the same inputs (key mask as the -1e9 fill, dropout
mask as dropout_cases.py states it), the pad columns of dq / dk / dv are exact zeros, and between them the cases reach every family
and every pass of the plan.

The bound is the one each family's own test holds it to, imported from there: 2e-4 against fp64 autograd everywhere -- the
close(..., tol=2e-4) of test_backward_gpu._attention_bwd_case, which dropout_cases.BWD names and test_dropout_kernels_gpu.py uses,
and test_wide_heads_gpu.BWD for the wide heads.  All cases run once, in a module fixture (a few milliseconds each)."""
import pytest
import torch

import attn_bwd_route_cases as arc
import dropout_cases as dc
from helpers import rel_err
from test_wide_heads_gpu import BWD as WIDE_BWD

pytestmark = pytest.mark.gpu

# (case, split mode, the family it must take, the pass in front of it)
PICKS = (
    # one pass: the three buckets of the fp32 kernel, padding rows in each; 64 | 68 and 128 | 129 with the split product on ...
    ('s20', 1, 'one_pass', None), ('s32', 1, 'one_pass', None), ('s33', 1, 'one_pass', None), ('s64', 1, 'one_pass', None),
    ('s65', 1, 'one_pass', None), ('s68', 1, 'sp', None), ('s96', 1, 'sp', None), ('s128', 1, 'sp', None), ('s129', 1, 'long_sp', 'split'),
    # ... and off
    ('s64', 0, 'one_pass', None), ('s68', 0, 'one_pass', None), ('s128', 0, 'one_pass', None), ('s129', 0, 'long', 'fp32'),
    # what keeps S = 96 off the split product: a key mask, unpadded heads, an odd head, misaligned q / k / v or dq / dk / dv, leading
    # dimensions that are no multiples of 4, dout off the 8-byte boundary
    ('s96_mask', 1, 'one_pass', None), ('s96_h20', 1, 'one_pass', None), ('s96_h15', 1, 'one_pass', None), ('s96_off', 1, 'one_pass', None),
    ('s96_doff', 1, 'one_pass', None), ('s96_ld1', 1, 'one_pass', None), ('s96_dld1', 1, 'one_pass', None),
    ('s96_dout_off', 1, 'one_pass', None),
    # dropout on every arithmetic; a key mask in the smallest and the largest bucket
    ('s32_p1', 1, 'one_pass', None), ('s96_p1', 1, 'sp', None), ('s96_p1', 0, 'one_pass', None), ('s160_p1', 1, 'long_sp', 'split'),
    ('s160_p1', 0, 'long', 'fp32'), ('s32_mask', 0, 'one_pass', None), ('s128_mask', 1, 'one_pass', None),
    # key blocks: two, and four; padded and unpadded heads; behind the statistics pass or, with the forward's lse, delta alone
    ('s160', 1, 'long_sp', 'split'), ('s160_h20', 0, 'long', 'fp32'), ('s512', 1, 'long_sp', 'split'), ('s512_h20', 0, 'long', 'fp32'),
    ('s160_lse', 1, 'long_sp', 'delta'), ('s160_lse', 0, 'long', 'delta'), ('s256_h20_lse', 1, 'long_sp', 'delta'),
    # wide heads: NK = 3, 4, 8; more than one 64-row block; mask, dropout, and the lse entry
    ('s64_w36', 1, 'wide', None), ('s64_w64', 0, 'wide', None), ('s64_w128', 1, 'wide', None), ('s160_w36', 1, 'wide', None),
    ('s64_w64_mask', 1, 'wide', None), ('s64_w64_p1', 1, 'wide', None), ('s160_w36_lse', 1, 'wide', None),
)


def reference(c, kw):
    """(out, dqkv [tok, 3, n_head, head_dim]) in fp64 from the tensors the call is given."""
    n_seq, S, h, hd = c['n_seq'], c['S'], c['n_head'], c['hd']
    vals = torch.stack([kw[n].cpu() for n in 'qkv'], dim=1).reshape(n_seq * S, 3, h, -1)[..., :hd]
    mask = kw['key_mask'].cpu().view(n_seq, S) if kw.get('key_mask') is not None else None
    m = dc.multiplier(c['p'], arc.DROPOUT_SEED, arc.DROPOUT_SITE, (n_seq, h, S, S)) if c['p'] else None
    return dc.attn_bwd_ref(vals, kw['dout'].cpu(), n_seq, S, h, hd, kw['scale'], mask=mask, m=m)


@pytest.fixture(scope='module')
def runs():
    """{(case id, mode): what the call did}, every pick run once."""
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from lime_cikm25_amd import _lib, ops
    lib = _lib.load()
    by_id = {c['id']: c for c in arc.CASES}
    start = lib.lime_set_split_gemm(-1)
    out = {}
    try:
        for cid, mode, _, _ in PICKS:
            c = by_id[cid]
            fn, kw = arc.build(c)
            want_out, want = reference(c, kw)
            if kw.get('out') is not None:                # the output of the forward this call is the backward of (dropout included)
                kw['out'] = want_out.float().cuda()
            lib.lime_set_split_gemm(mode)
            plan = ops.token_attention_bwd_plan(**kw)
            got = getattr(ops, fn)(**kw)
            torch.cuda.synchronize()
            got = got.cpu().reshape(c['n_seq'] * c['S'], 3, c['n_head'], c['hs'])
            out[(cid, mode)] = dict(plan, err=rel_err(got[..., :c['hd']].numpy(), want.numpy()), finite=bool(torch.isfinite(got).all()),
                                    pads_zero=bool((got[..., c['hd']:] == 0).all()))
    finally:
        lib.lime_set_split_gemm(start)
    return out


@pytest.mark.parametrize('cid,mode,family,stats_pass', PICKS, ids=['%s@%d' % p[:2] for p in PICKS])
def test_the_route_computes_the_gradients(runs, cid, mode, family, stats_pass):
    r = runs[(cid, mode)]
    tol = WIDE_BWD if family == 'wide' else dc.BWD
    print('%s@%d %s: rel err %.3e (bound %.0e)' % (cid, mode, '; '.join(r['kernels']), r['err'], tol))
    assert (r['family'], r['stats_pass']) == (family, stats_pass)
    assert r['finite'] and r['err'] < tol
    assert r['pads_zero'], 'pad columns must be exact zeros'


def test_the_picks_reach_every_family_and_pass(runs):
    from lime_cikm25_amd import _lib
    assert {r['family'] for r in runs.values()} == {f for f in _lib.BWD_ATTN_FAMILY.values() if f is not None}
    assert {r['stats_pass'] for r in runs.values()} == set(_lib.BWD_ATTN_PASS.values())
