"""The fp32 token-attention forward on the GPU, one case of attn_route_cases.py per family of lime_token_attention_plan_f32 and one on
each side of each routing threshold: the ops call succeeds, its output agrees with a plain fp64 softmax attention of the same inputs
(key mask as the -1e9 fill, dropout mask as dropout_cases.py states it), rows of sequences beyond the device-side count stay as they
were, and between them the cases reach every family of the plan.

Bounds are the ones each family's own test holds it to, imported from there: the exact-fp32 MFMA kernel test_kernels_gpu.TIGHT, the
split-product kernels test_split_gemm_gpu.TIGHT, the wide heads test_wide_heads_gpu.TIGHT (all 2e-5), every dropout-drawing call
dropout_cases.TIGHT (5e-5, test_dropout_kernels_gpu.py); the log-sum-exp output the 1e-5 of test_wide_heads_gpu.test_forward.
All cases run once, in a module fixture (a few milliseconds each)."""
import pytest
import torch

import attn_route_cases as arc
import dropout_cases as dc
from helpers import rel_err
from test_kernels_gpu import TIGHT as MFMA_TIGHT
from test_split_gemm_gpu import TIGHT as SPLIT_TIGHT
from test_wide_heads_gpu import TIGHT as WIDE_TIGHT

pytestmark = pytest.mark.gpu

LSE_TOL = 1e-5
TOL = {'sp': SPLIT_TIGHT, 'sp_long': SPLIT_TIGHT, 'sp_vocab': SPLIT_TIGHT, 'mfma': MFMA_TIGHT, 'wide': WIDE_TIGHT}

# (case, split mode, the family it must take)
PICKS = (
    # the one-pass split product at its three lengths; the same calls on the fp32 MFMA with the split product off
    ('plain_s32', 1, 'sp'), ('plain_s64', 1, 'sp'), ('plain_s128', 1, 'sp'), ('plain_s64', 0, 'mfma'),
    # lengths the split product does not take: NT = 1 (padding keys), 3, 8 (not FAST)
    ('plain_s20', 1, 'mfma'), ('plain_s96', 1, 'mfma'), ('plain_s160', 1, 'mfma'),
    # key blocks: 256 and 512, on either arithmetic
    ('plain_s256', 1, 'sp_long'), ('plain_s512', 1, 'sp_long'), ('plain_s256', 0, 'mfma'), ('plain_s512', 0, 'mfma'),
    # what keeps a call off the split product and off FAST: unpadded heads, an odd head, a key mask, misaligned q, a leading dimension
    # that is no multiple of 4
    ('plain_s128_h20', 1, 'mfma'), ('plain_s32_h15', 1, 'mfma'), ('plain_s64_mask', 1, 'mfma'), ('plain_s64_off', 1, 'mfma'),
    ('plain_s64_ld1', 1, 'mfma'), ('plain_s256_off', 1, 'mfma'),
    # a device-side sequence count
    ('count_s64', 1, 'sp'), ('count_s64_mask', 1, 'mfma'), ('count_s128', 0, 'mfma'), ('count_s256', 1, 'sp_long'),
    # the log-sum-exp output: the split product writes it from 256 on only
    ('lse_s128', 1, 'mfma'), ('lse_s256', 1, 'sp_long'), ('lse_s256', 0, 'mfma'), ('lse_s64_w36', 1, 'wide'),
    # the row map
    ('rows_s64', 1, 'sp'), ('rows_s64', 0, 'mfma'), ('rows_s96', 1, 'mfma'), ('rows_s256', 1, 'sp_long'), ('rows_s64_nodev', 1, 'sp'),
    # the per-vocabulary product
    ('vocab_s32', 1, 'sp_vocab'), ('vocab_s64', 1, 'sp_vocab'), ('vocab_s128', 1, 'sp_vocab'),
    # wide heads: NK = 3, 4, 8; more than one 64-row block; mask and count
    ('plain_s64_w36', 1, 'wide'), ('plain_s64_w64', 0, 'wide'), ('plain_s64_w128', 1, 'wide'), ('plain_s160_w36', 1, 'wide'),
    ('count_s64_w64_mask', 1, 'wide'), ('drop_p1_s64_w64', 1, 'wide'),
    # dropout: the split product, the one-pass kernel's three buckets (padded and unpadded heads), the blocked kernel behind either
    # statistics pass; p = 0 draws no mask
    ('drop_p1_s64', 1, 'sp'), ('drop_p1_s64', 0, 'dropout'), ('drop_p1_s32_h20', 1, 'dropout'), ('drop_p1_s128_h20', 1, 'dropout'),
    ('drop_p1_s96', 1, 'dropout'), ('drop_p0_s128', 0, 'dropout'), ('drop_p0_s128', 1, 'sp'), ('drop_p1_s64_off', 1, 'dropout'),
    ('drop_p1_s256', 1, 'dropout_long'), ('drop_p1_s256', 0, 'dropout_long'), ('drop_p1_s160_h20', 1, 'dropout_long'),
)


def reference(c, kw):
    """(out, log2-domain lse [n_seq, n_head, S]) in fp64 from the tensors the call was given."""
    n_seq, S, h, hd = c['n_seq'], c['S'], arc.N_HEAD, c['hd']
    n_tok = n_seq * S
    if c['form'] == 'vocab':                   # one fp32 add per element, as the kernel makes it
        rows = kw['qkv_vocab'].cpu()[kw['ids'].cpu().long()[:n_tok]] + kw['pos_rows'].cpu()[:S].repeat(n_seq, 1)
        ops3 = rows.view(n_tok, 3, h, 32)
    else:
        ops3 = torch.stack([kw[n].cpu() for n in 'qkv'], dim=1)
        if c['form'] == 'rows':
            ops3 = ops3[kw['row_map'].cpu().long()[:n_tok]]
        ops3 = ops3.reshape(n_tok, 3, h, -1)
    vals = ops3[..., :hd].double()
    mask = kw['key_mask'].cpu().view(n_seq, S) if kw.get('key_mask') is not None else None
    m = dc.multiplier(c['p'], arc.DROPOUT_SEED, arc.DROPOUT_SITE, (n_seq, h, S, S)) if c['p'] > 0 else None
    return dc.attn_ref(vals, n_seq, S, h, hd, kw['scale'], mask=mask, m=m)


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
        for cid, mode, _ in PICKS:
            c = by_id[cid]
            fn, kw = arc.build(c)
            lib.lime_set_split_gemm(mode)
            plan = ops.token_attention_plan(c['form'], **kw)
            got = getattr(ops, fn)(**kw)
            torch.cuda.synchronize()
            assert got is not None, cid
            want, want_lse = reference(c, kw)
            live = (arc.N_DEV if c['dev'] else c['n_seq']) * c['S']
            r = dict(family=plan['family'], kernels=plan['kernels'], err=rel_err(got[:live].cpu().numpy(), want[:live].numpy()),
                     untouched=bool((got[live:] == 0).all()), finite=bool(torch.isfinite(got).all()))
            if kw.get('lse') is not None:
                r['lse_err'] = rel_err(kw['lse'].cpu().view(c['n_seq'], c['S'], arc.N_HEAD).permute(0, 2, 1).numpy(), want_lse.numpy())
            out[(cid, mode)] = r
    finally:
        lib.lime_set_split_gemm(start)
    return out


@pytest.mark.parametrize('cid,mode,family', PICKS, ids=['%s@%d' % p[:2] for p in PICKS])
def test_the_route_computes_attention(runs, cid, mode, family):
    r = runs[(cid, mode)]
    c = {c['id']: c for c in arc.CASES}[cid]
    tol = dc.TIGHT if c['form'] == 'dropout' else TOL[family]
    print('%s@%d %s: rel err %.3e (bound %.0e)%s' % (cid, mode, '; '.join(r['kernels']), r['err'], tol,
                                                    ', lse %.3e' % r['lse_err'] if 'lse_err' in r else ''))
    assert r['family'] == family
    assert r['finite'] and r['err'] < tol
    assert r['untouched'], 'rows beyond the device-side count were written'
    if 'lse_err' in r:
        assert r['lse_err'] < LSE_TOL


def test_the_picks_reach_every_family(runs):
    from lime_cikm25_amd import _lib
    assert {r['family'] for r in runs.values()} == {f for f in _lib.ATTN_FAMILY.values() if f is not None}
    assert any(c['dev'] for c in arc.CASES if any(c['id'] == p[0] for p in PICKS))
