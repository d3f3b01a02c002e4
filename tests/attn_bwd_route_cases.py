"""The fp32 token-attention backward routing cases shared by tools/attn_routes.py --bwd (which runs each of them on the GPU and records
the kernels that ran) and tests/test_attn_bwd_plan_cpu.py / test_attn_bwd_plan_gpu.py (which ask lime_token_attention_bwd_plan_f32 for
the same decisions): the backward sibling of attn_route_cases.py, whose modes and sequence / head counts it shares.  Pure data, but for
build(), which makes a case's device tensors.  The table reaches both sides of every rule of the routing.

A case is a dict: id, S, hd (head_dim), hs (head_stride), n_seq, n_head, and
  mask      a key mask
  p         dropout probability
  off       q / k / v start one float past a 16-byte boundary
  ld        the leading dimension of q / k / v: 'row' the three operands side by side, 'row1' one float more (no multiple of 4)
  doff, dld the same two for the dqkv buffer
  dout_off  dout starts one float past a 16-byte boundary (a 4-byte boundary, not an 8-byte one)
  out       the forward's output is handed over (default: where S > 128)
  lse       the forward's log-sum-exp is handed over
"""
import math
import zlib

from attn_route_cases import MODES, N_SEQ, N_HEAD, DROPOUT_SEED, DROPOUT_SITE  # noqa: F401  (MODES: for the table's users)


def _case(cid, S, hd=20, hs=32, n_seq=N_SEQ, n_head=N_HEAD, mask=False, p=None, off=False, ld='row', doff=False, dld='row',
          dout_off=False, out=None, lse=False):
    return dict(id=cid, S=S, hd=hd, hs=hs, n_seq=n_seq, n_head=n_head, mask=mask, p=p, off=off, ld=ld, doff=doff, dld=dld,
                dout_off=dout_off, out=S > 128 if out is None else out, lse=lse)


def _cases():
    c = []
    add = lambda *a, **k: c.append(_case(*a, **k))
    # one pass, heads padded to 32 columns: the 32 / 64 / 128 buckets of token_attn_bwd_kernel; under the split product 64 < S <= 128 with
    # S % 4 == 0 is attn_bwd_sp_kernel (FULL at 128 only)
    for S in (20, 32, 33, 64, 65, 68, 96, 128):
        add('s%d' % S, S)
    add('s96_h32', 96, hd=32)
    # what keeps S = 96 off the split product
    add('s96_h20', 96, hs=20)
    add('s96_h15', 96, hd=15)                                  # an odd head, and an odd ldo
    add('s96_mask', 96, mask=True)
    add('s96_off', 96, off=True)
    add('s96_ld1', 96, ld='row1')
    add('s96_doff', 96, doff=True)
    add('s96_dld1', 96, dld='row1')
    add('s96_dout_off', 96, dout_off=True)
    # dropout on the probabilities: the fp32 and the split one-pass kernels, the blocked kernels
    add('s32_p1', 32, p=0.1)
    add('s96_p1', 96, p=0.1)
    add('s160_p1', 160, p=0.1)
    add('s32_mask', 32, mask=True)
    add('s128_mask', 128, mask=True)
    add('s160_mask', 160, mask=True)                           # refused
    # key blocks: the statistics pass (or delta alone behind a forward that kept its lse), the blocked kernel, the dq reduction
    for S in (129, 160, 256, 512):
        for hs in (32, 20):
            tag = 's%d' % S + ('' if hs == 32 else '_h20')
            add(tag, S, hs=hs)
            add(tag + '_lse', S, hs=hs, lse=True)
    add('s160_noout', 160, out=False)                          # the wrapper refuses
    add('s160_lse_nh65', 160, n_seq=1, n_head=65, lse=True)    # refused
    add('s160_lse_nh40_h32', 160, hd=32, n_seq=1, n_head=40, lse=True)   # refused: n_head * head_dim > 1024
    add('s160_nh40_h32', 160, hd=32, n_seq=1, n_head=40)       # the limit is the lse entry's alone
    # wide heads: NK = ceil(head_dim / 16) = 3 .. 8
    for hd in (36, 64, 128):
        add('s64_w%d' % hd, 64, hd=hd, hs=hd)
    add('s160_w36', 160, hd=36, hs=36)
    add('s64_w64_mask', 64, hd=64, hs=64, mask=True)
    add('s64_w64_p1', 64, hd=64, hs=64, p=0.1)
    add('s160_w36_lse', 160, hd=36, hs=36, lse=True)           # the lse entry, which runs the wide kernels
    add('s160_w36_lse_noout', 160, hd=36, hs=36, lse=True, out=False)    # the plain entry
    add('s64_w34', 64, hd=34, hs=36)                           # refused: head_dim % 4
    add('s64_w132', 64, hd=132, hs=132)                        # refused
    add('s513_w64', 513, hd=64, hs=64)                         # refused
    add('s64_w64_off', 64, hd=64, hs=64, off=True)             # refused
    add('s64_w64_doff', 64, hd=64, hs=64, doff=True)           # refused
    add('s64_w36_ld1', 64, hd=36, hs=36, ld='row1')            # refused
    add('s64_w36_dld1', 64, hd=36, hs=36, dld='row1')          # refused
    # refused narrow calls
    add('s513', 513)
    add('hs_lt_hd', 32, hd=20, hs=10)
    add('s64_hs36', 64, hd=20, hs=36)
    add('bad_p', 64, p=1.0)
    add('bad_p_s513', 513, p=1.0)                              # the probability before the shape
    add('bad_p_w64', 64, hd=64, hs=64, p=1.0)
    # no sequences.  torch gives a tensor without elements a NULL address, so through the ops wrapper these record the NULL refusal;
    # tests/test_attn_bwd_plan_cpu.py states the library's own answer over made-up addresses
    add('empty', 64, n_seq=0)
    add('empty_s160', 160, n_seq=0)
    add('empty_w64', 64, hd=64, hs=64, n_seq=0)
    ids = [x['id'] for x in c]
    assert len(set(ids)) == len(ids)
    return c


CASES = _cases()


def case_ids():
    return ['%s@%d' % (c['id'], mode) for c in CASES for mode in MODES]


def layout(c):
    """(columns of one q / k / v operand, their leading dimension, q's float offset, dqkv's leading dimension and float offset, dout's
    leading dimension and float offset): what build() lays out and what the CPU test states over made-up addresses."""
    W = c['n_head'] * c['hs']
    pitch = {'row': 3 * W, 'row1': 3 * W + 1}
    return W, pitch[c['ld']], int(c['off']), pitch[c['dld']], int(c['doff']), c['n_head'] * c['hd'], int(c['dout_off'])


def build(c):
    """(name of the ops wrapper, its keyword arguments) for case c: real device tensors, misaligned where the case says so.  Padding
    columns of a head (head_stride > head_dim) hold zeros, as every padded-layout kernel expects.  ``out`` / ``lse`` are those of the
    plain (no dropout) forward, computed on the CPU."""
    import torch
    gen = torch.Generator().manual_seed(zlib.crc32(c['id'].encode()))
    S, hd, hs, n_seq, nh = c['S'], c['hd'], c['hs'], c['n_seq'], c['n_head']
    W, ld, start, ldd, dstart, ldo, ostart = layout(c)
    n_tok = n_seq * S
    scale = hd ** -0.5

    def strided(rows, cols, pitch, first, val=None):
        buf = torch.zeros(rows * pitch + 8, dtype=torch.float32, device='cuda')
        view = buf.as_strided((rows, cols), (pitch, 1), first)
        if val is not None:
            view.copy_(val)
        return view

    val = torch.randn(n_tok, 3 * nh, hs, generator=gen)
    if hs > hd:
        val[:, :, hd:] = 0
    qkv = strided(n_tok, 3 * W, ld, start, val.reshape(n_tok, 3 * W))
    dout = strided(n_tok, nh * hd, ldo, ostart, torch.randn(n_tok, nh * hd, generator=gen))
    kw = dict(q=qkv[:, :W], k=qkv[:, W:2 * W], v=qkv[:, 2 * W:], dout=dout, n_seq=n_seq, S=S, n_head=nh, head_dim=hd, scale=scale,
              head_stride=hs, dqkv=strided(n_tok, 3 * W, ldd, dstart))
    mask = None
    if c['mask']:
        mask = torch.rand(n_seq, S, generator=gen) < 0.7
        mask[:, :1] = True
        kw['key_mask'] = mask.reshape(-1).cuda()
    if c['p'] is not None:
        kw['dropout'] = (c['p'], DROPOUT_SEED, DROPOUT_SITE)
    if c['out'] or c['lse']:
        q, k, v = (val[:, i * nh:(i + 1) * nh].reshape(n_seq, S, nh, hs).permute(0, 2, 1, 3) for i in range(3))
        s = scale * (q @ k.transpose(-1, -2))
        if mask is not None:
            s = s.masked_fill(~mask[:, None, None, :], -1e9)
        if c['out']:
            o = torch.softmax(s, -1) @ v[..., :hd]
            kw['out'] = o.permute(0, 2, 1, 3).reshape(n_tok, nh * hd).contiguous().cuda()
        if c['lse']:                                            # log2 domain, [tokens, n_head]
            kw['lse'] = (torch.logsumexp(s, -1) * math.log2(math.e)).permute(0, 2, 1).reshape(-1).contiguous().cuda()
    return 'token_attention_bwd', kw
