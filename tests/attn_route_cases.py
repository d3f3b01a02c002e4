"""The fp32 token-attention forward routing cases shared by tools/attn_routes.py (which runs each of them on the GPU and records the
kernels that ran) and tests/test_attn_plan_cpu.py / test_attn_plan_gpu.py (which ask lime_token_attention_plan_f32 for the same
decisions).  Pure data, but for build(), which makes a case's device tensors.  Every case is tiny: N_SEQ sequences x N_HEAD heads
is 9 (sequence, head) pairs, so the 4-per-group and 2-per-group packing of the persistent kernels has a partial last group; where a
case has a device-side sequence count it is N_DEV, so the last sequence's output rows must stay as they were.  The table reaches
both sides of every rule of the routing; every case is run under each split mode of MODES.

A case is a dict: id, form, S, hd (head_dim), hs (head_stride), n_seq, and
  form   'plain' | 'count' (device-side sequence count) | 'lse' | 'rows' (row map) | 'vocab' | 'dropout'
  mask   a key mask (plain / count)
  dev    a device-side sequence count (count always; rows / vocab optionally)
  p      dropout probability (dropout)
  off    q / k / v (vocab: the product and the positional rows) start one float past a 16-byte boundary
  ld     the leading dimension of q / k / v: 'row' the three operands side by side, 'row1' one float more (no multiple of 4),
         'huge' (vocab) past the 1 << 21 floats its 32-bit offsets reach
"""
import zlib

MODES = (0, 1, 5)                  # lime_set_split_gemm(): only bit 0 (the split product) matters to attention
N_SEQ, N_HEAD, N_DEV = 3, 3, 2
VOCAB = 50                         # rows of the vocab form's product
DROPOUT_SEED, DROPOUT_SITE = 1234, 7
HUGE_LD = (1 << 21) + 4
FORMS = ('plain', 'count', 'lse', 'rows', 'vocab', 'dropout')
CALLS = {'plain': 'token_attention', 'count': 'token_attention', 'lse': 'token_attention', 'rows': 'token_attention_rows',
         'vocab': 'token_attention_vocab', 'dropout': 'token_attention_dropout'}


def _case(cid, form, S, hd=20, hs=32, n_seq=N_SEQ, mask=False, dev=None, p=0.0, off=False, ld='row'):
    dev = (form == 'count') if dev is None else dev
    return dict(id=cid, form=form, S=S, hd=hd, hs=hs, n_seq=n_seq, mask=mask, dev=dev, p=p, off=off, ld=ld)


def _cases():
    c = []
    add = lambda *a, **k: c.append(_case(*a, **k))
    # plain, heads padded to 32 columns: the split-product kernels at 32 / 64 / 128 (one pass) and 256 / 512 (key blocks), the fp32
    # MFMA kernel at every other length (NT = 1, 3, 8) and everywhere under mode 0; S = 513 is refused
    for S in (20, 32, 64, 96, 128, 160, 256, 512, 513):
        add('plain_s%d' % S, 'plain', S)
    # unpadded heads: never the split product, never FAST
    for S in (20, 32, 128, 160, 512):
        add('plain_s%d_h20' % S, 'plain', S, hs=20)
    add('plain_s32_h15', 'plain', 32, hd=15, hs=15)            # no 8-byte loads
    add('plain_s64_h32', 'plain', 64, hd=32, hs=32)
    add('plain_s64_mask', 'plain', 64, mask=True)
    add('plain_s64_off', 'plain', 64, off=True)                # the general loaders
    add('plain_s64_ld1', 'plain', 64, ld='row1')
    add('plain_s256_off', 'plain', 256, off=True)
    add('plain_hs_lt_hd', 'plain', 32, hd=20, hs=10)           # refused
    # wide heads: NK = ceil(head_dim / 16) = 3 .. 8
    for hd in (36, 64, 128):
        add('plain_s64_w%d' % hd, 'plain', 64, hd=hd, hs=hd)
    add('plain_s160_w36', 'plain', 160, hd=36, hs=36)
    add('plain_s64_w34', 'plain', 64, hd=34, hs=36)            # refused: head_dim % 4
    add('plain_s64_w132', 'plain', 64, hd=132, hs=132)         # refused
    add('plain_s513_w64', 'plain', 513, hd=64, hs=64)          # refused
    add('plain_s64_w64_off', 'plain', 64, hd=64, hs=64, off=True)       # refused
    add('plain_s64_w36_ld1', 'plain', 64, hd=36, hs=36, ld='row1')      # refused
    add('plain_s64_w64_mask', 'plain', 64, hd=64, hs=64, mask=True)
    # a device-side sequence count, with and without a key mask
    for S in (20, 32, 64, 96, 128, 256):
        add('count_s%d' % S, 'count', S)
        add('count_s%d_mask' % S, 'count', S, mask=True)
    add('count_s64_h20', 'count', 64, hs=20)
    add('count_s64_w64', 'count', 64, hd=64, hs=64)
    add('count_s64_w64_mask', 'count', 64, hd=64, hs=64, mask=True)
    add('count_s513', 'count', 513)
    # the log-sum-exp output: the split product writes it at 256 / 512 only
    for S in (20, 64, 128, 256, 512):
        add('lse_s%d' % S, 'lse', S)
    add('lse_s256_h20', 'lse', 256, hs=20)
    add('lse_s256_off', 'lse', 256, off=True)
    add('lse_s64_w36', 'lse', 64, hd=36, hs=36)
    add('lse_s513', 'lse', 513)
    add('lse_hs_lt_hd', 'lse', 32, hd=20, hs=10)
    # the row map: whole 32-key tiles only, and no instantiation for 5, 6 or 7 of them
    for S in (32, 64, 96, 128, 256, 512):
        add('rows_s%d' % S, 'rows', S, dev=True)
    add('rows_s64_nodev', 'rows', 64)
    add('rows_s64_h32', 'rows', 64, hd=32, dev=True)
    add('rows_s20', 'rows', 20, dev=True)                      # refused
    add('rows_s160', 'rows', 160, dev=True)                    # refused
    add('rows_s64_off', 'rows', 64, dev=True, off=True)        # refused
    add('rows_s64_ld1', 'rows', 64, dev=True, ld='row1')       # refused
    add('rows_s64_w36', 'rows', 64, hd=36, dev=True)           # refused
    # the per-vocabulary product: taken at 32 / 64 / 128 under the split product, else not applicable
    for S in (32, 64, 96, 128, 256):
        add('vocab_s%d' % S, 'vocab', S, dev=True)
    add('vocab_s64_nodev', 'vocab', 64)
    add('vocab_s64_w36', 'vocab', 64, hd=36, dev=True)
    add('vocab_s64_off', 'vocab', 64, dev=True, off=True)
    add('vocab_s64_ld1', 'vocab', 64, dev=True, ld='row1')
    add('vocab_s32_huge', 'vocab', 32, dev=True, ld='huge')
    # dropout on the probabilities: the split product (padded heads, 32 / 64 / 128), the one-pass kernel's 32 / 64 / 128 buckets, the
    # statistics pass + the blocked kernel from 129 on
    for p, tag in ((0.0, 'p0'), (0.1, 'p1')):
        for S in (32, 64, 128):
            add('drop_%s_s%d' % (tag, S), 'dropout', S, p=p)
            add('drop_%s_s%d_h20' % (tag, S), 'dropout', S, hs=20, p=p)
        add('drop_%s_s20' % tag, 'dropout', 20, p=p)
        add('drop_%s_s96' % tag, 'dropout', 96, p=p)
        add('drop_%s_s256' % tag, 'dropout', 256, p=p)
    add('drop_p1_s160_h20', 'dropout', 160, hs=20, p=0.1)
    add('drop_p1_s64_off', 'dropout', 64, p=0.1, off=True)
    add('drop_p1_s64_ld1', 'dropout', 64, p=0.1, ld='row1')
    add('drop_p1_s64_w64', 'dropout', 64, hd=64, hs=64, p=0.1)
    add('drop_p0_s64_w36', 'dropout', 64, hd=36, hs=36)
    add('drop_p1_s513', 'dropout', 513, p=0.1)                 # refused
    add('drop_p1_s64_hs36', 'dropout', 64, hd=20, hs=36, p=0.1)         # refused: head_stride > 32 under a narrow head
    add('drop_bad_p', 'dropout', 64, p=1.0)                    # refused
    add('drop_bad_p_w64', 'dropout', 64, hd=64, hs=64, p=1.0)  # refused
    add('drop_bad_p_s513', 'dropout', 513, p=1.0)              # refused: the shape before the probability
    # no sequences.  torch gives a tensor without elements a NULL address, so through the ops wrappers only the rows form (whose
    # operands are views of a buffer with rows of its own) reaches the library's "nothing to launch"; the others record the NULL
    # refusal, and tests/test_attn_plan_cpu.py states the library's own answers over made-up addresses
    for form in FORMS:
        add('%s_empty' % form, form, 64, n_seq=0, dev=True if form in ('rows', 'vocab') else None)
    add('plain_empty_w64', 'plain', 64, hd=64, hs=64, n_seq=0)
    add('plain_empty_s513', 'plain', 513, n_seq=0)             # the checks come before the count
    add('vocab_empty_s96', 'vocab', 96, n_seq=0, dev=True)
    ids = [x['id'] for x in c]
    assert len(set(ids)) == len(ids)
    return c


CASES = _cases()


def case_ids():
    return ['%s@%d' % (c['id'], mode) for c in CASES for mode in MODES]


def layout(c):
    """(columns of one operand, leading dimension of q / k / v, float offset of q's first element): what build() lays out and what
    the CPU test states over made-up addresses."""
    hs = 32 if c['form'] in ('rows', 'vocab') else c['hs']
    W = N_HEAD * hs
    ld = {'row': 3 * W, 'row1': 3 * W + 1, 'huge': HUGE_LD}[c['ld']]
    return W, ld, 1 if c['off'] else 0


def build(c):
    """(name of the ops wrapper, its keyword arguments) for case c: real device tensors, misaligned where the case says so.  Padding
    columns of a head (head_stride > head_dim) hold zeros, as every padded-layout kernel expects."""
    import torch
    gen = torch.Generator().manual_seed(zlib.crc32(c['id'].encode()))
    S, hd, n_seq, form = c['S'], c['hd'], c['n_seq'], c['form']
    W, ld, start = layout(c)
    hs = W // N_HEAD
    n_tok = n_seq * S

    def operands(rows, cols, scale=1.0):
        """`cols` / W operands of `rows` rows side by side in one buffer of pitch ld"""
        if c['ld'] == 'huge':                          # never read: the call is not taken.  One uninitialised buffer, viewed with the pitch
            buf = torch.empty(max(rows - 1, 0) * ld + cols + 8, dtype=torch.float32, device='cuda')
            return buf.as_strided((rows, cols), (ld, 1), start)
        buf = torch.zeros(rows * ld + 8, dtype=torch.float32, device='cuda')
        view = buf.as_strided((rows, cols), (ld, 1), start)
        val = torch.randn(rows, cols // hs, hs, generator=gen) * scale
        if hs > hd:
            val[:, :, hd:] = 0
        view.copy_(val.reshape(rows, cols))
        return view

    def count():
        return torch.tensor([N_DEV], dtype=torch.int32, device='cuda') if c['dev'] else None

    kw = dict(n_seq=n_seq, S=S, n_head=N_HEAD, head_dim=hd, scale=hd ** -0.5)
    if form == 'vocab':
        kw['qkv_vocab'] = operands(1 if c['ld'] == 'huge' else VOCAB, 3 * W, 0.7)
        kw['pos_rows'] = operands(S, 3 * W, 0.7)
        kw['ids'] = torch.randint(0, 1 if c['ld'] == 'huge' else VOCAB, (n_tok,), generator=gen).to(torch.int32).cuda()
        kw['n_seq_dev'] = count()
    else:
        rows = n_tok + S if form == 'rows' else n_tok
        qkv = operands(rows, 3 * W)
        kw.update(q=qkv[:, :W], k=qkv[:, W:2 * W], v=qkv[:, 2 * W:])
        if form == 'rows':
            kw['row_map'] = torch.randperm(rows, generator=gen)[:max(n_tok, 1)].to(torch.int32).cuda()
            kw['n_seq_dev'] = count()
        elif form == 'dropout':
            kw.update(p=c['p'], seed=DROPOUT_SEED, site=DROPOUT_SITE, head_stride=hs)
        else:
            kw['head_stride'] = hs
            if c['mask']:
                m = torch.rand(n_seq, S, generator=gen) < 0.7
                m[:, :1] = True
                kw['key_mask'] = m.reshape(-1).cuda()
            if form == 'count':
                kw['n_seq_dev'] = count()
            if form == 'lse':
                kw['lse'] = torch.zeros(n_tok * N_HEAD, dtype=torch.float32, device='cuda')
    if form != 'dropout':
        out_rows = max(n_tok, 1) if form == 'rows' else n_tok          # rows: a pointer to hand over even without sequences
        kw['out'] = torch.zeros((out_rows, N_HEAD * hd), dtype=torch.float32, device='cuda')
    return CALLS[form], kw
