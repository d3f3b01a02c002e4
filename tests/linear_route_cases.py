"""The lime_linear_f32 routing cases shared by tools/linear_routes.py (which launches each of them on the GPU and records the kernel that
ran) and tests/test_linear_plan_cpu.py / test_linear_plan_gpu.py (which ask lime_linear_plan_f32 for the same decisions).  Pure data,
but for build(), which makes a case's device tensors.  The shapes are the smallest that still reach each branch of the routing
(DESIGN.md section 5), on both sides of every threshold; every case is run under each split mode of MODES.

A case is a dict: id, M, N, K, act, and the operands it has --
  res   None | 'dense' | 'div' (one row broadcast to RES_DIV rows) | 'mod' (a periodic [RES_MOD, N] table) | 'ids' (gathered rows) |
        'ids_pe' (gathered rows + a positional table of RES_PERIOD rows)
  ln / rstd / pool32 / m_dev / c_ids / a_ids / a_pe / dropout: flags
  off   operands ('a', 'w', 'c', 'res') whose base address is 4 bytes past a 16-byte boundary
  ld1   operands whose leading dimension is the row length + 1
"""
import zlib

MODES = (0, 1, 3, 4, 5)            # lime_set_split_gemm(): 0 fp32 kernels, 1 split product, |2 also out_proj, |4 without the fill rules
RES_DIV, RES_MOD, RES_PERIOD, RES_ROWS, A_ROWS, A_PERIOD = 4, 32, 32, 100, 500, 32
DROPOUT = (0.25, 1234, 7)          # p, seed, site


def _case(cid, M, N, K=64, act=None, res=None, ln=False, rstd=False, pool32=False, m_dev=False, c_ids=False, a_ids=False, a_pe=False,
          dropout=False, off=(), ld1=()):
    return dict(id=cid, M=M, N=N, K=K, act=act, res=res, ln=ln, rstd=rstd, pool32=pool32, m_dev=m_dev, c_ids=c_ids, a_ids=a_ids or a_pe,
                a_pe=a_pe, dropout=dropout, off=tuple(off), ld1=tuple(ld1))


def _cases():
    c = []
    add = lambda *a, **k: c.append(_case(*a, **k))
    # M 4095 / 4096: the mid-M kernel hands over to the big-M kernels
    for M in (4095, 4096):
        for N in (256, 1280):
            add('m%d_n%d' % (M, N), M, N)
    # M 12287 / 12288: the epilogues the split-product kernel takes from there on only
    for M in (12287, 12288):
        for N in (256, 1280):
            add('tanh_m%d_n%d' % (M, N), M, N, act='tanh')
            add('sigmoid_m%d_n%d' % (M, N), M, N, act='sigmoid')
            add('resids_m%d_n%d' % (M, N), M, N, res='ids')
            add('resdiv_m%d_n%d' % (M, N), M, N, res='div')
    # few tiles: 159 vs 160 tiles of 128 x 256 (M = 4096: 32 row blocks x 4 / 5 column blocks), also with the epilogues of the mid-M kernel
    for N in (1024, 1280):
        add('fewtiles_n%d' % N, 4096, N)
        add('fewtiles_relu_n%d' % N, 4096, N, act='relu')
        add('fewtiles_res_n%d' % N, 4096, N, res='dense')
    # the fill rule at 256 CUs (N = 1280: four 320-column blocks): 0.25, 0.4375 | 0.453, 0.5; with m_dev the rule is skipped
    for M in (4096, 7168, 7169, 8192):
        add('fill_m%d' % M, M, 1280)
        add('fill_mdev_m%d' % M, M, 1280, m_dev=True)
    # K: the split product needs two 32-deep chunks, the fp32 LDS-DMA kernel two 16-deep ones, the mid-M kernel one
    for K in (60, 64, 28, 32, 12, 16):
        add('k%d_big' % K, 8192, 1280, K=K)
        add('k%d_mid' % K, 1700, 256, K=K)
    # operands that are not 16-byte friendly
    for tag, M, N in (('big', 8192, 1280), ('mid', 1700, 256)):
        add('k62_%s' % tag, M, N, K=62, res='dense')
        add('k63_%s' % tag, M, N, K=63, res='dense')
        add('n%d_%s' % (N - 2, tag), M, N - 2, res='dense')
        for op in ('a', 'w', 'c', 'res'):
            add('off_%s_%s' % (op, tag), M, N, res='dense', off=(op,))
            add('ld1_%s_%s' % (op, tag), M, N, res='dense', ld1=(op,))
    # the LayerNorm epilogue
    for N in (256, 260, 300, 304, 320):
        add('ln_n%d' % N, 4096, N, ln=True)
        add('ln_relu_n%d' % N, 4096, N, ln=True, act='relu')
        add('ln_small_n%d' % N, 1000, N, ln=True, res='dense')
        add('ln_small_off_n%d' % N, 1000, N, ln=True, res='dense', off=('c',))
        for res in ('dense', 'ids_pe'):
            for rstd in (False, True):
                for off in ((), ('c',)):
                    add('ln_%s%s%s_n%d' % (res, '_rstd' if rstd else '', '_off' if off else '', N), 4096, N, ln=True, res=res, rstd=rstd, off=off)
        add('ln_pool_n%d' % N, 4096, N, ln=True, res='dense', pool32=True)
        add('ln_pool_off_n%d' % N, 4096, N, ln=True, res='dense', pool32=True, off=('c',))
    # out_proj behind the compaction (m_dev: the fill rule is skipped): the fp32 kernel's, the split product's under split mode 1 | 2
    add('ln_ids_pe_mdev_n300', 4096, 300, ln=True, res='ids_pe', m_dev=True)
    add('ln_ids_pe_rstd_mdev_n300', 4096, 300, ln=True, res='ids_pe', rstd=True, m_dev=True)
    add('ln_pool_ids_n300', 4096, 300, ln=True, res='ids_pe', pool32=True)
    add('ln_pool_nores_n300', 4096, 300, ln=True, pool32=True)
    add('ln_pool_m4100', 4100, 300, ln=True, res='dense', pool32=True)
    add('ln_pool_m2048', 2048, 300, ln=True, res='dense', pool32=True)
    add('ln_n324', 4096, 324, ln=True, res='dense')
    add('ln_small_n324', 1000, 324, ln=True, res='dense')
    add('ln_tanh_n300', 4096, 300, ln=True, act='tanh')
    add('ln_relu_res_n300', 4096, 300, ln=True, act='relu', res='dense')
    # plain / ReLU / residual over the column counts of the 256 / 320 blocks, the 304 / 208 trimmed slabs and the N = 1280 tie
    for N in (200, 208, 256, 300, 320, 400, 1200, 1280):
        add('plain_n%d' % N, 8192, N)
        add('relu_n%d' % N, 8192, N, act='relu')
        add('res_n%d' % N, 8192, N, res='dense')
        add('resmod_n%d' % N, 8192, N, res='mod')
    add('resids_big_n400', 8192, 400, res='ids')
    # c_ids: the legal form, and each way of breaking it
    add('cids_n960', 4096, 960, res='mod', c_ids=True)
    add('cids_n1024', 4096, 1024, res='mod', c_ids=True)
    add('cids_n1000', 4096, 1000, res='mod', c_ids=True)
    add('cids_ln', 4096, 320, res='mod', c_ids=True, ln=True)
    add('cids_relu', 4096, 960, res='mod', c_ids=True, act='relu')
    add('cids_resids', 4096, 960, res='ids', c_ids=True)
    add('cids_dense', 4096, 960, res='dense', c_ids=True)
    add('cids_m4000', 4000, 960, res='mod', c_ids=True)
    add('cids_off_c', 4096, 960, res='mod', c_ids=True, off=('c',))
    add('cids_k62', 4096, 960, K=62, res='mod', c_ids=True)
    # the ReLU gradient: fused in the 256-column split-product tiles, else two passes
    for M, N in ((8192, 512), (8192, 1024), (8192, 320), (8192, 1280), (2048, 512)):
        add('relugrad_m%d_n%d' % (M, N), M, N, act='relu_grad', res='dense')
    add('relugrad_off', 8192, 1024, act='relu_grad', res='dense', off=('res',))
    # dropout behind the activation: fused in the split-product ReLU kernel, else a pass of its own
    for M, N in ((4096, 512), (4000, 512), (8192, 1280)):
        add('dropout_relu_m%d_n%d' % (M, N), M, N, act='relu', dropout=True)
        add('dropout_none_m%d_n%d' % (M, N), M, N, dropout=True)
    # a positional A operand: the general kernel's big tiles and its 64 x 64 tiles at 16 / 8 / 4-byte staging
    for N in (256, 320):
        add('ape_big_n%d' % N, 4096, N, a_pe=True)
        add('ape_big_relu_n%d' % N, 4096, N, a_pe=True, act='relu')
    add('ape_big_res', 4096, 256, a_pe=True, res='dense')
    for K in (64, 62, 63):
        add('ape_small_k%d' % K, 1000, 256, K=K, a_pe=True)
    add('ape_ln', 4096, 300, a_pe=True, ln=True)
    # the general kernel's 64 x 64 tiles without a_pe (misaligned small problems) and gathered A rows
    add('aids_mid', 1700, 256, a_ids=True)
    add('aids_big', 8192, 1280, a_ids=True)
    add('aids_small_k62', 1000, 256, K=62, a_ids=True)
    # the mid-M tile shapes: 32 x 32 (M = 40, 1700), 32 x 64 (3000), 64 x 64 (9000), with its run-time epilogues
    for M in (40, 1700, 3000, 9000):
        add('mid_m%d' % M, M, 400, act='tanh', res='dense')
        add('mid_mdev_m%d' % M, M, 400, m_dev=True)
    add('mid_resdiv', 1700, 400, res='div')
    add('mid_resmod', 1700, 400, res='mod')
    add('mid_resids', 1700, 400, act='sigmoid', res='ids')
    # a device-side row count on operands the LDS-DMA kernels do not take
    add('mdev_k62', 1700, 256, K=62, m_dev=True)
    add('mdev_ln_small', 1000, 300, ln=True, res='dense', m_dev=True)
    add('mdev_ln_big', 4096, 300, ln=True, res='dense', m_dev=True)
    ids = [x['id'] for x in c]
    assert len(set(ids)) == len(ids)
    return c


CASES = _cases()


def case_ids():
    return ['%s@%d' % (c['id'], mode) for c in CASES for mode in MODES]


def build(c):
    """ops.linear's keyword arguments for case c: real device tensors, misaligned where the case says so."""
    import torch
    gen = torch.Generator().manual_seed(zlib.crc32(c['id'].encode()))
    M, N, K = c['M'], c['N'], c['K']

    def mat(name, rows, cols, fill=True):
        ld = cols + (1 if name in c['ld1'] else 0)
        start = 1 if name in c['off'] else 0
        buf = torch.zeros(rows * ld + 8, dtype=torch.float32, device='cuda')
        view = buf.as_strided((rows, cols), (ld, 1), start)
        if fill:
            view.copy_(torch.randn(rows, cols, generator=gen) * (cols ** -0.5 if name == 'w' else 1.0))
        return view

    def ids(n, hi, perm=False):
        t = torch.randperm(hi, generator=gen)[:n] if perm else torch.randint(0, hi, (n,), generator=gen)
        return t.to(torch.int32).cuda()

    kw = dict(w=mat('w', N, K), bias=torch.randn(N, generator=gen).cuda(), act=c['act'])
    if c['a_ids']:
        kw.update(a=mat('a', A_ROWS, K), a_ids=ids(M, A_ROWS))
        if c['a_pe']:
            kw.update(a_pe=mat('a_pe', A_PERIOD, K), a_period=A_PERIOD)
    else:
        kw['a'] = mat('a', M, K)
    res = c['res']
    if res == 'dense':
        kw['res'] = mat('res', M, N)
    elif res == 'div':
        kw.update(res=mat('res', (M + RES_DIV - 1) // RES_DIV, N), res_div=RES_DIV)
    elif res == 'mod':
        kw.update(res=mat('res', RES_MOD, N), res_mod=RES_MOD)
    elif res in ('ids', 'ids_pe'):
        kw.update(res=mat('res', RES_ROWS, N), res_ids=ids(M, RES_ROWS))
        if res == 'ids_pe':
            kw.update(res_pe=mat('res_pe', RES_PERIOD, N), res_period=RES_PERIOD)
        if c['c_ids']:
            kw['res_mod'] = RES_MOD
    if c['ln']:
        kw['ln'] = (torch.randn(N, generator=gen).cuda(), torch.randn(N, generator=gen).cuda())
        if c['rstd']:
            kw['ln_rstd'] = torch.zeros(M, dtype=torch.float32, device='cuda')
    if c['pool32']:
        kw['pool32'] = True
    if c['m_dev']:
        kw['m_dev'] = torch.tensor([M - 3], dtype=torch.int32, device='cuda')
    if c['c_ids']:
        kw['c_ids'] = ids(M, M, perm=True)
    if c['dropout']:
        kw['dropout'] = DROPOUT
    kw['out'] = mat('c', M // 32 if (c['pool32'] and M % 32 == 0) else M, N, fill=False)
    return kw
