"""Plan and launch agree on the device: ops.linear_plan (lime_linear_plan_f32 with this device's CU count) names the kernel that
lime_last_linear_kernel() reports after ops.linear ran the same arguments -- one or two cases of linear_route_cases.py per instantiation
family and both sides of each routing threshold.  No numerics here: test_kernels_gpu.py and test_split_gemm_gpu.py own those."""
import pytest
import torch

import linear_route_cases as lrc

pytestmark = pytest.mark.gpu

# (case id, split modes)
PICKED = [
    ('m4095_n1280', (1,)), ('m4096_n1280', (1,)),
    ('tanh_m12287_n1280', (1,)), ('tanh_m12288_n1280', (1,)), ('sigmoid_m12288_n1280', (1,)),
    ('resids_m12287_n1280', (1,)), ('resids_m12288_n1280', (1,)), ('resdiv_m12287_n1280', (1,)), ('resdiv_m12288_n1280', (1,)),
    ('fewtiles_n1024', (0, 1, 5)), ('fewtiles_n1280', (0, 1)),
    ('fill_m7168', (1,)), ('fill_m7169', (1,)), ('fill_mdev_m7168', (1,)),
    ('k60_big', (1,)), ('k64_big', (1,)), ('k28_big', (0,)), ('k32_big', (0,)), ('k12_mid', (1,)), ('k16_mid', (1,)),
    ('off_a_big', (1,)), ('ld1_c_big', (1,)), ('k62_mid', (1,)), ('k63_mid', (1,)), ('n254_mid', (1,)),
    ('ln_dense_n300', (0, 1)), ('ln_ids_pe_n300', (1,)), ('ln_ids_pe_mdev_n300', (1, 3)), ('ln_dense_rstd_n304', (0,)), ('ln_pool_n300', (0, 1)), ('ln_dense_off_n320', (1,)),
    ('ln_n256', (1,)), ('ln_small_n260', (1,)),
    ('plain_n400', (0,)), ('relu_n200', (4,)), ('res_n1200', (4,)), ('plain_n1280', (0, 1)),
    ('cids_n960', (0, 1)),
    ('relugrad_m8192_n1024', (1,)), ('relugrad_m8192_n320', (1,)), ('relugrad_m2048_n512', (1,)),
    ('dropout_relu_m8192_n1280', (1,)), ('dropout_relu_m4000_n512', (1,)), ('dropout_none_m4096_n512', (1,)),
    ('ape_big_n320', (1,)), ('ape_small_k62', (1,)),
    ('mid_m40', (1,)), ('mid_m1700', (1,)), ('mid_m3000', (1,)), ('mid_m9000', (1,)),
]


@pytest.mark.filterwarnings('ignore:lime_linear_f32. LayerNorm epilogue on operands that are not 16-byte aligned')
def test_plan_names_the_kernel_that_runs():
    from lime_cikm25_amd import _lib, ops
    lib = _lib.load()
    by_id = {c['id']: c for c in lrc.CASES}
    start = lib.lime_set_split_gemm(-1)
    wrong, families = [], set()
    try:
        for cid, modes in PICKED:
            kw = lrc.build(by_id[cid])
            for mode in modes:
                lib.lime_set_split_gemm(mode)
                plan = ops.linear_plan(**kw)                 # raises unless the call returns OK
                ops.linear(**kw)                             # raises unless the call returns OK
                ran = lib.lime_last_linear_kernel().decode()
                families.add(plan['family'])
                if plan['kernel'] != ran:
                    wrong.append('%s@%d: planned %s, ran %s' % (cid, mode, plan['kernel'], ran))
        torch.cuda.synchronize()
    finally:
        lib.lime_set_split_gemm(start)
    assert not wrong, '\n'.join(wrong)
    assert families == {'sp', 'pp', 'mid', 'general'}
