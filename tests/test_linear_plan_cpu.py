"""lime_linear_plan_f32 on the CPU: for every case of linear_route_cases.py under every split mode the plan names the kernel the commit
BEFORE the routing became a plan launched on an MI355X (profiles/linear_routes_parent.txt, written there by tools/linear_routes.py:
recorded, not produced by the code under test), with the second pass and the mid-M tile shape that go with it, or refuses with the
status and message that commit returned.  The argument blocks hold made-up addresses: the library must not read through them.
No GPU: n_cu = 256, the MI355X's CU count, is passed in."""
import ctypes
import os

import pytest

import linear_route_cases as lrc
from lime_cikm25_amd import _lib
from lime_cikm25_amd.build import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CU = 256

# Cases ops.linear itself refuses (ValueError) before the library sees them, so the recording holds no status for them; the library's
# own answer, as its source reads: both are argument blocks neither big-M kernel takes.
NOT_LAUNCHABLE = {
    'ln_pool_m4100': (-2, 'pool32 needs the big-M kernel (M >= 4096 and a multiple of 32, LayerNorm + dense residual, 16-byte operands)'),
    'cids_dense': (-2, 'c_ids needs the big-M kernel (M >= 4096, 16-byte operands, periodic residual, no LayerNorm, act none)'),
}


def recorded():
    """{'id@mode': (status, kernel, message)} of the parent's run."""
    out = {}
    for line in open(os.path.join(ROOT, 'profiles', 'linear_routes_parent.txt')):
        key, status, kernel, rest = line.rstrip('\n').split(' ', 3)
        if status == '0':
            kernel, _sha = (kernel + ' ' + rest).rsplit(' ', 1)            # the kernel name has spaces, the hash has none
            got = (0, kernel, None)
        else:
            got = (status if status == 'ValueError' else int(status), None, rest.split(' ', 1)[1])
        cid, modes = key.split('@')                                        # one line per outcome: the modes that gave it
        for mode in modes.split(','):
            assert '%s@%s' % (cid, mode) not in out
            out['%s@%s' % (cid, mode)] = got
    return out


def fake_args(c):
    """The lime_linear_args ops.linear builds for case c, over addresses that are not memory."""
    a = _lib.LinearArgs()
    M, N, K = c['M'], c['N'], c['K']
    addr = lambda name, base: base + (4 if name in c['off'] else 0)
    ld = lambda name, cols: cols + (1 if name in c['ld1'] else 0)
    a.a, a.lda = addr('a', 0x10000), ld('a', K)
    if c['a_ids']:
        a.a_ids = 0x20000
    if c['a_pe']:
        a.a_pe, a.lda_pe, a.a_period = 0x30000, K, lrc.A_PERIOD
    a.w, a.ldw, a.bias = addr('w', 0x40000), ld('w', K), 0x50000
    res = c['res']
    if res:
        a.res, a.ldr, a.res_div = addr('res', 0x60000), ld('res', N), lrc.RES_DIV if res == 'div' else 1
        if res in ('ids', 'ids_pe'):
            a.res_ids = 0x70000
            if res == 'ids_pe':
                a.res_pe, a.ldr_pe, a.res_period = 0x80000, N, lrc.RES_PERIOD
        elif res == 'mod':
            a.res_mod = lrc.RES_MOD
    if c['ln']:
        a.ln_gamma, a.ln_beta, a.ln_eps = 0xA0000, 0xB0000, 1e-5
        if c['rstd']:
            a.ln_rstd = 0xC0000
    a.c, a.ldc = addr('c', 0x90000), ld('c', N)
    a.M, a.N, a.K, a.act, a.act_scale = M, N, K, _lib.LIME_ACT[c['act']], 1.0
    a.pool32 = 1 if c['pool32'] else 0
    if c['m_dev']:
        a.m_dev = 0xD0000
    if c['c_ids']:
        a.c_ids = 0xE0000
    if c['dropout']:
        a.dropout_p, a.dropout_seed, a.dropout_site = lrc.DROPOUT
    return a


def mid_shape(M, N):
    """The smallest mid-M tiles that still run in one round of three workgroups per CU (gemm_mid_f32.hip), stated independently."""
    slots, up = 3 * N_CU, lambda x, t: (x + t - 1) // t
    return 2 if up(M, 32) * up(N, 32) <= slots else 1 if up(M, 32) * up(N, 64) <= slots else 0


@pytest.fixture(scope='module')
def lib():
    build_library()
    lib = _lib.load()
    prev = lib.lime_set_split_gemm(-1)
    yield lib
    lib.lime_set_split_gemm(prev)


@pytest.fixture(scope='module')
def parent():
    return recorded()


def test_the_recording_covers_every_case_and_every_threshold_pair_launched(parent):
    assert sorted(parent) == sorted(lrc.case_ids())
    refused_by_ops = {k.split('@')[0] for k, v in parent.items() if v[0] == 'ValueError'}
    assert refused_by_ops == set(NOT_LAUNCHABLE)


@pytest.mark.parametrize('mode', lrc.MODES)
def test_plan_names_what_the_parent_launched(lib, parent, mode):
    lib.lime_set_split_gemm(mode)
    for c in lrc.CASES:
        key = '%s@%d' % (c['id'], mode)
        status, kernel, message = parent[key]
        if status == 'ValueError':
            status, message = NOT_LAUNCHABLE[c['id']]
        plan = _lib.LinearPlan()
        got = lib.lime_linear_plan_f32(ctypes.byref(fake_args(c)), N_CU, ctypes.byref(plan))
        assert got == status, key
        if status != 0:
            assert message in lib.lime_last_error_string().decode(), key
            continue
        assert plan.name.decode() == kernel, key
        # Fused in the split-product kernel only: the ReLU gradient in its RES = 3 instantiation, dropout in its ReLU instantiations.
        # Anywhere else the recorded kernel ran the bare GEMM and a pass of its own followed.
        sp = kernel.startswith('gemm_sp_kernel<')
        relu_grad_fused = sp and kernel.split(', ')[3] == '3'
        dropout_fused = sp and c['act'] == 'relu'
        want_pass = (_lib.LINEAR_PASS_RELU_BWD if c['act'] == 'relu_grad' and not relu_grad_fused else 0) | \
                    (_lib.LINEAR_PASS_DROPOUT if c['dropout'] and not dropout_fused else 0)
        assert plan.second_pass == want_pass, key
        family = {'gemm_sp_kernel': 1, 'gemm_pp_kernel': 2, 'gemm_mid_kernel': 3, 'gemm_f32_kernel': 4}[kernel.split('<')[0]]
        assert plan.family == family, key
        assert plan.mid_shape == (mid_shape(c['M'], c['N']) if family == 3 else -1), key


def test_mid_shapes_of_the_four_sizes(lib):
    lib.lime_set_split_gemm(1)
    by_id = {c['id']: c for c in lrc.CASES}
    for M, shape, tiles in ((40, 2, 2 * 13), (1700, 2, 54 * 13), (3000, 1, 94 * 7), (9000, 0, 141 * 7)):
        plan = _lib.LinearPlan()
        assert lib.lime_linear_plan_f32(ctypes.byref(fake_args(by_id['mid_m%d' % M])), N_CU, ctypes.byref(plan)) == 0
        assert (plan.name.decode(), plan.mid_shape, plan.tiles) == ('gemm_mid_kernel', shape, tiles)


def test_plan_follows_the_cu_count_it_is_given(lib):
    """M = 7169, N = 1280 is 116 tiles of 256 x 320: fill 0.453 of one round on 256 CUs, 0.38 of one round on 304."""
    lib.lime_set_split_gemm(1)
    a = fake_args({c['id']: c for c in lrc.CASES}['fill_m7169'])
    names = []
    for n_cu in (256, 304):
        plan = _lib.LinearPlan()
        assert lib.lime_linear_plan_f32(ctypes.byref(a), n_cu, ctypes.byref(plan)) == 0
        names.append(plan.name.decode().split('<')[0])
    assert names == ['gemm_sp_kernel', 'gemm_pp_kernel']


def test_plan_rejects_what_linear_rejects_and_plans_nothing_for_no_rows(lib):
    plan = _lib.LinearPlan()
    assert lib.lime_linear_plan_f32(None, N_CU, ctypes.byref(plan)) == -1
    assert b'lime_linear_plan_f32: args is NULL' in lib.lime_last_error_string()
    a = fake_args(lrc.CASES[0])
    assert lib.lime_linear_plan_f32(ctypes.byref(a), N_CU, None) == -1
    a.M = 0
    assert lib.lime_linear_plan_f32(ctypes.byref(a), N_CU, ctypes.byref(plan)) == 0
    assert (plan.family, plan.second_pass, plan.mid_shape, plan.tiles, plan.name) == (0, 0, -1, 0, b'')
