"""lime_token_attention_bwd_plan_f32 on the CPU: for every case of attn_bwd_route_cases.py under every split mode the plan names the
kernels the commit BEFORE the backward's routing became a plan launched on an MI355X (profiles/attn_bwd_routes_parent.txt, written there
by tools/attn_routes.py --bwd from a kernel trace: recorded, not produced by the code under test), or answers with the status and
message that commit returned.  The argument blocks hold made-up addresses with the case's alignments: the library must not read
through them."""
import ctypes
import os

import pytest

import attn_bwd_route_cases as arc
from lime_cikm25_amd import _lib
from lime_cikm25_amd.build import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = _lib.CONSTANTS

# Cases the ops wrapper itself refuses (ValueError) before the library sees them have no status in the recording; the library's own
# answer to the block the wrapper would have built, as that commit's source reads (attention_bwd: the blocked path's `out` check)
NOT_LAUNCHABLE = {'s160_noout': (C['LIME_ERR_BAD_ARG'],
                                 'lime_token_attention_bwd_f32: S > 128 needs the forward output `out` (delta = dO . O)')}

# kernel as the trace names it -> the plan's family / pass
FAMILY = {'token_attn_bwd_kernel': C['LIME_BWD_ATTN_ONE_PASS'], 'attn_bwd_sp_kernel': C['LIME_BWD_ATTN_SP'],
          'attn_bwd_long_kernel': C['LIME_BWD_ATTN_LONG'], 'attn_bwd_long_sp_kernel': C['LIME_BWD_ATTN_LONG_SP'],
          'wide_bwd_kv_kernel': C['LIME_BWD_ATTN_WIDE']}
PASS = {'attn_stats_kernel<false>': C['LIME_BWD_ATTN_PASS_STATS_FP32'], 'attn_stats_kernel<true>': C['LIME_BWD_ATTN_PASS_STATS_SPLIT'],
        'attn_delta_kernel': C['LIME_BWD_ATTN_PASS_DELTA']}
REDUCE = 'attn_dq_reduce_kernel'


def family_of(kernels):
    """the family and the pass a recorded launch sequence stands for"""
    if not kernels:
        return C['LIME_BWD_ATTN_NONE'], C['LIME_BWD_ATTN_PASS_NONE']
    body = kernels[-2] if kernels[-1] == REDUCE else kernels[-1]
    return FAMILY[body.split('<')[0]], PASS.get(kernels[0], C['LIME_BWD_ATTN_PASS_NONE'])


def recorded():
    """{'id@mode': (status, [kernels], message)} of the parent's run."""
    out = {}
    for line in open(os.path.join(ROOT, 'profiles', 'attn_bwd_routes_parent.txt')):
        key, status, rest = (line.rstrip('\n').split(' ', 2) + [''])[:3]
        if status == '0':
            _sha, kernels = rest.split(' ', 1)
            got = (0, [] if kernels == '-' else kernels.split('; '), None)
        else:
            got = (status if status == 'ValueError' else int(status), None, rest)
        cid, modes = key.split('@')                                        # one line per outcome: the modes that gave it
        for mode in modes.split(','):
            assert '%s@%s' % (cid, mode) not in out
            out['%s@%s' % (cid, mode)] = got
    return out


def fake_args(lib, c, shift=0, n_seq=None):
    """The lime_token_attention_bwd_args ops.token_attention_bwd builds for case c, over addresses that are not memory (`shift`: a
    multiple of 16 bytes added to all of them).  A tensor without elements has the address NULL, as torch gives it to the wrapper;
    `n_seq` overrides the case's count and nothing else (the library's own answer for no sequences)."""
    a = _lib.TokenAttentionBwdArgs()
    S, hd, nh = c['S'], c['hd'], c['n_head']
    W, ld, start, ldd, dstart, ldo, ostart = arc.layout(c)
    addr = lambda base: base + shift
    a.n_seq, a.S, a.n_head, a.head_dim, a.head_stride, a.scale = c['n_seq'] if n_seq is None else n_seq, S, nh, hd, c['hs'], hd ** -0.5
    a.ld_qkv, a.ld_dqkv, a.ldo = ld, ldd, ldo
    filled = c['n_seq'] > 0
    if filled:
        a.q, a.k, a.v = (addr(0x100000) + 4 * (start + i * W) for i in range(3))
        a.dq, a.dk, a.dv = (addr(0x4000000) + 4 * (dstart + i * W) for i in range(3))
        a.dout = addr(0x8000000) + 4 * ostart
    need = lib.lime_token_attention_bwd_workspace_wide(c['n_seq'], S, nh, hd)
    if need:
        a.workspace, a.workspace_floats = addr(0x10000000), max(need, 1 << 20)
    if c['out']:
        a.out, a.ld_out = addr(0xC000000) if filled else None, ldo
    # the wrapper's rule: the lse entry only where a workspace is needed and, for wide heads, only with S > 128 and `out` given
    if c['lse'] and need and (hd <= 32 or (S > 128 and c['out'])):
        a.entry, a.lse = C['LIME_BWD_ATTN_ENTRY_LSE'], addr(0xE000000)
        return a
    a.entry = C['LIME_BWD_ATTN_ENTRY_PLAIN']
    if c['mask'] and filled:
        a.key_mask = addr(0xF000000)
    if c['p'] is not None:
        a.dropout_p, a.dropout_seed, a.dropout_site = c['p'], arc.DROPOUT_SEED, arc.DROPOUT_SITE
    return a


def plan_of(lib, a):
    plan = _lib.TokenAttentionBwdPlan()
    st = lib.lime_token_attention_bwd_plan_f32(ctypes.byref(a), ctypes.byref(plan))
    return st, plan.family, plan.stats_pass, [plan.name[i].value.decode() for i in range(plan.n_launches)]


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


def test_the_recording_covers_every_case_family_and_pass(parent):
    assert sorted(parent) == sorted(arc.case_ids())
    assert {k.split('@')[0] for k, v in parent.items() if v[0] == 'ValueError'} == set(NOT_LAUNCHABLE)
    seen = [family_of(k) for _, k, _ in parent.values() if k]
    passes = {v for n, v in C.items() if n.startswith('LIME_BWD_ATTN_PASS_')}
    families = {v for n, v in C.items() if n.startswith('LIME_BWD_ATTN_') and not n.startswith(('LIME_BWD_ATTN_PASS_', 'LIME_BWD_ATTN_ENTRY_'))}
    assert {f for f, _ in seen} | {C['LIME_BWD_ATTN_NONE']} == families
    assert {p for _, p in seen} | {C['LIME_BWD_ATTN_PASS_NONE']} == passes
    assert set(FAMILY.values()) | {C['LIME_BWD_ATTN_NONE']} == families and set(PASS.values()) | {C['LIME_BWD_ATTN_PASS_NONE']} == passes


@pytest.mark.parametrize('mode', arc.MODES)
def test_plan_names_what_the_parent_launched(lib, parent, mode):
    lib.lime_set_split_gemm(mode)
    for c in arc.CASES:
        key = '%s@%d' % (c['id'], mode)
        status, kernels, message = parent[key]
        if status == 'ValueError':
            status, message = NOT_LAUNCHABLE[c['id']]
        got, family, stats, names = plan_of(lib, fake_args(lib, c))
        assert got == status, key
        if status < 0:
            assert lib.lime_last_error_string().decode() == message, key
            assert (family, stats, names) == (0, 0, []), key
            continue
        assert names == kernels, key
        assert (family, stats) == family_of(kernels), key
        # different, equally aligned addresses: the same plan
        assert plan_of(lib, fake_args(lib, c, shift=0x40)) == (got, family, stats, names), key


@pytest.mark.parametrize('mode', arc.MODES)
def test_no_sequences_launch_nothing(lib, mode):
    """n_seq = 0 over real addresses, which the ops wrapper cannot state (the recording holds its NULL refusals): as the library's source
    reads, the checks in front of the count run, then nothing is launched and nothing behind the count is asked."""
    lib.lime_set_split_gemm(mode)
    by_id = {c['id']: c for c in arc.CASES}
    nothing = (0, C['LIME_BWD_ATTN_NONE'], C['LIME_BWD_ATTN_PASS_NONE'], [])
    for c in arc.CASES:
        if c['n_seq'] == 0:
            continue
        full = plan_of(lib, fake_args(lib, c))
        got = plan_of(lib, fake_args(lib, c, n_seq=0))
        if full[0] == 0:
            assert got == nothing, c['id']
        else:
            assert got == nothing or got[0] == full[0], c['id']
    for cid in ('s513', 'hs_lt_hd', 's64_hs36', 's64_w34', 's513_w64', 's64_w64_off', 's64_w36_dld1'):      # in front of the count
        assert plan_of(lib, fake_args(lib, by_id[cid], n_seq=0))[0] == C['LIME_ERR_UNSUPPORTED'], cid
    assert plan_of(lib, fake_args(lib, by_id['bad_p'], n_seq=0))[0] == C['LIME_ERR_BAD_ARG']
    for cid in ('s160_mask', 's160_noout', 's160_lse_nh65'):                                                # behind it
        assert plan_of(lib, fake_args(lib, by_id[cid], n_seq=0)) == nothing, cid


def test_plan_rejects_a_missing_block_and_an_unknown_entry(lib):
    plan = _lib.TokenAttentionBwdPlan()
    assert lib.lime_token_attention_bwd_plan_f32(None, ctypes.byref(plan)) == -1
    assert b'lime_token_attention_bwd_plan_f32: args is NULL' in lib.lime_last_error_string()
    a = fake_args(lib, arc.CASES[0])
    assert lib.lime_token_attention_bwd_plan_f32(ctypes.byref(a), None) == -1
    for entry in (-1, 2):
        a.entry = entry
        assert lib.lime_token_attention_bwd_plan_f32(ctypes.byref(a), ctypes.byref(plan)) == -1
        assert b'lime_token_attention_bwd_plan_f32: entry' in lib.lime_last_error_string()


def test_the_run_entry_refuses_a_missing_block_before_any_launch(lib):
    """lime_token_attention_bwd_f32 over nothing that could launch: no block, an entry outside the enum, and all-zero blocks, which the
    first check of either entry (lse, then the operands) refuses."""
    assert lib.lime_token_attention_bwd_f32(None, None) == -1
    assert b'lime_token_attention_bwd_f32: args is NULL' in lib.lime_last_error_string()
    for entry in (-1, 2):
        a = _lib.TokenAttentionBwdArgs()
        a.entry = entry
        assert lib.lime_token_attention_bwd_f32(ctypes.byref(a), None) == -1
        assert lib.lime_last_error_string().decode() == 'lime_token_attention_bwd_f32: entry %d' % entry
    for entry, message in (('plain', 'lime_token_attention_bwd_f32: null pointer'), ('lse', 'lime_token_attention_bwd_lse_f32: lse is NULL')):
        a = _lib.TokenAttentionBwdArgs()
        a.entry = _lib.BWD_ATTN_ENTRY[entry]
        assert lib.lime_token_attention_bwd_f32(ctypes.byref(a), None) == -1
        assert lib.lime_last_error_string().decode() == message
