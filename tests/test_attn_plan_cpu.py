"""lime_token_attention_plan_f32 on the CPU: for every case of attn_route_cases.py under every split mode the plan names the kernels
the commit BEFORE the routing became a plan launched on an MI355X (profiles/attn_routes_parent.txt, written there by
tools/attn_routes.py from a kernel trace: recorded, not produced by the code under test), or answers with the status and message that
commit returned.  The argument blocks hold made-up addresses with the case's alignments: the library must not read through them."""
import ctypes
import os

import pytest

import attn_route_cases as arc
from lime_cikm25_amd import _lib
from lime_cikm25_amd.build import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = _lib.CONSTANTS

# Cases an ops wrapper itself refuses (ValueError) before the library sees them would have no status in the recording and would be
# checked against the library's source here.  The table has none: what the wrappers refuse there never reaches a routing rule.
NOT_LAUNCHABLE = {}

# kernel as the trace names it -> the plan's family
FAMILY = {'token_attn_sp_kernel': C['LIME_ATTN_SP'], 'token_attn_sp_long_kernel': C['LIME_ATTN_SP_LONG'],
          'token_attn_sp_vocab_kernel': C['LIME_ATTN_SP_VOCAB'], 'token_attn_kernel': C['LIME_ATTN_MFMA'], 'wide_fwd_kernel': C['LIME_ATTN_WIDE'],
          'token_attn_fwd_dropout_kernel': C['LIME_ATTN_DROPOUT'], 'attn_fwd_long_dropout_kernel': C['LIME_ATTN_DROPOUT_LONG']}
STATS = {'attn_stats_kernel<false>': C['LIME_ATTN_STATS_FP32'], 'attn_stats_kernel<true>': C['LIME_ATTN_STATS_SPLIT']}


def recorded():
    """{'id@mode': (status, [kernels], message)} of the parent's run."""
    out = {}
    for line in open(os.path.join(ROOT, 'profiles', 'attn_routes_parent.txt')):
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


def fake_args(c, shift=0, n_seq=None):
    """The lime_token_attention_args the ops wrapper of case c builds, over addresses that are not memory (`shift`: a multiple of 16
    bytes added to all of them).  A tensor without elements has the address NULL, as torch gives it to the wrappers; `n_seq`
    overrides the case's count WITHOUT that (the library's own answer for no sequences)."""
    a = _lib.TokenAttentionArgs()
    form, hd = c['form'], c['hd']
    W, ld, start = arc.layout(c)
    empty = c['n_seq'] == 0 and n_seq is None
    n_seq = c['n_seq'] if n_seq is None else n_seq
    addr = lambda base: base + shift
    a.form = _lib.ATTN_FORM[form]
    a.n_seq, a.S, a.n_head, a.head_dim, a.head_stride, a.scale = n_seq, c['S'], arc.N_HEAD, hd, W // arc.N_HEAD, hd ** -0.5
    a.ld_qkv, a.ldo = ld, arc.N_HEAD * hd
    if not (empty and form in ('plain', 'count', 'lse', 'dropout')):       # there q / k / v have n_seq * S rows
        a.q, a.k, a.v = (addr(0x100000) + 4 * (start + i * W) for i in range(3))
    if not (empty and form != 'rows'):                                     # the rows case hands over a row of its own
        a.out = addr(0x900000)
    if form == 'vocab':
        a.pos_rows = addr(0x300000) + 4 * start
    if form == 'rows' or (form == 'vocab' and not empty):
        a.row_map = addr(0x800000)
    if c['mask']:
        a.key_mask = addr(0x500000)
    if c['dev']:
        a.n_seq_dev = addr(0x600000)
    if form == 'lse' and not empty:
        a.lse = addr(0x700000)
    if form == 'dropout':
        a.dropout_p, a.dropout_seed, a.dropout_site = c['p'], arc.DROPOUT_SEED, arc.DROPOUT_SITE
        a.workspace_floats = 0 if hd > 32 else _lib.load().lime_token_attention_stats_workspace(n_seq, c['S'], arc.N_HEAD)
        if a.workspace_floats:
            a.workspace = addr(0xA00000)
    return a


def plan_of(lib, a):
    plan = _lib.TokenAttentionPlan()
    st = lib.lime_token_attention_plan_f32(ctypes.byref(a), ctypes.byref(plan))
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


def test_the_recording_covers_every_case_and_every_family(parent):
    assert sorted(parent) == sorted(arc.case_ids())
    assert {k.split('@')[0] for k, v in parent.items() if v[0] == 'ValueError'} == set(NOT_LAUNCHABLE)
    seen = {FAMILY[k[-1].split('<')[0]] for _, k, _ in parent.values() if k}
    want = {v for n, v in C.items() if n.startswith('LIME_ATTN_') and not n.startswith(('LIME_ATTN_FORM_', 'LIME_ATTN_STATS_'))}
    assert seen | {C['LIME_ATTN_NONE']} == want
    assert any(k == [] for _, k, _ in parent.values())                     # "nothing to launch" is there too
    assert {c['form'] for c in arc.CASES} == set(arc.FORMS)


@pytest.mark.parametrize('mode', arc.MODES)
def test_plan_names_what_the_parent_launched(lib, parent, mode):
    lib.lime_set_split_gemm(mode)
    for c in arc.CASES:
        key = '%s@%d' % (c['id'], mode)
        status, kernels, message = parent[key]
        got, family, stats, names = plan_of(lib, fake_args(c))
        assert got == status, key
        if status < 0:
            assert lib.lime_last_error_string().decode() == message, key
        if status != 0:
            assert (family, stats, names) == (0, 0, []), key
            continue
        assert names == kernels, key
        assert family == (FAMILY[kernels[-1].split('<')[0]] if kernels else C['LIME_ATTN_NONE']), key
        assert stats == (STATS[kernels[0]] if len(kernels) == 2 else C['LIME_ATTN_STATS_NONE']), key
        # different, equally aligned addresses: the same plan
        assert plan_of(lib, fake_args(c, shift=0x40)) == (got, family, stats, names), key


@pytest.mark.parametrize('mode', arc.MODES)
def test_no_sequences_launch_nothing(lib, mode):
    """n_seq = 0 over real addresses, which the ops wrappers cannot state (the recording holds their NULL refusals): as the library's
    source reads, every form's checks run first, then nothing is launched -- and the vocab form answers LIME_NOT_APPLICABLE before it
    looks at the count."""
    lib.lime_set_split_gemm(mode)
    by_id = {c['id']: c for c in arc.CASES}
    for c in arc.CASES:
        if c['n_seq'] == 0 or c['ld'] == 'huge':
            continue
        full = plan_of(lib, fake_args(c))
        got = plan_of(lib, fake_args(c, n_seq=0))
        if full[0] == 0:
            assert got == (0, C['LIME_ATTN_NONE'], 0, []), c['id']
        else:
            assert got[0] == full[0], c['id']                              # refused, or not applicable, whatever the count
    assert plan_of(lib, fake_args(by_id['vocab_empty'], n_seq=0))[0] == (0 if mode & 1 else C['LIME_NOT_APPLICABLE'])
    assert plan_of(lib, fake_args(by_id['vocab_empty_s96'], n_seq=0))[0] == C['LIME_NOT_APPLICABLE']
    assert plan_of(lib, fake_args(by_id['plain_empty_s513'], n_seq=0))[0] == C['LIME_ERR_UNSUPPORTED']
    assert plan_of(lib, fake_args(by_id['plain_empty_w64'], n_seq=0)) == (0, C['LIME_ATTN_NONE'], 0, [])


def test_plan_rejects_a_missing_block(lib):
    plan = _lib.TokenAttentionPlan()
    assert lib.lime_token_attention_plan_f32(None, ctypes.byref(plan)) == -1
    assert b'lime_token_attention_plan_f32: args is NULL' in lib.lime_last_error_string()
    a = fake_args(arc.CASES[0])
    assert lib.lime_token_attention_plan_f32(ctypes.byref(a), None) == -1
    a.form = 6
    assert lib.lime_token_attention_plan_f32(ctypes.byref(a), ctypes.byref(plan)) == -1


def test_the_run_entry_refuses_a_missing_block_before_any_launch(lib):
    """lime_token_attention_f32 over nothing that could launch: no block, a form outside the enum, and all-zero blocks, which every
    form's first check (the operands) refuses under the form's own name."""
    assert lib.lime_token_attention_f32(None, None) == C['LIME_ERR_BAD_ARG']
    assert b'lime_token_attention_f32: args is NULL' in lib.lime_last_error_string()
    for form in (-1, 6):
        a = _lib.TokenAttentionArgs()
        a.form = form
        assert lib.lime_token_attention_f32(ctypes.byref(a), None) == C['LIME_ERR_BAD_ARG']
        assert lib.lime_last_error_string().decode() == 'lime_token_attention_f32: form %d' % form
    names = {'plain': 'count', 'count': 'count', 'lse': 'lse', 'rows': 'rows', 'vocab': 'vocab', 'dropout': 'dropout'}
    for form in arc.FORMS:
        a = _lib.TokenAttentionArgs()
        a.form = _lib.ATTN_FORM[form]
        assert lib.lime_token_attention_f32(ctypes.byref(a), None) == C['LIME_ERR_BAD_ARG'], form
        assert lib.lime_last_error_string().decode() == 'lime_token_attention_%s_f32: %s pointer' % (
            names[form], 'null' if form == 'dropout' else 'NULL'), form
