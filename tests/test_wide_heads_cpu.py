"""Attention heads wider than 32 columns on the CPU: the models of tests/wide_head_cases.py (head_num 3 / 5, MHSA with head_dim 64 / 48) hold
the reference's state_dict key for key (tests/golden/wide_*.npz, tools/make_wide_head_goldens.py), the training step leaves out exactly
the parameters the reference's backward leaves without a gradient, and the kernels of csrc/token_attn_wide_f32.hip were compiled without
scratch.  No GPU."""
import json

import pytest

import wide_head_cases
from helpers import load_golden
from lime_cikm25_amd import Model, build, training


@pytest.mark.parametrize('name', list(wide_head_cases.CASES))
def test_state_dict_is_the_reference_one(name):
    cfg, _, _ = wide_head_cases.build_case(name)
    g = load_golden(name)
    model = Model(cfg)
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == json.loads(str(g['state_dict_spec']))
    assert sorted(k for k, p in model.named_parameters() if p.requires_grad) == sorted(json.loads(str(g['trainable'])))


@pytest.mark.parametrize('name', wide_head_cases.GRAD_CASES)
def test_dead_parameters_are_the_ones_the_reference_gives_no_gradient(name):
    cfg, _, _ = wide_head_cases.build_case(name)
    g = load_golden('grad_' + name)
    model = Model(cfg)
    without = json.loads(str(g['without_grad']))
    frozen = [k for k, p in dict(model.named_parameters()).items() if not p.requires_grad and k in without]
    assert sorted(training.dead_parameters(model) + frozen) == sorted(without)
    assert not set(training.dead_parameters(model)) & set(frozen)
    assert training.TrainStep.bucket_names(model) == json.loads(str(g['with_grad']))       # the reference's gradients, in its order


def test_wide_kernels_are_scratch_free():
    """Every head-width instantiation (48 .. 128 padded columns) of the three kernels, no scratch and no spilled register."""
    build.build_library()
    res = json.load(open(build.RESOURCES))
    assert res['source_hash'] == build.source_hash()
    unit = res['units']['token_attn_wide_f32']
    for kernel in ('wide_fwd_kernel', 'wide_bwd_q_kernel', 'wide_bwd_kv_kernel'):
        assert sum(1 for n in unit if n.startswith(kernel + '<')) == 6, kernel
    for name, r in unit.items():
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0, (name, r)
