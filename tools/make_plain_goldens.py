"""Generate the goldens of the baseline models -- a content encoder as the news encoder itself, no LIME (tests/golden/plain_*.npz forward
taps, grad_plain_*.npz gradients) -- by running the IMPORTED REFERENCE on CPU (build container only), for the cases of
tests/plain_cases.py.

    python tools/make_plain_goldens.py [case ...]
    python tools/make_plain_goldens.py --probe case [...]     # the guard's figure for the case's seed, seed + 100, ... to the first pass

The procedure is that of tools/make_user_goldens.py -- ``model.eval(); model.training = True`` keeps every child in eval mode (no dropout)
while ``Model.forward`` takes the [B, K] training shape -- with the same taps; the gradients come from tools/make_grad_goldens.py with
the case table swapped, through its two guards.  KCNN gets the entity pickles and CPU ``device`` attributes of
tools/make_kcnn_goldens.py.  A third guard: a gradient golden in which a parameter's gradient is exactly zero pins nothing there and is
refused -- except the tensors whose gradient IS identically zero (make_grad_goldens.ZERO_GRADIENTS, and ``user_node_embedding`` when the
rows of the forward do not reach past the history slots).  Only outputs are stored.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ref_harness  # noqa: E402
import plain_cases  # noqa: E402
import make_grad_goldens  # noqa: E402
import make_kcnn_goldens  # noqa: E402
from lime_cikm25_amd import synth  # noqa: E402

HIST_ROWS = 2   # history-level tensors are stored for the first rows only (fixture size)
_plain_build = ref_harness.build_reference_model


def build_reference_model(config, word_embedding):
    if config.news_encoder == 'KCNN':
        return make_kcnn_goldens.build_reference_model(config, word_embedding)
    return _plain_build(config, word_embedding)


def run_case(name):
    cfg, batch, case = plain_cases.build_case(name)
    torch.manual_seed(0)
    model = build_reference_model(cfg, synth.synth_word_embedding(cfg, plain_cases.WEIGHT_SEED))
    assert model.model_name == '%s-%s' % (cfg.news_encoder, cfg.user_encoder)
    model.initialize()
    synth.fill_state_dict(model, plain_cases.WEIGHT_SEED)
    model.eval()
    if not case['eval_shape']:
        model.training = True          # children stay in eval mode
    taps = {}

    def tap(key):
        def hook(_m, _inp, out):
            taps.setdefault(key, []).append(out)
        return hook

    ue = model.user_encoder
    hooks = [model.news_encoder.register_forward_hook(tap('news_out')), ue.register_forward_hook(tap('user_representation'))]
    if cfg.use_candidate_ware_clicked_news_attention:
        hooks.append(ue.candidate_aware_attn.register_forward_hook(tap('cand_aware')))
    if cfg.user_encoder == 'MHSA':
        hooks.append(ue.multiheadAttention.register_forward_hook(tap('self_attention')))
        hooks.append(ue.affine.register_forward_hook(tap('affine')))
    with torch.no_grad():
        logits = model(*batch.values())
    for h in hooks:
        h.remove()
    # the candidates' call of the news encoder comes first (model.py:171), the history's second (userEncoders.py:110)
    out = {'logits': logits, 'news_representation': taps['news_out'][0], 'user_representation': taps['user_representation'][0]}
    if 'cand_aware' in taps:
        out['hist_refined'] = taps['cand_aware'][0][0][:HIST_ROWS]
        out['attn_weights_agg'] = taps['cand_aware'][0][1]
    if 'self_attention' in taps:
        out['self_attention'] = taps['self_attention'][0][:HIST_ROWS]
        # the hook sees affine's output before the in-place dropout (off: eval children) and ReLU of userEncoders.py:487
        out['post_affine'] = torch.relu(taps['affine'][0][:HIST_ROWS])
    arrays = {k: v.detach().cpu().numpy().copy() for k, v in out.items()}
    arrays['state_dict_spec'] = np.array(json.dumps([[k, list(v.shape)] for k, v in model.state_dict().items()]))
    arrays['trainable'] = np.array(json.dumps(sorted(k for k, p in model.named_parameters() if p.requires_grad)))
    return arrays


def check_pins_something(name, arrays):
    cfg, _, case = plain_cases.build_case(name)
    for k in json.loads(str(arrays['with_grad'])):
        if float(arrays['norm:' + k]) > 0.0 or k.endswith(make_grad_goldens.ZERO_GRADIENTS):
            continue
        if k.endswith('user_node_embedding') and case['B'] <= cfg.max_history_num:
            continue                               # the GraphSAGE mean runs over history slots alone: identically zero
        raise ValueError('%s: the reference gradient of %s is exactly zero: the golden would pin nothing there' % (name, k))


def probe(name, tries=12):
    """Print the guard's figure for the case's batch seed, seed + 100, ... and stop at the first seed that passes every guard."""
    seed0 = plain_cases.CASES[name]['seed']
    for seed in range(seed0, seed0 + 100 * tries, 100):
        plain_cases.CASES[name]['seed'] = seed
        try:
            arrays = make_grad_goldens.run_case(name)
            check_pins_something(name, arrays)
            print('%-34s seed %4d: passes, worst %s %.2e' % ((name, seed) + make_grad_goldens.guard(name, arrays)))
            return seed
        except ValueError as e:
            print('%-34s seed %4d: refused -- %s' % (name, seed, e))
    raise SystemExit('%s: no seed passed' % name)


def main():
    ref_harness.build_reference_model = build_reference_model          # tools/make_grad_goldens.py builds its models through it
    make_grad_goldens.golden_cases.build_case = plain_cases.build_case
    make_grad_goldens.KEEP = 512          # per large tensor: a file stays about the size of the user-encoder gradient goldens
    args = sys.argv[1:]
    if args and args[0] == '--probe':
        for name in args[1:] or list(plain_cases.GRAD_CASES):
            probe(name)
        return
    outdir = os.path.join(ROOT, 'tests', 'golden')
    for name in args or list(plain_cases.CASES):
        arrays = run_case(name)
        path = os.path.join(outdir, name + '.npz')
        np.savez_compressed(path, **arrays)
        print('%-34s %7.1f KB  logits[0]=%s  %d state-dict keys' % (name, os.path.getsize(path) / 1024.0, arrays['logits'].reshape(-1)[:3],
                                                                   len(json.loads(str(arrays['state_dict_spec'])))))
        if name in plain_cases.GRAD_CASES:
            arrays = make_grad_goldens.run_case(name)
            check_pins_something(name, arrays)
            # the guards of tools/make_grad_goldens.py: the zero-gradient residue, and the reference against its own fp64 gradients
            print("%-34s the reference's fp32 gradients against its own fp64 ones: worst %s %.2e" % (
                ('grad_' + name,) + make_grad_goldens.guard(name, arrays)))
            path = os.path.join(outdir, 'grad_' + name + '.npz')
            np.savez_compressed(path, **arrays)
            print('%-34s %7.1f KB  loss %.6f  %d tensors with grad, %d without' % (
                'grad_' + name, os.path.getsize(path) / 1024.0, float(arrays['loss']), len(json.loads(str(arrays['with_grad']))),
                len(json.loads(str(arrays['without_grad'])))))


if __name__ == '__main__':
    main()
