"""Generate the goldens of the ATT and MHSA user encoders (tests/golden/user_*.npz forward taps, grad_user_*.npz gradients) by running
the IMPORTED REFERENCE on CPU (build container only), for the cases of tests/user_cases.py.

    python tools/make_user_goldens.py [case ...]

The procedure is that of tools/make_goldens.py -- ``model.eval(); model.training = True`` keeps every child in eval mode (no dropout)
while ``Model.forward`` takes the [B, K] training shape -- with the taps of these user encoders (no GraphSAGE to hook); the gradients
come from tools/make_grad_goldens.py with the case table swapped.  Only outputs are stored.
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
import user_cases  # noqa: E402
import make_grad_goldens  # noqa: E402
from lime_cikm25_amd import synth  # noqa: E402

HIST_ROWS = 2   # history-level tensors are stored for the first rows only (fixture size)


def run_case(name):
    cfg, batch, case = user_cases.build_case(name)
    torch.manual_seed(0)
    model = ref_harness.build_reference_model(cfg, synth.synth_word_embedding(cfg, user_cases.WEIGHT_SEED))
    model.initialize()
    synth.fill_state_dict(model, user_cases.WEIGHT_SEED)
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


def main():
    make_grad_goldens.golden_cases.build_case = user_cases.build_case
    make_grad_goldens.KEEP = 512          # per large tensor: a file stays well under the size of the CROWN gradient goldens
    outdir = os.path.join(ROOT, 'tests', 'golden')
    for name in sys.argv[1:] or list(user_cases.CASES):
        arrays = run_case(name)
        path = os.path.join(outdir, name + '.npz')
        np.savez_compressed(path, **arrays)
        print('%-26s %7.1f KB  logits[0]=%s  %d state-dict keys' % (name, os.path.getsize(path) / 1024.0, arrays['logits'].reshape(-1)[:3],
                                                                   len(json.loads(str(arrays['state_dict_spec'])))))
        if name in user_cases.GRAD_CASES:
            arrays = make_grad_goldens.run_case(name)
            # the guards of tools/make_grad_goldens.py: the zero-gradient residue, and the reference against its own fp64 gradients
            print("%-26s the reference's fp32 gradients against its own fp64 ones: worst %s %.2e" % (
                ('grad_' + name,) + make_grad_goldens.guard(name, arrays)))
            path = os.path.join(outdir, 'grad_' + name + '.npz')
            np.savez_compressed(path, **arrays)
            print('%-26s %7.1f KB  loss %.6f  %d tensors with grad, %d without' % (
                'grad_' + name, os.path.getsize(path) / 1024.0, float(arrays['loss']), len(json.loads(str(arrays['with_grad']))),
                len(json.loads(str(arrays['without_grad'])))))


if __name__ == '__main__':
    main()
