"""Generate the goldens of the MLP click predictor (tests/golden/mlp_*.npz forward taps, grad_mlp_*.npz gradients) by running the
IMPORTED REFERENCE on CPU (build container only) with ``click_predictor='mlp'``, for the cases of tests/mlp_cases.py.

    python tools/make_mlp_goldens.py [case ...]

The procedure is that of tools/make_user_goldens.py -- ``model.eval(); model.training = True`` keeps every child in eval mode (no
dropout, ``Model.dropout`` included) while ``Model.forward`` takes the [B, K] training shape; the gradients come from
tools/make_grad_goldens.py with the case table swapped, through its guards.  One tensor is new to them: ``out.bias`` adds a constant to
every logit of a row, which the softmax loss does not feel, so its gradient is identically zero and the reference stores rounding
residue there.  It joins make_grad_goldens.ZERO_GRADIENTS by its full name (the fp32-against-fp64 guard then leaves it out, as it
leaves the key biases out), and its residue is printed and held to the bound the gradient test gives the implementation:
``zero_gradient_bound`` -- the number of logits times fp32's epsilon.  Only outputs are stored.
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
import mlp_cases  # noqa: E402
import make_grad_goldens  # noqa: E402
from lime_cikm25_amd import synth  # noqa: E402

HIST_ROWS = 2   # history-level tensors are stored for the first rows only (fixture size)


def zero_gradient_bound(n_logits):
    """What a gradient that is identically zero may hold in fp32 (tests/test_mlp_predictor_gpu.py states the derivation)."""
    return n_logits * float(np.finfo(np.float32).eps)


def run_case(name):
    cfg, batch, case = mlp_cases.build_case(name)
    torch.manual_seed(0)
    model = ref_harness.build_reference_model(cfg, synth.synth_word_embedding(cfg, mlp_cases.WEIGHT_SEED))
    assert model.click_predictor == 'mlp' and model.mlp.weight.shape == (model.news_embedding_dim // 2, 2 * model.news_embedding_dim)
    model.initialize()
    synth.fill_state_dict(model, mlp_cases.WEIGHT_SEED)
    model.eval()
    if not case['eval_shape']:
        model.training = True          # children stay in eval mode
    taps = {}

    def tap(key):
        def hook(_m, _inp, out):
            taps.setdefault(key, []).append(out)
        return hook

    hooks = [model.news_encoder.register_forward_hook(tap('news_out')), model.user_encoder.register_forward_hook(tap('user_representation'))]
    with torch.no_grad():
        logits = model(*batch.values())
    for h in hooks:
        h.remove()
    # the candidates' call of the news encoder comes first (model.py:171), the history's second (userEncoders.py:110)
    out = {'logits': logits, 'news_representation': taps['news_out'][0], 'user_representation': taps['user_representation'][0]}
    arrays = {k: v.detach().cpu().numpy().copy() for k, v in out.items()}
    arrays['state_dict_spec'] = np.array(json.dumps([[k, list(v.shape)] for k, v in model.state_dict().items()]))
    arrays['trainable'] = np.array(json.dumps(sorted(k for k, p in model.named_parameters() if p.requires_grad)))
    return arrays


def main():
    make_grad_goldens.golden_cases.build_case = mlp_cases.build_case
    make_grad_goldens.KEEP = 512          # per large tensor: a file stays about the size of the user-encoder gradient goldens
    outdir = os.path.join(ROOT, 'tests', 'golden')
    for name in sys.argv[1:] or list(mlp_cases.CASES):
        arrays = run_case(name)
        path = os.path.join(outdir, name + '.npz')
        np.savez_compressed(path, **arrays)
        print('%-28s %7.1f KB  logits[0]=%s  %d state-dict keys' % (name, os.path.getsize(path) / 1024.0, arrays['logits'].reshape(-1)[:3],
                                                                   len(json.loads(str(arrays['state_dict_spec'])))))
        if name in mlp_cases.GRAD_CASES:
            arrays = make_grad_goldens.run_case(name)
            # the key biases keep the guard of tools/make_grad_goldens.py; out.bias gets the bound of the gradient test
            make_grad_goldens.check_zero_gradients(name, arrays)
            residue = float(np.abs(arrays['full:' + mlp_cases.ZERO_GRADIENT]).max())
            bound = zero_gradient_bound(arrays['logits'].size)
            print("%-28s the reference's residue on %s: %.2e (bound %.2e)" % ('grad_' + name, mlp_cases.ZERO_GRADIENT, residue, bound))
            if residue > bound:
                raise ValueError('%s: the residue on %s is above the bound' % (name, mlp_cases.ZERO_GRADIENT))
            kept = make_grad_goldens.ZERO_GRADIENTS
            make_grad_goldens.ZERO_GRADIENTS = kept + (mlp_cases.ZERO_GRADIENT,)
            try:
                k, worst = make_grad_goldens.reference_double_error(name)
            finally:
                make_grad_goldens.ZERO_GRADIENTS = kept
            print("%-28s the reference's fp32 gradients against its own fp64 ones: worst %s %.2e" % ('grad_' + name, k, worst))
            if worst > 0.5 * make_grad_goldens.TOL:
                raise ValueError("%s: the reference's fp32 gradient of %s is %.2e from its own fp64 gradient, above half of the %.0e the "
                                 "gradient check allows: pick another batch seed for the case" % (name, k, worst, make_grad_goldens.TOL))
            path = os.path.join(outdir, 'grad_' + name + '.npz')
            np.savez_compressed(path, **arrays)
            print('%-28s %7.1f KB  loss %.6f  %d tensors with grad, %d without' % (
                'grad_' + name, os.path.getsize(path) / 1024.0, float(arrays['loss']), len(json.loads(str(arrays['with_grad']))),
                len(json.loads(str(arrays['without_grad'])))))


if __name__ == '__main__':
    main()
