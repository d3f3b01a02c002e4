"""Generate tests/golden/grad_*.npz: loss and parameter gradients of one training step's forward + backward, by running
the IMPORTED REFERENCE on CPU (build container only) -- the pin of SURVEY.md section 8f row 2.

    python tools/make_grad_goldens.py

The reference model is built as in tools/make_goldens.py; ``model.eval(); model.training = True`` keeps every child in
eval mode (no dropout: the gradients are deterministic) while ``Model.forward`` takes the [B, K] training shape.  The loss
is the trainer's ``negative_log_softmax`` (trainer.py:71-73).  Stored per parameter that received a gradient: the whole
tensor when it has at most 2048 elements, else its 2048 largest-magnitude entries (flat indices + values), plus the L2 norm
and the sum; and the names whose ``.grad`` stayed None.  The ablation cases keep 512 entries per large tensor.

Two guards stand between the reference's run and a golden file (``guard``; tools/make_user_goldens.py uses the same ones): the
yardstick has to be good for more than it asks (``reference_double_error``), and a golden must not reject the exact value of an
identically-zero gradient (``check_zero_gradients``).
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
from lime_cikm25_amd import synth  # noqa: E402
import golden_cases  # noqa: E402

CASES = ('cfg1_crown', 'cfg1_mhsa', 'spill', 'empty_history', 'full_len', 'long_body', 'two_layers') + golden_cases.ABLATION_GRAD_CASES
KEEP = 2048
KEEP_SMALL = 512            # per large tensor of the cases in SMALL_CASES: their files stay well under the largest one committed
SMALL_CASES = golden_cases.ABLATION_GRAD_CASES
TOL = 1e-3                  # the gradient check's tolerance (tests/test_training_gpu.py, compare_grads)
# The gradient of a softmax attention's key bias is identically zero (a constant added to every key's score of a query leaves the
# softmax alone): what the reference stores there is its own rounding residue.  The gradient check (compare_grads: 1e-3 relative,
# floor 1e-5) resolves 1e-8 absolute on such a tensor, so a golden whose residue reaches that rejects the exact gradient itself
# and is refused here: pick another batch seed for the case (tests/user_cases.py says where that was done).
ZERO_GRADIENTS = ('multiheadAttention.W_K.bias', 'candidate_aware_attn.key_proj.bias')
RESOLUTION = TOL * 1e-5
# Goldens committed before the fp64 yardstick existed whose reference run is above half of TOL from its own fp64 gradients (measured
# with 16 threads: cfg1_mhsa 5.9e-4 on base_news_encoder.attention.affine1.bias, spill 1.2e-3 on word_embedding.weight).  ``guard``
# reports them and lets them through, so that this tool still reproduces every committed file; a new case gets no such entry.
# Moving them to other batch seeds rewrites their forward goldens too and is a change of its own.
ABOVE_HALF_TOL = ('cfg1_mhsa', 'spill')


def _reference_model(cfg):
    torch.manual_seed(0)
    model = ref_harness.build_reference_model(cfg, synth.synth_word_embedding(cfg, golden_cases.WEIGHT_SEED))
    model.initialize()
    synth.fill_state_dict(model, golden_cases.WEIGHT_SEED)
    model.eval()
    model.training = True
    return model


def training_loss(model, logits):
    """The loss a case differentiates: the trainer's ``negative_log_softmax`` (trainer.py:71-73).  A tool whose cases train with more
    than that swaps this function (tools/make_aux_goldens.py adds trainer.py:137-139's auxiliary loss); ``run_case`` and the guard's two
    runs both go through it."""
    return (-torch.log_softmax(logits, dim=1).select(dim=1, index=0)).mean()


def reference_double_error(name):
    """How far the reference's fp32 gradients are from the reference's own fp64 gradients, by compare_grads' measure over every entry
    (|a - b| / max(|a|, rms(a), 1e-5), a the fp32 gradient): -> (parameter, worst).  What this reaches is not left for an implementation.
    The ZERO_GRADIENTS tensors are left out: their exact value is zero, both runs hold rounding residue alone, and how much of it a
    golden may carry is ``check_zero_gradients``' question (its bound, 1e-8 absolute, is 1e-3 by this measure -- the two would
    contradict each other on the same numbers)."""
    cfg, batch, case = golden_cases.build_case(name)

    def grads(double):
        model = _reference_model(cfg)
        b = batch
        if double:
            model = model.double()
            b = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
        logits = model(*b.values())
        training_loss(model, logits).backward()
        out, seen = {}, set()
        for k, p in model.named_parameters():
            if id(p) not in seen and p.grad is not None:
                out[k] = p.grad.detach().double().reshape(-1).numpy()
            seen.add(id(p))
        return out

    g32, g64 = grads(False), grads(True)
    worst = ('', 0.0)
    for k, a in g32.items():
        if k.endswith(ZERO_GRADIENTS):
            continue
        floor = max(float(np.linalg.norm(a)) / max(1.0, a.size) ** 0.5, 1e-5)
        e = float(np.max(np.abs(g64[k] - a) / np.maximum(np.abs(a), floor)))
        if e > worst[1]:
            worst = (k, e)
    return worst


def check_zero_gradients(name, arrays):
    for k in json.loads(str(arrays['with_grad'])):
        if k.endswith(ZERO_GRADIENTS):
            # (a tensor above KEEP entries is stored as its largest-magnitude entries: their maximum is the tensor's)
            residue = float(np.abs(arrays['full:' + k] if 'full:' + k in arrays else arrays['val:' + k]).max())
            if residue >= RESOLUTION:
                raise ValueError("%s: the reference's residue on %s is %.2e, at or above the %.0e the gradient check resolves: the exact "
                                 "gradient (zero) would fail this golden" % (name, k, residue, RESOLUTION))


def guard(name, arrays):
    """Refuse (ValueError) a gradient golden that asks more than the reference itself delivers; -> (parameter, worst) of
    ``reference_double_error`` for the caller to print.  The value moves a little with the thread count of the run."""
    check_zero_gradients(name, arrays)
    k, worst = reference_double_error(name)
    if worst > 0.5 * TOL and name in ABOVE_HALF_TOL:
        print("%-18s NOTE: %.2e on %s is above half of the %.0e the gradient check allows (listed in ABOVE_HALF_TOL)" % (name, worst, k, TOL))
    elif worst > 0.5 * TOL:
        raise ValueError("%s: the reference's fp32 gradient of %s is %.2e from its own fp64 gradient, above half of the %.0e the gradient "
                         "check allows: pick another batch seed for the case" % (name, k, worst, TOL))
    return k, worst


def run_case(name):
    cfg, batch, case = golden_cases.build_case(name)
    assert not case['eval_shape']
    keep = KEEP_SMALL if name in SMALL_CASES else KEEP
    model = _reference_model(cfg)
    logits = model(*batch.values())
    loss = training_loss(model, logits)
    loss.backward()
    out = {'loss': loss.detach().numpy(), 'logits': logits.detach().numpy()}
    with_grad, without = [], []
    seen = set()
    for k, p in model.named_parameters():
        if id(p) in seen:
            continue
        seen.add(id(p))
        if p.grad is None:
            without.append(k)
            continue
        with_grad.append(k)
        g = p.grad.detach().reshape(-1)
        out['norm:' + k] = g.double().norm().numpy()
        out['sum:' + k] = g.double().sum().numpy()
        if g.numel() <= keep:
            out['full:' + k] = p.grad.detach().numpy()
        else:
            idx = torch.topk(g.abs(), keep).indices.sort().values
            out['idx:' + k] = idx.numpy()
            out['val:' + k] = g[idx].numpy()
    out['with_grad'] = np.array(json.dumps(with_grad))
    out['without_grad'] = np.array(json.dumps(without))
    return out


def main():
    outdir = os.path.join(ROOT, 'tests', 'golden')
    for name in sys.argv[1:] or CASES:
        arrays = run_case(name)
        print("%-18s the reference's fp32 gradients against its own fp64 ones: worst %s %.2e" % ((name,) + guard(name, arrays)))
        path = os.path.join(outdir, 'grad_' + name + '.npz')
        np.savez_compressed(path, **arrays)
        print('%-18s %7.1f KB  loss %.6f  %d tensors with grad, %d without' % (
            name, os.path.getsize(path) / 1024.0, float(arrays['loss']), len(json.loads(str(arrays['with_grad']))),
            len(json.loads(str(arrays['without_grad'])))))


if __name__ == '__main__':
    main()
