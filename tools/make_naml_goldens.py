"""Generate the NAML content encoder's goldens (tests/golden/naml_*.npz forward taps, grad_naml_*.npz gradients) by running the
IMPORTED REFERENCE on CPU (build container only), for the cases of tests/naml_cases.py.

    python tools/make_naml_goldens.py [case ...]

The forward and gradient procedures are those of tools/make_goldens.py and tools/make_grad_goldens.py (reused, with the case table
swapped for naml_cases): ``model.eval(); model.training = True`` keeps every child in eval mode (no dropout) while ``Model.forward``
takes the [B, K] training shape; the loss is the trainer's negative_log_softmax (trainer.py:71-73).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import naml_cases  # noqa: E402
import make_goldens  # noqa: E402
import make_grad_goldens  # noqa: E402


def main():
    # both tools look their cases up through golden_cases.build_case: point it at the NAML table for this run
    make_goldens.golden_cases.build_case = naml_cases.build_case
    make_grad_goldens.golden_cases.build_case = naml_cases.build_case
    # NAML has twice CNN's large tensors (two convolutions, two word attentions): keep fewer entries each, so a file stays near the
    # size of the CNN ones
    make_grad_goldens.KEEP = 1024
    outdir = os.path.join(ROOT, 'tests', 'golden')
    for name in sys.argv[1:] or list(naml_cases.CASES):
        arrays = make_goldens.run_case(name)
        path = os.path.join(outdir, name + '.npz')
        np.savez_compressed(path, **arrays)
        print('%-20s %7.1f KB  logits[0]=%s  %d state-dict keys' % (name, os.path.getsize(path) / 1024.0, arrays['logits'].reshape(-1)[:3],
                                                                   len(json.loads(str(arrays['state_dict_spec'])))))
        if name in naml_cases.GRAD_CASES:
            arrays = make_grad_goldens.run_case(name)
            path = os.path.join(outdir, 'grad_' + name + '.npz')
            np.savez_compressed(path, **arrays)
            print('%-20s %7.1f KB  loss %.6f  %d tensors with grad, %d without' % (
                'grad_' + name, os.path.getsize(path) / 1024.0, float(arrays['loss']), len(json.loads(str(arrays['with_grad']))),
                len(json.loads(str(arrays['without_grad'])))))


if __name__ == '__main__':
    main()
