"""Generate the CNN content encoder's goldens (tests/golden/cnn_*.npz forward taps, grad_cnn_*.npz gradients) by running the
IMPORTED REFERENCE on CPU (build container only), for the cases of tests/cnn_cases.py.

    python tools/make_cnn_goldens.py [case ...]

The forward and gradient procedures are those of tools/make_goldens.py and tools/make_grad_goldens.py (reused, with the case table
swapped for cnn_cases): ``model.eval(); model.training = True`` keeps every child in eval mode (no dropout) while ``Model.forward``
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

import cnn_cases  # noqa: E402
import make_goldens  # noqa: E402
import make_grad_goldens  # noqa: E402


def main():
    # both tools look their cases up through golden_cases.build_case: point it at the CNN table for this run
    make_goldens.golden_cases.build_case = cnn_cases.build_case
    make_grad_goldens.golden_cases.build_case = cnn_cases.build_case
    outdir = os.path.join(ROOT, 'tests', 'golden')
    for name in sys.argv[1:] or list(cnn_cases.CASES):
        arrays = make_goldens.run_case(name)
        path = os.path.join(outdir, name + '.npz')
        np.savez_compressed(path, **arrays)
        print('%-18s %7.1f KB  logits[0]=%s  %d state-dict keys' % (name, os.path.getsize(path) / 1024.0, arrays['logits'].reshape(-1)[:3],
                                                                   len(json.loads(str(arrays['state_dict_spec'])))))
        if name in cnn_cases.GRAD_CASES:
            arrays = make_grad_goldens.run_case(name)
            path = os.path.join(outdir, 'grad_' + name + '.npz')
            np.savez_compressed(path, **arrays)
            print('%-18s %7.1f KB  loss %.6f  %d tensors with grad, %d without' % (
                'grad_' + name, os.path.getsize(path) / 1024.0, float(arrays['loss']), len(json.loads(str(arrays['with_grad']))),
                len(json.loads(str(arrays['without_grad'])))))


if __name__ == '__main__':
    main()
