"""Generate the goldens of the wide-head cases (tests/golden/wide_*.npz forward taps, grad_wide_*.npz gradients) by running the
IMPORTED REFERENCE on CPU (build container only), for the cases of tests/wide_head_cases.py.

    python tools/make_wide_head_goldens.py [case ...]

Nothing new is computed here: the case table is swapped into tools/make_goldens.py (CROWN user encoder: its GraphSAGE taps) or
tools/make_user_goldens.py (ATT / MHSA user encoders) for the forward taps and into tools/make_grad_goldens.py for the gradients, with
that tool's two guards in front of every gradient file.  Only outputs are stored.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import wide_head_cases  # noqa: E402
import make_goldens  # noqa: E402
import make_user_goldens  # noqa: E402
import make_grad_goldens  # noqa: E402


def main():
    # the three tools look their cases up through these two modules
    make_grad_goldens.golden_cases.build_case = wide_head_cases.build_case
    make_user_goldens.user_cases.build_case = wide_head_cases.build_case
    make_grad_goldens.KEEP = 512          # per large tensor: the files stay the size of the user-encoder gradient goldens
    outdir = os.path.join(ROOT, 'tests', 'golden')
    for name in sys.argv[1:] or list(wide_head_cases.CASES):
        cfg = wide_head_cases.build_case(name)[0]
        arrays = (make_goldens if cfg.user_encoder == 'CROWN' else make_user_goldens).run_case(name)
        path = os.path.join(outdir, name + '.npz')
        np.savez_compressed(path, **arrays)
        print('%-26s %7.1f KB  logits[0]=%s  %d state-dict keys' % (name, os.path.getsize(path) / 1024.0, arrays['logits'].reshape(-1)[:3],
                                                                   len(json.loads(str(arrays['state_dict_spec'])))))
        if name in wide_head_cases.GRAD_CASES:
            arrays = make_grad_goldens.run_case(name)
            print("%-26s the reference's fp32 gradients against its own fp64 ones: worst %s %.2e" % (
                ('grad_' + name,) + make_grad_goldens.guard(name, arrays)))
            path = os.path.join(outdir, 'grad_' + name + '.npz')
            np.savez_compressed(path, **arrays)
            print('%-26s %7.1f KB  loss %.6f  %d tensors with grad, %d without' % (
                'grad_' + name, os.path.getsize(path) / 1024.0, float(arrays['loss']), len(json.loads(str(arrays['with_grad']))),
                len(json.loads(str(arrays['without_grad'])))))


if __name__ == '__main__':
    main()
