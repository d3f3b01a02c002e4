"""Generate the CNE content encoder's goldens (tests/golden/cne_*.npz forward taps, grad_cne_*.npz gradients) by running the
IMPORTED REFERENCE on CPU (build container only), for the cases of tests/cne_cases.py.

    python tools/make_cne_goldens.py [case ...]

The forward and gradient procedures are those of tools/make_goldens.py and tools/make_grad_goldens.py (reused, with the case table
swapped for cne_cases): ``model.eval(); model.training = True`` keeps every child in eval mode (no dropout) while ``Model.forward``
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

import torch  # noqa: E402

import cne_cases  # noqa: E402
import make_goldens  # noqa: E402
import make_grad_goldens  # noqa: E402
import ref_harness  # noqa: E402
from lime_cikm25_amd import synth  # noqa: E402


def run_forward(name):
    """make_goldens.run_case for a user encoder without GraphSAGE (its hooks name the CROWN user encoder's modules): the taps the CNE
    tests read -- logits, news_representation, the content encoder's output for candidates and history, user_representation."""
    cfg, batch, case = cne_cases.build_case(name)
    torch.manual_seed(0)
    model = ref_harness.build_reference_model(cfg, synth.synth_word_embedding(cfg, cne_cases.WEIGHT_SEED))
    model.initialize()
    synth.fill_state_dict(model, cne_cases.WEIGHT_SEED)
    model.eval()
    if not case['eval_shape']:
        model.training = True          # children stay in eval mode
    taps = {}

    def tap(key):
        def hook(_m, _inp, out):
            taps.setdefault(key, []).append(out)
        return hook

    ne = model.news_encoder
    hooks = [ne.register_forward_hook(tap('news_out')), ne.base_news_encoder.register_forward_hook(tap('content')),
             model.user_encoder.register_forward_hook(tap('user_representation'))]
    with torch.no_grad():
        logits = model(*batch.values())
    for h in hooks:
        h.remove()
    out = {'logits': logits, 'news_representation': taps['news_out'][0], 'cand_content': taps['content'][0],
           'hist_content': taps['content'][1][:make_goldens.HIST_ROWS], 'user_representation': taps['user_representation'][0]}
    arrays = {k: v.detach().cpu().numpy().copy() for k, v in out.items()}
    arrays['state_dict_spec'] = np.array(json.dumps([[k, list(v.shape)] for k, v in model.state_dict().items()]))
    arrays['trainable'] = np.array(json.dumps(sorted(k for k, p in model.named_parameters() if p.requires_grad)))
    return arrays


def stable_length_sort():
    """The reference sorts titles and bodies by length (newsEncoders.py:496-499) with torch's default sort and pairs them by sorted
    position, so the order of TIED lengths decides which news gates which -- and the default sort leaves that order to the build (the
    CPU one is unstable above 16 elements, a CUDA run orders ties differently again).  The goldens pin the defined behaviour: ties in
    input order.  For the run of the reference every torch.sort is made stable (no effect on sorts without ties)."""
    plain = torch.sort

    def sort(input, *args, **kwargs):
        kwargs['stable'] = True
        return plain(input, *args, **kwargs)
    torch.sort = sort


def main():
    stable_length_sort()
    # both tools look their cases up through golden_cases.build_case: point it at the CNE table for this run
    make_goldens.golden_cases.build_case = cne_cases.build_case
    make_grad_goldens.golden_cases.build_case = cne_cases.build_case
    # CNE has a dozen large tensors (two LSTMs of four matrices, four gate matrices, four attentions): keep fewer entries each, so no
    # file is larger than the largest NAML one
    make_grad_goldens.KEEP = 512
    outdir = os.path.join(ROOT, 'tests', 'golden')
    for name in sys.argv[1:] or list(cne_cases.CASES):
        arrays = make_goldens.run_case(name) if cne_cases.CASES[name]['cfg'].get('user_encoder', 'CROWN') == 'CROWN' else run_forward(name)
        path = os.path.join(outdir, name + '.npz')
        np.savez_compressed(path, **arrays)
        print('%-20s %7.1f KB  logits[0]=%s  %d state-dict keys' % (name, os.path.getsize(path) / 1024.0, arrays['logits'].reshape(-1)[:3],
                                                                   len(json.loads(str(arrays['state_dict_spec'])))))
        if name in cne_cases.GRAD_CASES:
            arrays = make_grad_goldens.run_case(name)
            # refuses a golden that asks more than the reference delivers (pick another batch seed in cne_cases then)
            print("%-20s the reference's fp32 gradients against its own fp64 ones: worst %s %.2e" % ((name,) + make_grad_goldens.guard(name, arrays)))
            path = os.path.join(outdir, 'grad_' + name + '.npz')
            np.savez_compressed(path, **arrays)
            print('%-20s %7.1f KB  loss %.6f  %d tensors with grad, %d without' % (
                'grad_' + name, os.path.getsize(path) / 1024.0, float(arrays['loss']), len(json.loads(str(arrays['with_grad']))),
                len(json.loads(str(arrays['without_grad'])))))


if __name__ == '__main__':
    main()
