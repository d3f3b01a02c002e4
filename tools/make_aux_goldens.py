"""Generate the gradient goldens of the category-prediction loss (tests/golden/grad_aux_*.npz) by running the IMPORTED REFERENCE on CPU
(build container only), for the cases of tests/aux_cases.py.

    python tools/make_aux_goldens.py [case ...]
    python tools/make_aux_goldens.py --probe case [...]     # the guard's figure for the case's seed, seed + 100, ... to the first pass

The procedure is tools/make_grad_goldens.py's with the case table swapped and the trainer's whole loss (trainer.py:131-139):
``nll + model.news_encoder.auxiliary_loss.mean()`` when the attribute is not None after the forward -- in ``run_case`` and in both runs
of the guard, which applies unchanged.  Stored, outputs only: what ``make_grad_goldens.run_case`` stores (``loss`` is the sum), ``nll``,
``aux`` (the attribute; ``aux_none`` says it was None and ``aux`` is then 0) and ``aux_candidates``: alpha x the value of the
predictor's FIRST call of the forward, the one on the candidate rows (model.py:171), which the history call overwrites
(userEncoders.py:110) -- stored so that a test can show it is NOT the term."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import aux_cases  # noqa: E402
import make_grad_goldens  # noqa: E402

_nll = make_grad_goldens.training_loss


def training_loss(model, logits):
    aux = model.news_encoder.auxiliary_loss                            # trainer.py:137-139
    return _nll(model, logits) if aux is None else _nll(model, logits) + aux.mean()


def run_case(name):
    cfg, batch, _ = aux_cases.build_case(name)
    arrays = make_grad_goldens.run_case(name)
    # the forward once more, without a backward: the two parts of the loss and the value of each predictor call
    model = make_grad_goldens._reference_model(cfg)
    enc = getattr(model.news_encoder, 'base_news_encoder', model.news_encoder)
    calls = []
    hook = enc.category_predictor.register_forward_hook(lambda _m, inp, out: calls.append((int(inp[0].shape[0]), float(out))))
    with torch.no_grad():
        logits = model(*batch.values())
    hook.remove()
    B, N = batch['news_category'].shape
    H = batch['user_category'].shape[1]
    assert [rows for rows, _ in calls] == [B * N, B * H], calls
    aux = model.news_encoder.auxiliary_loss
    arrays['nll'] = _nll(model, logits).numpy()
    arrays['aux_none'] = np.array(aux is None)
    arrays['aux'] = np.array(0.0 if aux is None else float(aux), dtype=np.float32)
    arrays['aux_candidates'] = np.array(cfg.alpha * calls[0][1], dtype=np.float32)
    total = float(arrays['nll']) + float(arrays['aux'])
    assert abs(total - float(arrays['loss'])) <= 1e-6 * max(1.0, abs(total)), (total, float(arrays['loss']))
    if aux is not None:
        assert abs(float(aux) - cfg.alpha * calls[1][1]) <= 1e-6 * abs(float(aux)), (float(aux), calls)
    return arrays


def probe(name, tries=12):
    """Print the guard's figure for the case's batch seed, seed + 100, ... and stop at the first seed that passes."""
    seed0 = aux_cases.CASES[name]['seed']
    for seed in range(seed0, seed0 + 100 * tries, 100):
        aux_cases.CASES[name]['seed'] = seed
        try:
            arrays = run_case(name)
            print('%-32s seed %4d: passes, worst %s %.2e' % ((name, seed) + make_grad_goldens.guard(name, arrays)))
            return seed
        except ValueError as e:
            print('%-32s seed %4d: refused -- %s' % (name, seed, e))
    raise SystemExit('%s: no seed passed' % name)


def main():
    make_grad_goldens.golden_cases.build_case = aux_cases.build_case
    make_grad_goldens.training_loss = training_loss
    make_grad_goldens.KEEP = 512          # per large tensor: a file stays about the size of the baselines' gradient goldens
    args = sys.argv[1:]
    if args and args[0] == '--probe':
        for name in args[1:] or list(aux_cases.CASES):
            probe(name)
        return
    outdir = os.path.join(ROOT, 'tests', 'golden')
    for name in args or list(aux_cases.CASES):
        arrays = run_case(name)
        print("%-32s the reference's fp32 gradients against its own fp64 ones: worst %s %.2e" % (
            ('grad_' + name,) + make_grad_goldens.guard(name, arrays)))
        path = os.path.join(outdir, 'grad_' + name + '.npz')
        np.savez_compressed(path, **arrays)
        print('%-32s %7.1f KB  loss %.6f = nll %.6f + aux %s (candidates\' call: %.6f)  %d tensors with grad, %d without' % (
            'grad_' + name, os.path.getsize(path) / 1024.0, float(arrays['loss']), float(arrays['nll']),
            'None' if bool(arrays['aux_none']) else '%.6f' % float(arrays['aux']), float(arrays['aux_candidates']),
            len(json.loads(str(arrays['with_grad']))), len(json.loads(str(arrays['without_grad'])))))


if __name__ == '__main__':
    main()
