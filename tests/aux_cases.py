"""Golden-vector cases of the category-prediction loss of the bare CROWN baselines (``config.alpha``, reference newsEncoders.py:358-364,
trainer.py:137-139), in the structure of plain_cases.CASES and built from the same generator (``golden_cases.EDITS`` / ``WEIGHT_SEED`` /
lime_cikm25_amd.synth).  tools/make_aux_goldens.py runs the imported reference on them with the loss
``nll + model.news_encoder.auxiliary_loss.mean()`` where the attribute is not None; tests/test_aux_loss_*.py regenerate the same inputs
and weights.  Only outputs are stored (tests/golden/grad_aux_*.npz).

The figure beside a case is what the guard of tools/make_grad_goldens.py printed for the seed it has: the worst relative gap between the
reference's fp32 gradients and its own fp64 ones, which has to stay under half of the check's 1e-3 (it moves a little with the thread
count of the run)."""
from lime_cikm25_amd.config import make_config
from lime_cikm25_amd import synth

import golden_cases
import plain_cases

EDITS = golden_cases.EDITS
WEIGHT_SEED = golden_cases.WEIGHT_SEED

_CFG1 = plain_cases._CFG1
_TINY = plain_cases._TINY

CASES = {
    # the original CROWN with its recipe's loss: the term is alpha x the mean over the B H = 24 history rows
    # (guard: 7.1e-5, word_embedding.weight)
    'aux_crown_crown': dict(cfg=dict(news_encoder='CROWN', user_encoder='CROWN', alpha=0.3, **_TINY), B=4, N=3, seed=501, eval_shape=False,
                            edit='none'),
    # the ATT user encoder re-invokes the news encoder at userEncoders.py:548; B H = 80 rows
    # (guard: 2.3e-4, word_embedding.weight)
    'aux_crown_att': dict(cfg=dict(news_encoder='CROWN', user_encoder='ATT', alpha=0.3, **_CFG1), B=8, N=2, seed=502, eval_shape=False,
                          edit='none'),
    # MHSA at userEncoders.py:475, with the weight at 1
    # (seeds 503 and 603 leave a residue of 6.3e-8 and 4.1e-8 on the self-attention's key bias, an identically-zero gradient of which the
    # check resolves 1e-8; 703 passes: 1.4e-4, user_encoder.multiheadAttention.W_K.weight)
    'aux_crown_mhsa': dict(cfg=dict(news_encoder='CROWN', user_encoder='MHSA', alpha=1.0, **_TINY), B=4, N=3, seed=703, eval_shape=False,
                           edit='none'),
    # rows whose history is all padding: every slot of them counts in the mean, with category 0
    # (guard: 7.9e-5, word_embedding.weight)
    'aux_crown_crown_empty_history': dict(cfg=dict(news_encoder='CROWN', user_encoder='CROWN', alpha=0.3, **_TINY), B=4, N=2, seed=504,
                                          eval_shape=False, edit='empty_history'),
    # under LIME the wrapper's attribute is the None it copied at construction (newsEncoders.py:100-103): no term, no fc gradient
    # (guard: 4.8e-5, word_embedding.weight)
    'aux_lime_crown_crown': dict(cfg=dict(news_encoder='LIME', content_encoder='CROWN', user_encoder='CROWN', alpha=0.3, **_TINY), B=4, N=2,
                                 seed=505, eval_shape=False, edit='none'),
}

BARE_CASES = tuple(n for n in CASES if n != 'aux_lime_crown_crown')
FC = ('news_encoder.category_predictor.fc.weight', 'news_encoder.category_predictor.fc.bias')


def build_case(name, seed=None):
    """-> (config, OrderedDict of the 26 inputs, case dict).  ``seed``: another batch seed than the case's (the golden tool's probe)."""
    c = CASES[name]
    seed = c['seed'] if seed is None else seed
    cfg = make_config(**c['cfg'])
    batch = synth.make_batch(cfg, c['B'], c['N'], seed=seed, eval_shape=c['eval_shape'])
    batch = EDITS[c['edit']](cfg, batch)
    return cfg, batch, c
