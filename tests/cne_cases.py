"""Golden-vector cases of the CNE content encoder (LIME-CNE-CROWN / -ATT), in the structure of golden_cases.CASES and built from the
same generator (``golden_cases.EDITS`` / ``WEIGHT_SEED`` / lime_cikm25_amd.synth).  tools/make_cne_goldens.py runs the imported
reference on them; tests/test_cne_*.py regenerate the same inputs and weights.  Only outputs are stored (tests/golden/cne_*.npz,
grad_cne_*.npz)."""
from lime_cikm25_amd.config import make_config
from lime_cikm25_amd import synth

import golden_cases

EDITS = golden_cases.EDITS
WEIGHT_SEED = golden_cases.WEIGHT_SEED

_SMALL = dict(vocabulary_size=5000, category_num=18, subCategory_num=270, content_encoder='CNE')
_TINY = dict(max_history_num=6, max_title_length=8, max_abstract_length=16, batch_size=4, **_SMALL)

CASES = {
    # two unit tiles of 16 per direction
    'cne_small': dict(cfg=dict(hidden_dim=32, **_TINY), B=4, N=2, seed=61, eval_shape=False, edit='none'),
    # the default hidden size (25 unit tiles of 16); padding news of length 1 and all-padding history rows
    'cne_h400_empty_history': dict(cfg=dict(**_TINY), B=4, N=2, seed=62, eval_shape=False, edit='empty_history'),
    # a hidden size that is no multiple of 32, the full 32- and 128-step recurrences
    'cne_body128': dict(cfg=dict(hidden_dim=48, max_history_num=3, max_title_length=32, max_abstract_length=128, batch_size=2, **_SMALL),
                        B=2, N=2, seed=63, eval_shape=False, edit='none'),
    # the content encoder under a second user encoder
    'cne_att': dict(cfg=dict(hidden_dim=32, user_encoder='ATT', **_TINY), B=4, N=2, seed=66, eval_shape=False, edit='none'),
    # the reference's eval path (one candidate per row, no N axis): forward only
    'cne_eval': dict(cfg=dict(hidden_dim=32, **_TINY), B=4, N=1, seed=65, eval_shape=True, edit='none'),
}

GRAD_CASES = ('cne_small', 'cne_h400_empty_history', 'cne_body128', 'cne_att')


def build_case(name):
    """-> (config, OrderedDict of the 26 inputs, case dict)."""
    c = CASES[name]
    cfg = make_config(**c['cfg'])
    batch = synth.make_batch(cfg, c['B'], c['N'], seed=c['seed'], eval_shape=c['eval_shape'])
    batch = EDITS[c['edit']](cfg, batch)
    return cfg, batch, c
