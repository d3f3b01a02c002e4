"""Golden-vector cases of the NAML content encoder (LIME-NAML-CROWN), in the structure of golden_cases.CASES and built from the same
generator (``golden_cases.EDITS`` / ``WEIGHT_SEED`` / lime_cikm25_amd.synth).  tools/make_naml_goldens.py runs the imported reference
on them; tests/test_naml_*.py regenerate the same inputs and weights.  Only outputs are stored (tests/golden/naml_*.npz,
grad_naml_*.npz)."""
from lime_cikm25_amd.config import make_config
from lime_cikm25_amd import synth

import golden_cases

EDITS = golden_cases.EDITS
WEIGHT_SEED = golden_cases.WEIGHT_SEED

_SMALL = dict(vocabulary_size=5000, category_num=18, subCategory_num=270, content_encoder='NAML')

CASES = {
    # BASELINE.json configs[0] shape (batch 8, history 10, title 16, body 32, K = 1+1), cnn_method 'naive', window 3
    'naml_naive': dict(cfg=dict(max_history_num=10, max_title_length=16, max_abstract_length=32, batch_size=8, **_SMALL),
                       B=8, N=2, seed=51, eval_shape=False, edit='none'),
    # three convolutions per text (windows 1 / 3 / 5, 100 outputs each) writing column slices of one output
    'naml_group3': dict(cfg=dict(cnn_method='group3', cnn_kernel_num=300, max_history_num=6, max_title_length=16, max_abstract_length=32,
                                 batch_size=4, **_SMALL),
                        B=4, N=3, seed=52, eval_shape=False, edit='none'),
    # window 5, 128-token bodies: one body sequence fills a whole 128-row tile of the fused attention pool
    'naml_w5_body128': dict(cfg=dict(cnn_window_size=5, max_history_num=3, max_title_length=32, max_abstract_length=128, batch_size=2,
                                     **_SMALL),
                            B=2, N=2, seed=53, eval_shape=False, edit='none'),
    # padding news and all-padding history rows
    'naml_empty_history': dict(cfg=dict(max_history_num=6, max_title_length=8, max_abstract_length=16, batch_size=4, **_SMALL),
                               B=4, N=2, seed=54, eval_shape=False, edit='empty_history'),
    # the reference's eval path (one candidate per row, no N axis): forward only
    'naml_eval': dict(cfg=dict(max_history_num=10, max_title_length=16, max_abstract_length=32, batch_size=8, **_SMALL),
                      B=8, N=1, seed=55, eval_shape=True, edit='none'),
}

GRAD_CASES = ('naml_naive', 'naml_group3', 'naml_w5_body128', 'naml_empty_history')


def build_case(name):
    """-> (config, OrderedDict of the 26 inputs, case dict)."""
    c = CASES[name]
    cfg = make_config(**c['cfg'])
    batch = synth.make_batch(cfg, c['B'], c['N'], seed=c['seed'], eval_shape=c['eval_shape'])
    batch = EDITS[c['edit']](cfg, batch)
    return cfg, batch, c
