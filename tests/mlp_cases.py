"""Golden-vector cases of the MLP click predictor (config.click_predictor = 'mlp'; reference model.py:113-115, :139-141, :182-184), in
the structure of golden_cases.CASES and built from the same generator (``golden_cases.EDITS`` / ``WEIGHT_SEED`` /
lime_cikm25_amd.synth).  tools/make_mlp_goldens.py runs the imported reference on them; tests/test_mlp_predictor_*.py regenerate the
same inputs and weights.  Only outputs are stored (tests/golden/mlp_*.npz, grad_mlp_*.npz).

The hidden layer is mlp: 2 D -> Dh = D // 2.  LIME: D = 400, Dh = 200; MHSA-MHSA (NRMS): D = 300, Dh = 150, an odd Dh / 2; CROWN-CROWN:
D = 900, Dh = 450.  The figure beside a gradient case is what the tool's guard printed for it: the reference's fp32 gradients against
its own fp64 ones (tools/make_grad_goldens.py), which has to stay under half of the gradient check's 1e-3."""
from lime_cikm25_amd.config import make_config
from lime_cikm25_amd import synth

import golden_cases

EDITS = golden_cases.EDITS
WEIGHT_SEED = golden_cases.WEIGHT_SEED

_SMALL = dict(vocabulary_size=5000, category_num=18, subCategory_num=270, click_predictor='mlp')
# BASELINE.json configs[0] shape: batch 8, history 10, title 16, body 32, K = 1 + 1
_CFG1 = dict(max_history_num=10, max_title_length=16, max_abstract_length=32, batch_size=8, **_SMALL)
_TINY = dict(max_history_num=6, max_title_length=8, max_abstract_length=16, batch_size=4, **_SMALL)

CASES = {
    # LIME-CROWN-CROWN: the history-vs-candidate attention in front of the predictor (H rows per group)
    # (guard: 2.4e-4, word_embedding.weight; residue on out.bias 1.5e-8)
    'mlp_lime_crown_crown': dict(cfg=dict(content_encoder='CROWN', user_encoder='CROWN', **_CFG1), B=8, N=2, seed=301, eval_shape=False,
                                 edit='none'),
    # LIME-NAML-ATT: one pooled user vector per row
    # (guard: 2.2e-4, word_embedding.weight; residue on out.bias 7.5e-9)
    'mlp_lime_naml_att': dict(cfg=dict(content_encoder='NAML', user_encoder='ATT', **_CFG1), B=8, N=2, seed=302, eval_shape=False, edit='none'),
    # NRMS without LIME: D = 300, Dh = 150 -- an odd Dh / 2: rows of gu and nw are 8-byte, not 16-byte, aligned
    'mlp_plain_mhsa_mhsa': dict(cfg=dict(news_encoder='MHSA', user_encoder='MHSA', **_CFG1), B=8, N=2, seed=303, eval_shape=False, edit='none'),
    # the original CROWN: D = 900, Dh = 450
    'mlp_plain_crown_crown': dict(cfg=dict(news_encoder='CROWN', user_encoder='CROWN', **_TINY), B=4, N=3, seed=304, eval_shape=False,
                                  edit='none'),
    # no candidate-aware refinement: under ATT one user vector per HISTORY
    'mlp_no_cand_aware': dict(cfg=dict(content_encoder='NAML', user_encoder='ATT', use_candidate_ware_clicked_news_attention=False, **_TINY),
                              B=4, N=3, seed=305, eval_shape=False, edit='none'),
    # all-padding histories
    'mlp_empty_history': dict(cfg=dict(content_encoder='CROWN', user_encoder='CROWN', **_TINY), B=4, N=2, seed=306, eval_shape=False,
                              edit='empty_history'),
    # the reference's eval path (one candidate per row, no N axis): forward only
    'mlp_lime_crown_crown_eval': dict(cfg=dict(content_encoder='CROWN', user_encoder='CROWN', **_CFG1), B=8, N=1, seed=307, eval_shape=True,
                                      edit='none'),
}

GRAD_CASES = ('mlp_lime_crown_crown', 'mlp_lime_naml_att')
# ``out.bias`` adds one constant to every logit of a row, which the softmax loss does not feel: its gradient is identically zero and the
# reference stores rounding residue there (tools/make_mlp_goldens.py prints it)
ZERO_GRADIENT = 'out.bias'


def build_case(name):
    """-> (config, OrderedDict of the 26 inputs, case dict)."""
    c = CASES[name]
    cfg = make_config(**c['cfg'])
    batch = synth.make_batch(cfg, c['B'], c['N'], seed=c['seed'], eval_shape=c['eval_shape'])
    batch = EDITS[c['edit']](cfg, batch)
    return cfg, batch, c
