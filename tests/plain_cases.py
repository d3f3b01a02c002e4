"""Golden-vector cases of the baseline models -- a content encoder as the news encoder itself, no LIME (config.news_encoder = 'CROWN',
'CNN', 'NAML', 'MHSA', 'KCNN'; reference model.py:41-62) -- in the structure of golden_cases.CASES and built from the same generator
(``golden_cases.EDITS`` / ``WEIGHT_SEED`` / lime_cikm25_amd.synth; KCNN's entity ids from kcnn_cases.with_entities).
tools/make_plain_goldens.py runs the imported reference on them; tests/test_plain_*.py regenerate the same inputs and weights.  Only
outputs are stored (tests/golden/plain_*.npz, grad_plain_*.npz).

The batch seeds of the gradient cases: tools/make_plain_goldens.py applies the guards of tools/make_grad_goldens.py (the reference's fp32
gradients within half of the check's 1e-3 of its own fp64 ones, no zero-gradient residue the check resolves) and ``--probe`` walks a
case's seed, seed + 100, ... to the first that passes.  The figure beside a case is what the guard printed for the seed it has (it moves
a little with the thread count of the run); where the case's first seed failed, the comment says by how much."""
from lime_cikm25_amd.config import make_config
from lime_cikm25_amd import synth

import golden_cases
import kcnn_cases

EDITS = golden_cases.EDITS
WEIGHT_SEED = golden_cases.WEIGHT_SEED

_SMALL = dict(vocabulary_size=5000, category_num=18, subCategory_num=270)
# BASELINE.json configs[0] shape: batch 8, history 10, title 16, body 32, K = 1 + 1
_CFG1 = dict(max_history_num=10, max_title_length=16, max_abstract_length=32, batch_size=8, **_SMALL)
_TINY = dict(max_history_num=6, max_title_length=8, max_abstract_length=16, batch_size=4, **_SMALL)

CASES = {
    # CROWN-CROWN, the original CROWN: D = 900, the unfused refinement, the news encoder's own category_affine on the user side
    # (guard: 3.6e-5, candidate_aware_attn.key_proj.weight)
    'plain_crown_crown': dict(cfg=dict(news_encoder='CROWN', user_encoder='CROWN', **_TINY), B=4, N=3, seed=201, eval_shape=False, edit='none'),
    # rows per forward (8) > history slots (6): user-node slots in the GraphSAGE mean at D = 900
    # (guard: 1.0e-4, word_embedding.weight)
    'plain_crown_crown_spill': dict(cfg=dict(news_encoder='CROWN', user_encoder='CROWN', **_TINY), B=8, N=2, seed=202, eval_shape=False,
                                    edit='none'),
    # (guard: 7.7e-5, word_embedding.weight)
    'plain_crown_crown_empty_history': dict(cfg=dict(news_encoder='CROWN', user_encoder='CROWN', **_TINY), B=4, N=2, seed=203,
                                            eval_shape=False, edit='empty_history'),
    # the reference's eval path (one candidate per row, no N axis): forward only
    'plain_crown_crown_eval': dict(cfg=dict(news_encoder='CROWN', user_encoder='CROWN', **_TINY), B=4, N=1, seed=204, eval_shape=True,
                                   edit='none'),
    # (guard: 6.3e-5, word_embedding.weight)
    'plain_crown_att': dict(cfg=dict(news_encoder='CROWN', user_encoder='ATT', **_TINY), B=4, N=3, seed=205, eval_shape=False, edit='none'),
    # NAML-ATT is NAML, MHSA-MHSA is NRMS
    # (seeds 206 and 306 leave the reference's word_embedding gradient 6.0e-4 and 6.5e-4 from its fp64 one, above half of the check's 1e-3;
    # 406 is the first under it: 3.3e-4)
    'plain_naml_att': dict(cfg=dict(news_encoder='NAML', user_encoder='ATT', **_CFG1), B=8, N=2, seed=406, eval_shape=False, edit='none'),
    'plain_naml_att_eval': dict(cfg=dict(news_encoder='NAML', user_encoder='ATT', **_CFG1), B=8, N=1, seed=207, eval_shape=True, edit='none'),
    # (guard: 2.2e-4, attention.affine1.bias)
    'plain_mhsa_mhsa': dict(cfg=dict(news_encoder='MHSA', user_encoder='MHSA', **_CFG1), B=8, N=2, seed=208, eval_shape=False, edit='none'),
    # (seeds 209 and 309 leave a residue of 4.9e-8 and 4.5e-8 on the self-attention's key bias, an identically-zero gradient of which the
    # check resolves 1e-8; 409 passes: 1.3e-4, user_encoder.attention.affine1.weight)
    'plain_cnn_mhsa': dict(cfg=dict(news_encoder='CNN', user_encoder='MHSA', **_TINY), B=4, N=3, seed=409, eval_shape=False, edit='none'),
    # (guard: 6.7e-5, candidate_aware_attn.key_proj.weight)
    'plain_kcnn_att': dict(cfg=dict(news_encoder='KCNN', user_encoder='ATT', entity_size=600, **_TINY), B=4, N=3, seed=210, eval_shape=False,
                           edit='none'),
    # no candidate-aware refinement at all: the encoder holds no candidate_aware_attn and category_embedding gets its gradient from the
    # news side alone
    # (guard: 1.5e-4, attention.affine1.bias)
    'plain_mhsa_mhsa_no_cand_aware': dict(cfg=dict(news_encoder='MHSA', user_encoder='MHSA', use_candidate_ware_clicked_news_attention=False,
                                                   **_TINY),
                                          B=4, N=2, seed=211, eval_shape=False, edit='none'),
    # util.py:34: the plain dot product (remaining_lifetime is not read)
    # (guard: 4.7e-5, word_embedding.weight)
    'plain_crown_crown_no_weighting': dict(cfg=dict(news_encoder='CROWN', user_encoder='CROWN', use_remaining_lifetime_weighting=False, **_TINY),
                                           B=4, N=3, seed=212, eval_shape=False, edit='lifetime_signs'),
}

GRAD_CASES = tuple(n for n, c in CASES.items() if not c['eval_shape'])


def build_case(name, seed=None):
    """-> (config, OrderedDict of the 26 inputs, case dict).  ``seed``: another batch seed than the case's (the golden tool's probe)."""
    c = CASES[name]
    seed = c['seed'] if seed is None else seed
    cfg = make_config(**c['cfg'])
    batch = synth.make_batch(cfg, c['B'], c['N'], seed=seed, eval_shape=c['eval_shape'])
    batch = EDITS[c['edit']](cfg, batch)
    if cfg.news_encoder == 'KCNN':
        batch = kcnn_cases.with_entities(cfg, batch, seed)
    return cfg, batch, c
