"""Model.score_pool / recommend / score_lists / recommend_lists and the grouped dev pass with LIME's candidates composed in the
kernel (model.OCCURRENCE_MATCH, lime_grouped_match_occurrence_f32) on the MI355X: against the cached dev pass (helpers.rel_err <=
1e-3, the bar of tests/test_recommend_gpu.py, whose fixture -- 60 news, three users of whom one has an empty history, a pool of 37
news over five topics -- this file takes), against the materialised path (bit for bit where no product is re-associated, KTOL where
one is), with a count of the launches that must not run any more, and with the models that keep the materialised path as controls."""
import numpy as np
import pytest
import torch

import test_recommend_gpu as R
from helpers import rel_err
from test_lists_gpu import IMP_LENS, PER, dev_split, no_near_ties
from test_recommend_gpu import C, K, TOL, U
from lime_cikm25_amd import DeviceBehaviors, DeviceCorpus, model as model_module, ops, util

pytestmark = pytest.mark.gpu

KTOL = 2e-5                     # fp32-level kernel against the same sums in another order, as tests/test_plain_gpu.py

# the fixture recipe's configurations this file adds (R.build reads R.CASES by name; R's own parametrisations are made already)
R.CASES.update({
    'mlp_crown_user': dict(click_predictor='mlp'),
    'mlp_att_user': dict(user_encoder='ATT', click_predictor='mlp'),
    'identity_concat': dict(user_encoder='ATT', lime_output_dim=0),
    'baseline': dict(news_encoder='CROWN'),
})
APPLICABLE = ['crown_user', 'att_user', 'mhsa_user', 'add', 'attention_off', 'att_attention_off', 'kcnn_content', 'fixed_lifetime',
              'mlp_crown_user', 'mlp_att_user']
SAME_BITS = ['att_user', 'mhsa_user', 'att_attention_off']      # ATT / MHSA with the dot product: the candidate row has the same bits
CONTROLS = ['gated', 'identity_concat', 'baseline']             # occurrence_match_applicable() is False: the switch changes nothing
LIST_LENS = [20, 0, 9]                                          # three lists of unequal length, one of them empty
P = sum(LIST_LENS)


@pytest.fixture
def switch(monkeypatch):
    def turn(on):
        monkeypatch.setattr(model_module, 'OCCURRENCE_MATCH', bool(on))
    return turn


def list_args(args, want):
    """The pool fixture's pairs as three lists: user u's list is LIST_LENS[u] news of the pool, from position 3 u on -> (score_lists'
    arguments, the cached pass's scores of those pairs)."""
    at = [np.arange(3 * u, 3 * u + n) for u, n in enumerate(LIST_LENS)]
    users = torch.from_numpy(np.repeat(np.arange(U), LIST_LENS)).cuda()
    cols = torch.from_numpy(np.concatenate(at)).cuda()
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(LIST_LENS)]).astype(np.int64))
    out = {k: args[k] for k in ('news_cache', 'corpus', 'hist_index', 'hist_mask', 'user_freshness', 'user_lifetime')}
    out.update(cand_offsets=off, cand_index=args['cand_index'][cols], cand_freshness=args['cand_freshness'][cols],
               cand_lifetime=args['cand_lifetime'][users, cols])
    return out, want[users, cols]


@pytest.mark.parametrize('name', APPLICABLE)
def test_pool_and_lists_equal_the_cached_pass(name, switch):
    model, args, want, n_src, *_ = R.build(name)
    assert model.occurrence_match_applicable()
    switch(True)
    got = model.score_pool(**args, n_src=n_src)
    assert got.shape == (U, C) and torch.isfinite(got).all()
    e = rel_err(got.cpu().numpy(), want.cpu().numpy())
    zeros = want == 0
    largs, lwant = list_args(args, want)
    lgot = model.score_lists(**largs, n_src=n_src)
    assert lgot.shape == (P,) and torch.isfinite(lgot).all()
    le = rel_err(lgot.cpu().numpy(), lwant.cpu().numpy())
    print('%s: composed score_pool vs score_behaviors rel err %.2e over %d pairs (%d exact zeros); score_lists %.2e over %d pairs' % (
        name, e, U * C, int(zeros.sum()), le, P))
    assert e <= TOL and le <= TOL
    if model.click_predictor == 'dot_product':                             # (the MLP predictor has no lifetime weight: no exact zeros)
        assert int(zeros.sum()) > 0 and (got[zeros] == 0).all(), 'an exact zero of the cached pass must be an exact zero here'
        assert (lgot[lwant == 0] == 0).all()
    # several passes: a pair's bits do not depend on the pass
    assert torch.equal(model.score_pool(**args, n_src=n_src, pairs_per_pass=40), got)
    assert torch.equal(model.score_lists(**largs, n_src=n_src, pairs_per_pass=40), lgot)


def _same_choice(pos_on, top_on, pos_off, scores_off, tol):
    """The rule of tests/test_recommend_gpu.py where two scores may tie within the rounding difference: the positions are the same,
    or the scores of the yardstick at the chosen positions are those it chose itself, within tol."""
    if np.array_equal(pos_on, pos_off):
        return True
    for u in range(pos_on.shape[0]):
        live = pos_on[u] >= 0
        if (live != (pos_off[u] >= 0)).any():
            return False
        if np.abs(scores_off[u][pos_on[u][live]] - scores_off[u][pos_off[u][live]]).max(initial=0.0) > tol:
            return False
    return True


@pytest.mark.parametrize('name', APPLICABLE)
def test_recommend_and_recommend_lists_choose_what_the_materialised_path_chooses(name, switch):
    model, args, want, n_src, *_ = R.build(name)
    largs, _ = list_args(args, want)
    switch(False)
    pos0, _ = model.recommend(**args, k=K, n_src=n_src)
    s0 = model.score_pool(**args, n_src=n_src).cpu().numpy().astype(np.float64)
    lpos0, _ = model.recommend_lists(**largs, k=K, n_src=n_src)
    ls0 = model.score_lists(**largs, n_src=n_src).cpu().numpy().astype(np.float64)
    switch(True)
    pos1, top1 = model.recommend(**args, k=K, n_src=n_src)
    lpos1, ltop1 = model.recommend_lists(**largs, k=K, n_src=n_src)
    tol = TOL * float(np.abs(s0).mean())
    assert pos1.shape == (U, K) and (np.diff(top1.cpu().numpy(), axis=1) <= 0).all()
    assert _same_choice(pos1.cpu().numpy(), top1.cpu().numpy(), pos0.cpu().numpy(), s0, tol)
    bounds = np.concatenate([[0], np.cumsum(LIST_LENS)])
    per_list = [ls0[a:b] for a, b in zip(bounds[:-1], bounds[1:])]
    assert lpos1.shape == (U, K) and lpos1[1].tolist() == [-1] * K          # the empty list
    assert _same_choice(lpos1.cpu().numpy(), ltop1.cpu().numpy(), lpos0.cpu().numpy(), per_list, tol)


@pytest.mark.parametrize('name', APPLICABLE)
def test_on_against_off(name, switch, monkeypatch):
    """ATT / MHSA with the dot product: the bits of the materialised path taken with ops.FUSED_OCCURRENCE on (A[news] + T[pair] in
    one fp32 add, the add the kernel makes; qp is never felt).  Under the CROWN user encoder (Q) or the MLP predictor (W_n) the tables
    re-associate one product: KTOL, the project's bound for the same sums in another order."""
    model, args, want, n_src, *_ = R.build(name)
    largs, _ = list_args(args, want)
    monkeypatch.setattr(ops, 'FUSED_OCCURRENCE', True)
    switch(False)
    off, loff = model.score_pool(**args, n_src=n_src), model.score_lists(**largs, n_src=n_src)
    switch(True)
    on, lon = model.score_pool(**args, n_src=n_src), model.score_lists(**largs, n_src=n_src)
    e, le = rel_err(on.cpu().numpy(), off.cpu().numpy()), rel_err(lon.cpu().numpy(), loff.cpu().numpy())
    print('%s: composed vs materialised (FUSED_OCCURRENCE on) rel err %.2e (pool), %.2e (lists)' % (name, e, le))
    if name in SAME_BITS:
        assert torch.equal(on, off) and torch.equal(lon, loff)
    else:
        assert e <= KTOL and le <= KTOL


class _Rows:
    """The row counts of every encode_cached call and every ops.linear call (the Q and the MLP GEMMs go through it) while it is on."""

    def __init__(self, monkeypatch, model):
        self.encode, self.linear = [], []
        ne = model.news_encoder
        real_encode, real_linear = ne.encode_cached, ops.linear

        def encode_cached(cache, news_index, *a, **kw):
            self.encode.append(int(news_index.numel()))
            return real_encode(cache, news_index, *a, **kw)

        def linear(a, *rest, **kw):
            self.linear.append(int(a.shape[0]))
            return real_linear(a, *rest, **kw)
        monkeypatch.setattr(ne, 'encode_cached', encode_cached)
        monkeypatch.setattr(ops, 'linear', linear)


@pytest.mark.parametrize('name', ['crown_user', 'att_user', 'add', 'mlp_crown_user', 'mlp_att_user'])
def test_no_launch_runs_over_the_pairs(name, switch, monkeypatch):
    """With the tables in place neither encode_cached nor a Q / MLP GEMM runs with the pair count as its row count -- and the same
    counter does see them on the materialised path."""
    model, args, want, n_src, *_ = R.build(name)
    largs, _ = list_args(args, want)
    assert U * C not in (U * model.config.max_history_num, P) and P != U * model.config.max_history_num
    seen = {}
    for on in (False, True):
        switch(on)
        assert (model._candidate_tables(args['news_cache']) is not None) == on
        rows = _Rows(monkeypatch, model)
        model.score_pool(**args, n_src=n_src)
        model.score_lists(**largs, n_src=n_src)
        seen[on] = rows
        monkeypatch.undo()
    assert U * C in seen[False].encode and P in seen[False].encode, 'the counter must see the materialised rows'
    if name in ('crown_user', 'add', 'mlp_crown_user', 'mlp_att_user'):
        assert U * C in seen[False].linear and P in seen[False].linear      # Q under CROWN, nw under the MLP predictor
    for calls in (seen[True].encode, seen[True].linear):
        assert U * C not in calls and P not in calls, calls


@pytest.mark.parametrize('name', CONTROLS)
def test_models_that_keep_their_path_do_not_feel_the_switch(name, switch):
    model, args, want, n_src, *_ = R.build(name)
    assert not model.occurrence_match_applicable()
    largs, _ = list_args(args, want)
    switch(False)
    off, loff = model.score_pool(**args, n_src=n_src), model.score_lists(**largs, n_src=n_src)
    switch(True)
    assert torch.equal(model.score_pool(**args, n_src=n_src), off) and torch.equal(model.score_lists(**largs, n_src=n_src), loff)
    assert rel_err(off.cpu().numpy(), want.cpu().numpy()) <= TOL


@pytest.mark.parametrize('name', ['crown_user', 'att_user'])
def test_the_grouped_dev_pass(name, switch):
    """evaluate_cached_on_device(grouped=True) on the synthetic dev split of tests/test_lists_gpu.py: scores within that file's bound of
    the switch-off pass and, its scores having no near-ties inside an impression, the same four metrics."""
    for seed in range(51, 61):
        corpus, model, indices, labels = dev_split(name, seed)
        dev = DeviceBehaviors.from_devtest(DeviceCorpus(corpus), corpus, 'dev')
        switch(False)
        m0, s0 = util.evaluate_cached_on_device(model, dev, indices, labels, rows_per_forward=PER, return_scores=True, grouped=True)
        if no_near_ties(s0.cpu().numpy()):
            break
    else:
        pytest.fail('no seed gives the yardstick scores without near-ties inside an impression')
    assert dev.num == sum(IMP_LENS)
    switch(True)
    m1, s1 = util.evaluate_cached_on_device(model, dev, indices, labels, rows_per_forward=PER, return_scores=True, grouped=True)
    e = rel_err(s1.cpu().numpy(), s0.cpu().numpy())
    print('%s (split seed %d): composed vs materialised grouped dev pass rel err %.2e; metrics %s vs %s' % (name, seed, e, tuple(m1), tuple(m0)))
    assert e <= TOL
    assert all(abs(a - b) <= TOL for a, b in zip(m1, m0)) and len(tuple(m1)) == 4
