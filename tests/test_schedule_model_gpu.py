"""Model.score_schedule / Model.recommend_schedule on the MI355X, on the fixture of tests/test_recommend_gpu.py (60 news, three users of
whom one has an empty history, a pool of 37 news over five topics): slot s against ``score_pool`` / ``recommend`` called with
``cand_freshness + slot_offsets[s]`` -- bit for bit on the shared-user-side route and on a baseline, within KTOL on the factorised
route (lime_grouped_match_schedule_f32 rounds two partial sums where the existing kernels round one composed operand) --, the top-k
against lime_topk_rows_f32 on the schedule's own scores, the exclusion, and a count of the launches the factorised route must not make.
Three slots, not in order, whose offsets are chosen on the host from the fixture's values: one moves candidates past their expiry, one
moves some of them into the next freshness bucket as well (the first test checks both on the host)."""
import numpy as np
import pytest
import torch

import test_recommend_gpu as R
from helpers import rel_err
from test_occurrence_match_model_gpu import _same_choice
from test_recommend_gpu import C, K, TOL, U
from lime_cikm25_amd import model as model_module, newsEncoders, ops, serving

pytestmark = pytest.mark.gpu

KTOL = 2e-5
R.CASES.update({
    'mlp_crown_user': dict(click_predictor='mlp'),
    'baseline_naml_att': dict(news_encoder='NAML', user_encoder='ATT'),
})
# name -> the route of a schedule of several slots
ROUTE = {'crown_user': 'factorised', 'add': 'factorised', 'att_user': 'factorised', 'baseline_naml_att': 'factorised', 'gated': 'shared',
         'mlp_crown_user': 'shared'}
SAME_BITS = ['baseline_naml_att', 'gated', 'mlp_crown_user']           # the shared user side, and the baseline on either route
OFFSETS = [10.0, 3000.0, 0.0]
S = len(OFFSETS)


def slot_offsets():
    return torch.tensor(OFFSETS, dtype=torch.float32, device='cuda')


def shifted(args, offset):
    return dict(args, cand_freshness=args['cand_freshness'] + offset)


def test_the_offsets_cross_an_expiry_and_a_bucket_cut():
    model, args, *_ = R.build('crown_user')
    fresh = args['cand_freshness'].cpu()
    left = (args['cand_lifetime'].cpu() - fresh).numpy()                   # the remaining lifetime now, [U, C]
    assert ((left > 0) & (left - OFFSETS[0] < 0)).sum() > 0 and ((left - OFFSETS[0]) > 0).sum() > 0      # some expire in slot 0, some do not
    assert ((left - OFFSETS[1]) > 0).sum() > 0                                                            # ... nor do all in slot 1
    nb = model.config.num_buckets
    now, later = newsEncoders.reference_bucket(fresh, nb), newsEncoders.reference_bucket(fresh + OFFSETS[1], nb)
    moved = (now != later).numpy()
    assert 4 <= moved.sum() < C                                            # slot 1 moves some candidates into the next freshness bucket
    assert (moved[None, :] & (left - OFFSETS[1] > 0)).sum() > 0            # ... and some of those are still alive there: the weight is felt


@pytest.mark.parametrize('name', list(ROUTE))
def test_every_slot_is_score_pool_at_the_shifted_freshness(name, monkeypatch):
    model, args, want, n_src, *_ = R.build(name)
    assert model.schedule_route(S, args['hist_index'].shape[1]) == ROUTE[name]
    got = model.score_schedule(**args, slot_offsets=slot_offsets(), n_src=n_src)
    assert got.shape == (S, U, C) and got.dtype == torch.float32 and torch.isfinite(got).all()
    assert torch.equal(got, model.score_schedule(**args, slot_offsets=slot_offsets(), n_src=n_src)), 'two runs differ'
    monkeypatch.setattr(model_module, 'SCHEDULE_MATCH', False)
    assert model.schedule_route(S) in ('shared', 'expand')
    shared = model.score_schedule(**args, slot_offsets=slot_offsets(), n_src=n_src)
    monkeypatch.undo()
    several = model.score_schedule(**args, slot_offsets=slot_offsets(), n_src=n_src, pairs_per_pass=40)     # one user a pass
    for s, offset in enumerate(OFFSETS):
        pool = model.score_pool(**shifted(args, offset), n_src=n_src)
        assert torch.equal(shared[s], pool), 'the shared user side must give score_pool\'s bits'
        e = rel_err(got[s].cpu().numpy(), pool.cpu().numpy())
        e_several = rel_err(several[s].cpu().numpy(), model.score_pool(**shifted(args, offset), n_src=n_src, pairs_per_pass=40).cpu().numpy())
        print('%s slot %d (+%g): schedule vs score_pool rel err %.2e (one user a pass: %.2e), vs the shared user side %.2e' % (
            name, s, offset, e, e_several, rel_err(got[s].cpu().numpy(), shared[s].cpu().numpy())))
        if name in SAME_BITS:
            assert torch.equal(got[s], pool)
        else:
            assert e <= KTOL and e_several <= KTOL and rel_err(got[s].cpu().numpy(), shared[s].cpu().numpy()) <= KTOL
        if model.click_predictor == 'dot_product':                          # expired beyond the weight's range: exact zeros stay exact
            assert torch.equal(got[s] == 0, pool == 0)
    assert not torch.equal(got[1], got[2]), 'a slot that moves freshness buckets must differ'
    # (slot 0 moves no bucket: only the lifetime weight feels it, and the MLP predictor has none)
    assert torch.equal(got[0], got[2]) == (model.click_predictor == 'mlp')
    assert rel_err(got[2].cpu().numpy(), want.cpu().numpy()) <= TOL        # slot 2 is now: the cached dev pass


@pytest.mark.parametrize('name', list(ROUTE))
def test_one_slot_is_score_pool_itself(name):
    model, args, want, n_src, *_ = R.build(name)
    assert model.schedule_route(1) == 'single'
    for offset in (0.0, 10.0):
        one = model.score_schedule(**args, slot_offsets=torch.tensor([offset], device='cuda'), n_src=n_src)
        assert one.shape == (1, U, C) and torch.equal(one[0], model.score_pool(**shifted(args, offset), n_src=n_src))
    pos, top = model.recommend_schedule(**args, slot_offsets=[10.0], k=K, n_src=n_src)
    pos0, top0 = model.recommend(**shifted(args, 10.0), k=K, n_src=n_src)
    assert pos.shape == (1, U, K) and torch.equal(pos[0], pos0) and torch.equal(top[0], top0)


def test_a_baseline_under_the_mlp_predictor_is_one_slot_repeated():
    R.CASES['mlp_baseline'] = dict(news_encoder='NAML', user_encoder='ATT', click_predictor='mlp')
    model, args, want, n_src, *_ = R.build('mlp_baseline')
    assert model.schedule_route(S) == 'expand'
    got = model.score_schedule(**args, slot_offsets=slot_offsets(), n_src=n_src)
    pool = model.score_pool(**args, n_src=n_src)
    assert got.shape == (S, U, C) and got.is_contiguous()
    for s, offset in enumerate(OFFSETS):
        assert torch.equal(got[s], pool) and torch.equal(pool, model.score_pool(**shifted(args, offset), n_src=n_src))


@pytest.mark.parametrize('name', list(ROUTE))
def test_recommend_schedule_is_the_top_k_of_its_scores_and_recommend_s_choice(name):
    model, args, want, n_src, *_ = R.build(name)
    pos, top = model.recommend_schedule(**args, slot_offsets=slot_offsets(), k=K, n_src=n_src)
    assert pos.shape == top.shape == (S, U, K) and pos.dtype == torch.int32 and top.dtype == torch.float32
    scores = model.score_schedule(**args, slot_offsets=slot_offsets(), n_src=n_src)
    p2, t2 = ops.topk_rows(scores.view(S * U, C), K)
    assert torch.equal(pos.view(S * U, K), p2) and torch.equal(top.view(S * U, K), t2)
    for s, offset in enumerate(OFFSETS):
        pos0, _ = model.recommend(**shifted(args, offset), k=K, n_src=n_src)
        s0 = model.score_pool(**shifted(args, offset), n_src=n_src).cpu().numpy().astype(np.float64)
        tol = TOL * float(np.abs(s0).mean())
        assert (np.diff(top[s].cpu().numpy(), axis=1) <= 0).all()
        assert _same_choice(pos[s].cpu().numpy(), top[s].cpu().numpy(), pos0.cpu().numpy(), s0, tol)
        if name in SAME_BITS:
            assert torch.equal(pos[s], pos0)


@pytest.mark.parametrize('name', ['crown_user', 'baseline_naml_att', 'gated'])
def test_exclude_history_removes_the_same_candidates_in_every_slot(name):
    model, args, want, n_src, hist, mask, pool = R.build(name)
    plain = model.score_schedule(**args, slot_offsets=slot_offsets(), n_src=n_src)
    scores = model.score_schedule(**args, slot_offsets=slot_offsets(), n_src=n_src, exclude_history=True)
    pos, top = model.recommend_schedule(**args, slot_offsets=slot_offsets(), k=C, n_src=n_src, exclude_history=True)
    pos, top = pos.cpu().numpy(), top.cpu().numpy()
    gone = np.array([[int(n) in set(hist[u][mask[u]].tolist()) for n in pool] for u in range(U)])
    assert gone.sum(axis=1).tolist() == [3, 1, 0]
    keep = torch.from_numpy(~gone).cuda()
    for s in range(S):
        assert torch.isneginf(scores[s][~keep]).all() and torch.equal(scores[s][keep], plain[s][keep])
        for u in range(U):
            live = pos[s, u][pos[s, u] >= 0]
            assert len(live) == C - gone[u].sum() and not gone[u][live].any() and len(set(live.tolist())) == len(live)
            assert (pos[s, u][len(live):] == -1).all() and np.isneginf(top[s, u][len(live):]).all()
    one, several = (model.recommend_schedule(**args, slot_offsets=slot_offsets(), k=C, n_src=n_src, exclude_history=True, pairs_per_pass=p)
                    for p in (1 << 18, 40))
    if name in SAME_BITS:
        assert torch.equal(one[0], several[0]) and torch.equal(one[1], several[1])


class _Calls:
    """The row counts of every encode_cached and ops.linear call, and the number of match_operands calls, while it is on."""

    def __init__(self, monkeypatch, model):
        self.encode, self.linear, self.user_side, self.operands = [], [], 0, 0
        ne, ue = model.news_encoder, model.user_encoder
        real_encode, real_linear, real_operands, real_user_side = ne.encode_cached, ops.linear, ue.match_operands, serving.user_side

        def encode_cached(cache, news_index, *a, **kw):
            self.encode.append(int(news_index.numel()))
            return real_encode(cache, news_index, *a, **kw)

        def linear(a, *rest, **kw):
            self.linear.append(int(a.shape[0]))
            return real_linear(a, *rest, **kw)

        def match_operands(*a, **kw):
            self.operands += 1
            return real_operands(*a, **kw)

        def user_side(*a, **kw):
            self.user_side += 1
            return real_user_side(*a, **kw)
        monkeypatch.setattr(ne, 'encode_cached', encode_cached)
        monkeypatch.setattr(ops, 'linear', linear)
        monkeypatch.setattr(ue, 'match_operands', match_operands)
        monkeypatch.setattr(serving, 'user_side', user_side)


@pytest.mark.parametrize('name', ['crown_user', 'add', 'att_user', 'baseline_naml_att'])
def test_the_factorised_route_launches_nothing_over_the_slots(name, monkeypatch):
    """No encode_cached, Q or per-pair GEMM runs over S U C (or U C) rows, and the user side runs once per call, its operands once per
    pass -- not once per slot.  The same counter does see the per-pair rows, S times, on the shared-user-side route of a LIME model."""
    model, args, want, n_src, *_ = R.build(name)
    H = args['hist_index'].shape[1]
    assert len({S * U * C, U * C, C, U * H}) == 4
    seen = {}
    for route, passes, kw in (('factorised', 1, {}), ('factorised', U, dict(pairs_per_pass=40)), ('shared', 1, {})):
        if route == 'shared':
            monkeypatch.setattr(model_module, 'SCHEDULE_MATCH', False)
        calls = _Calls(monkeypatch, model)
        model.score_schedule(**args, slot_offsets=slot_offsets(), n_src=n_src, **kw)
        monkeypatch.undo()
        assert calls.user_side == 1 and calls.operands == passes, (route, calls.user_side, calls.operands)
        seen[route, passes] = calls
    for key in (('factorised', 1), ('factorised', U)):
        for rows in (seen[key].encode, seen[key].linear):
            assert S * U * C not in rows and U * C not in rows, rows
    if name != 'baseline_naml_att':
        assert seen['shared', 1].encode.count(U * C) == S, 'the counter must see the materialised rows, once per slot'
