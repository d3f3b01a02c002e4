"""util.evaluate_slates_on_device end to end on the MI355X: tiny models (LIME over CROWN, and the baseline NAML + ATT) on a synthetic dev
split of 40 impressions with 2 .. 30 candidates.  What a setting returns is held to the composition of pieces that have their own
tests: the slates of serving.select_segments on the pass's score buffer (the same device kernels: the same bits) and
recommend.slate_metrics on those slates -- this pins the plumbing (offsets, rows, news ids, labels, skip, key table) and does not
depend on near-ties in MMR.

The device dev pass raises, as evaluate.scoring does, for an impression with one class only; a single-row impression and one without
a positive are such impressions.  So the whole entry runs on the split without them (it keeps the label-less truth line), and the
split WITH them goes through util.sweep_slate_settings -- everything behind the scoring pass -- on the scores of score_behaviors."""
import os

import numpy as np
import pytest
import torch

from lime_cikm25_amd import DeviceBehaviors, DeviceCorpus, evaluate as E, recommend, serving
from lime_cikm25_amd import util as U
from lime_cikm25_amd.device_data import topic_table_of
from helpers import rel_err
from slate_cases import MODELS, dev_split, toy

pytestmark = pytest.mark.gpu

PER, K = 6, 5
U24, U53 = 2.0 ** -24, 2.0 ** -53
TOL = 1e-3                                        # grouped against row-wise scores (tests/test_lists_gpu.py)
SETTINGS = [{}, {'max_per_topic': 1}, {'mmr_lambda': 0.5, 'shortlist': 8}, {'max_per_topic': 1, 'mmr_lambda': 0.5, 'shortlist': 8}]
EXACT = (0, 1, 2, 3, 5, 6, 7)
_SPLITS = {}


def split(name, one_class=False, seed=71):
    key = (name, one_class, seed)
    if key not in _SPLITS:
        corpus, model, indices, labels = dev_split(name, seed=seed, one_class=one_class)
        dev = DeviceBehaviors.from_devtest(DeviceCorpus(corpus), corpus, 'dev')
        _SPLITS[key] = (model, dev, indices, labels)
    return _SPLITS[key]


def composed(model, dev, cache, scores, indices, labels, setting, k, value):
    """What a setting must give: select_segments called directly on the score buffer, recommend.slate_metrics on its slates."""
    offsets, row_labels, skip = E.impression_layout(indices, labels)
    quota = serving.topic_quota(dev.corpus, setting.get('max_per_topic'), setting.get('quota_by', 'category'))
    div = serving.diversity(model, cache, k, setting.get('mmr_lambda'), setting.get('shortlist'), setting.get('similarity'))
    cand = dev.cand_index.reshape(-1)
    positions, _ = serving.select_segments(scores, torch.from_numpy(offsets.astype(np.int64)).cuda(), None, quota, div, cand, k)
    table = serving.content_columns(model, cache)
    keys, cat_t, _ = topic_table_of(dev.corpus, setting.get('topic_by', 'category'))
    want = recommend.slate_metrics(positions.cpu().numpy(), k, offsets, cand.cpu().numpy(), row_labels, skip,
                                   None if value is None else value.cpu().numpy(), table.cpu().numpy(), keys.cpu().numpy(),
                                   n_keys=cat_t.numel())
    return want, positions.cpu().numpy(), table.shape[1]


def check_setting(res, want, E_cols, n_imp, what):
    per_w, status_w, sums_w, counts_w = want
    per, status = res['per_impression'].cpu().numpy(), res['status'].cpu().numpy()
    assert np.array_equal(status, status_w)
    assert (res['n_relevance'], res['n_diversity'], res['n_slates']) == tuple(int(c) for c in counts_w)
    for c in EXACT:
        assert np.array_equal(per[:, c], per_w[:, c]), (what, c)
    bound = (2 * E_cols + 8) * U24
    print('%s: ILD max |kernel - fp64| %.3e (bound %.3e); %s' % (what, np.abs(per[:, 4] - per_w[:, 4]).max(), bound,
                                                                 {k: v for k, v in res.items() if k not in ('per_impression', 'status')}))
    assert np.abs(per[:, 4] - per_w[:, 4]).max() <= bound
    for c, name in enumerate(U.SLATE_RESULT_KEYS):
        n = counts_w[0 if c < 4 else 1 if c == 4 else 2]
        mean = sums_w[c] / n
        room = bound if c == 4 else n_imp * U53 * max(1.0, np.abs(per_w[:, c]).max())
        assert abs(res[name] - mean) <= room, (what, name, res[name], mean)


@pytest.mark.parametrize('name', list(MODELS))
def test_the_sweep_is_the_composition_of_its_pieces(name):
    """The split with a single-row impression, one without a positive and a label-less truth line, behind the scoring pass."""
    model, dev, indices, labels = split(name, one_class=True)
    assert len(labels[5]) == 1 and sum(labels[7]) == 0 and labels[3] == [] and 1 < len(labels[7])
    cache = model.build_news_cache(dev.corpus)
    H = dev.hist_index.shape[1]
    scores = model.score_behaviors(dev, torch.arange(dev.num, device='cuda'), cache, n_src=min(dev.num, H + model.config.batch_size)).float()
    value = U.sweep_slate_settings(model, dev, cache, scores, indices, labels, [{}], K, 'freshness', per_impression=True)[0]
    results = U.sweep_slate_settings(model, dev, cache, scores, indices, labels, SETTINGS, K, 'remaining', per_impression=True)
    assert len(results) == len(SETTINGS)
    remaining = (dev.cand_lifetime - dev.cand_freshness).reshape(-1).float()
    slates = []
    for setting, res in zip(SETTINGS, results):
        want, positions, width = composed(model, dev, cache, scores, indices, labels, setting, K, remaining)
        check_setting(res, want, width, len(labels), '%s %s' % (name, setting))
        slates.append(positions)
    status = results[0]['status'].cpu().numpy()
    assert status[3] == 1 and status[5] == 2 and status[7] == 2 and (np.delete(status, [3, 5, 7]) == 0).all()
    assert all(np.array_equal(r['status'].cpu().numpy(), status) for r in results)
    # the settings are felt: the quota and the MMR each change some slate, and a quota of 1 leaves no topic twice in a slate
    assert not np.array_equal(slates[0], slates[1]) and not np.array_equal(slates[0], slates[2])
    per1 = results[1]['per_impression'].cpu().numpy()
    assert np.array_equal(per1[:, 5], per1[:, 6]) and results[1]['topics'] > results[0]['topics']
    assert results[2]['ild'] != results[0]['ild']
    want, _, width = composed(model, dev, cache, scores, indices, labels, {}, K, dev.cand_freshness.reshape(-1).float())
    check_setting(value, want, width, len(labels), name + ' value = freshness')
    # the whole entry raises for this split where the dev pass it runs raises
    with pytest.raises(ValueError, match='Only one class'):
        U.evaluate_cached_on_device(model, dev, indices, labels, rows_per_forward=PER)
    with pytest.raises(ValueError, match='Only one class'):
        U.evaluate_slates_on_device(model, dev, indices, labels, SETTINGS, k=K, rows_per_forward=PER)


@pytest.mark.parametrize('name', list(MODELS))
def test_the_entry_scores_once_and_returns_the_pass_beside_the_sweep(name, tmp_path):
    model, dev, indices, labels = split(name)
    n_imp = len(labels)
    assert labels[3] == [] and 38 <= n_imp <= 42 and min(len(l) for l in labels if l) >= 2 and max(len(l) for l in labels) > 20
    want_metrics, scores = U.evaluate_cached_on_device(model, dev, indices, labels, result_file=str(tmp_path / 'pass.txt'), rows_per_forward=PER,
                                                       return_scores=True)
    metrics, results = model.evaluate_slates(dev, indices, labels, SETTINGS, k=K, value='remaining', rows_per_forward=PER,
                                             per_impression=True, result_file=str(tmp_path / 'sweep.txt'))
    assert metrics == want_metrics                                     # bit for bit: the same pass
    assert (tmp_path / 'sweep.txt').read_bytes() == (tmp_path / 'pass.txt').read_bytes()
    cache = model.build_news_cache(dev.corpus)
    remaining = (dev.cand_lifetime - dev.cand_freshness).reshape(-1).float()
    for setting, res in zip(SETTINGS, results):
        want, _, width = composed(model, dev, cache, scores, indices, labels, setting, K, remaining)
        check_setting(res, want, width, n_imp, '%s %s' % (name, setting))
    # the plain setting at k = 10 and k = 5 is the pass's nDCG@10 and nDCG@5
    counted = sum(1 for l in labels if l and 0 < sum(l) < len(l))
    for k, col in ((10, 3), (5, 2)):
        m, (plain,) = U.evaluate_slates_on_device(model, dev, indices, labels, [{}], k=k, rows_per_forward=PER)
        assert m == want_metrics and plain['n_relevance'] == counted == n_imp - 1
        print('%s: plain nDCG@%d %.17g, the pass %.17g' % (name, k, plain['ndcg'], want_metrics[col]))
        assert abs(plain['ndcg'] - want_metrics[col]) <= n_imp * U53
        assert 'per_impression' not in plain and np.isnan(plain['value'])
    assert model.training is False


@pytest.mark.parametrize('name', list(MODELS))
def test_the_grouped_pass_gives_the_same_sweep(name):
    """The grouped scores equal the row-wise ones to fp32 rounding, so the statuses and the counted sets are the same and the metrics
    agree within the bar tests/test_lists_gpu.py sets for the scores.  (Two scores of an impression that rounding makes change places
    would move a slate entry; 40 impressions of up to 30 candidates leave no room to ask for a split without near-ties at that bar,
    as that file does for its 29 rows, so the split is the fixed one.)"""
    model, dev, indices, labels = split(name)
    kw = dict(k=K, value='freshness', rows_per_forward=PER, per_impression=True)
    m0, rows = U.evaluate_slates_on_device(model, dev, indices, labels, SETTINGS, **kw)
    m1, lists = U.evaluate_slates_on_device(model, dev, indices, labels, SETTINGS, grouped=True, **kw)
    assert rel_err(np.array(m1), np.array(m0)) <= TOL
    for setting, a, b in zip(SETTINGS, rows, lists):
        assert torch.equal(a['status'], b['status'])
        assert (a['n_relevance'], a['n_diversity'], a['n_slates']) == (b['n_relevance'], b['n_diversity'], b['n_slates'])
        got = np.array([b[name_] for name_ in U.SLATE_RESULT_KEYS])
        want = np.array([a[name_] for name_ in U.SLATE_RESULT_KEYS])
        print('%s %s: grouped - row-wise %s' % (name, setting, np.abs(got - want)))
        assert (np.abs(got - want) <= TOL * np.maximum(np.abs(want), 1.0)).all()


def test_trainer_with_slate_eval_keeps_its_rank_file_and_metrics(tmp_path, capsys):
    from lime_cikm25_amd.trainer import Trainer
    d = str(tmp_path)
    cfg, corpus, model = toy('CROWN', 'CROWN', batch_size=8, epoch=1, lr=1e-3, dataset='adressa', model_dir=d + '/models',
                             best_model_dir=d + '/best', dev_res_dir=d + '/dev/res', result_dir=d + '/results')
    np.random.seed(0)
    plain = Trainer(model, cfg, corpus, run_index=1, device_eval=True)
    sweep = Trainer(model, cfg, corpus, run_index=2, device_eval=True, slate_eval=dict(settings=SETTINGS[:2], k=3))
    assert plain.slate_eval is None and plain.last_slate_metrics is None and sweep.last_slate_metrics is None
    a = plain.evaluate(1)
    b = sweep.evaluate(1)
    name = model.model_name
    assert (open(os.path.join(sweep.dev_res_dir, '%s-1.txt' % name), 'rb').read()
            == open(os.path.join(plain.dev_res_dir, '%s-1.txt' % name), 'rb').read())
    assert a == b and all(isinstance(v, float) for v in b)            # bit-equal: the same pass
    assert len(sweep.last_slate_metrics) == 2 and set(sweep.last_slate_metrics[0]) == set(U.SLATE_RESULT_KEYS) | {'n_relevance', 'n_diversity',
                                                                                                                    'n_slates'}
    assert capsys.readouterr().out.count('slates {') == 2
    with pytest.raises(ValueError, match='max_per_topic'):
        Trainer(model, cfg, corpus, run_index=3, device_eval=True, slate_eval=dict(settings=[{'max_per_topic': 0}]))
    assert sweep.train() == 1 and len(sweep.results['auc']) == 1 and len(sweep.last_slate_metrics) == 2


def test_recommend_lists_returns_what_it_returned():
    """The tail of recommend_lists is serving.select_segments now: positions and scores equal the tail as it stood, called piece by piece."""
    model, dev, indices, labels = split('lime_crown_crown')
    cache = model.build_news_cache(dev.corpus)
    runs = U.impression_runs(indices, 0, dev.num)
    first = torch.from_numpy(runs[:-1]).cuda()
    users = (dev.hist_index[first], dev.hist_mask[first], dev.user_freshness[first], dev.user_lifetime[first])
    cands = (runs, dev.cand_index.reshape(-1), dev.cand_freshness.reshape(-1), dev.cand_lifetime.reshape(-1))
    for kw in (dict(), dict(max_per_topic=1), dict(mmr_lambda=0.5, shortlist=8), dict(max_per_topic=2, mmr_lambda=0.3, shortlist=16)):
        got_p, got_s = model.recommend_lists(cache, dev.corpus, *users, *cands, k=K, exclude_history=True, **kw)
        scores, offsets, gone = serving.score_lists(model, cache, dev.corpus, *users, *cands, None, 1 << 18, True, k=K)
        quota = serving.topic_quota(dev.corpus, kw.get('max_per_topic'), 'category')
        div = serving.diversity(model, cache, K, kw.get('mmr_lambda'), kw.get('shortlist'), None)
        if div is None:
            want_p, want_s = serving._top_segments(scores, offsets, gone, quota, cands[1], K)
        else:
            positions, top = serving._top_segments(scores, offsets, gone, quota, cands[1], div.shortlist)
            pair = (offsets[:-1].unsqueeze(1) + positions.clamp(min=0).long()).clamp(max=scores.numel() - 1)
            ids = torch.where(positions >= 0, cands[1].to(torch.int32)[pair], torch.full_like(positions, -1))
            want_p, want_s = serving._diverse(div, positions, top, ids, K)
        assert torch.equal(got_p, want_p) and torch.equal(got_s.view(torch.int32), want_s.view(torch.int32)), kw
        assert got_p.shape == (len(labels), K) and (got_p >= 0).any()
