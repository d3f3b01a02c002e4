"""The device-side dev pass on the MI355X: ops.rank_metrics (csrc/rank_metrics.hip) against util.rank_impressions (exact ranks,
byte-identical rank files) and evaluate.scoring / the eval goldens (metrics within the project's 1e-12), its status codes, its
run-to-run and grid-to-grid bitwise reproducibility, and util.evaluate_cached_on_device / Trainer(device_eval=True) against the
host-side cached pass on the toy corpus."""
import io
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, rel_err
from test_rank_metrics_cpu import files, golden, ragged_case, truth_of
from lime_cikm25_amd import Model, evaluate as E, formats, make_config, ops
from lime_cikm25_amd import util as U
from lime_cikm25_amd.device_data import DeviceBehaviors, DeviceCorpus

pytestmark = pytest.mark.gpu
ATOL = 1e-12                    # the project's bound for these metrics (tests/test_eval_harness.py): the sums have at most a few thousand
                                # fp64 terms of magnitude <= 1
KTOL = 2e-5                     # fp32-level kernel against the same sums in another order (tests/test_user_encoders_gpu.py)


def run_op(scores, indices, labels, **kw):
    off, lab, skip = E.impression_layout(indices, labels)
    s = torch.tensor(scores, dtype=torch.float32).cuda()
    res = ops.rank_metrics(s, torch.from_numpy(lab).cuda(), off, torch.from_numpy(skip).cuda(), **kw)
    torch.cuda.synchronize()
    return res


def check_against_host(scores, indices, labels, res, tmp_path, rank_file=None):
    """ranks exact, per-impression metrics and means within ATOL of evaluate.scoring (and of the closed forms' host twin)."""
    want_ranks = U.rank_impressions(scores, indices)
    got_ranks = U.ranks_to_lists(res.ranks, indices)
    assert got_ranks == want_ranks
    path = tmp_path / 'ranks.txt'
    U.write_rank_file(str(path), got_ranks)
    if rank_file is not None:
        assert path.read_text() == rank_file
    n_imp = len(labels)
    want_ranks = want_ranks + [[]] * (n_imp - len(want_ranks))
    per, status = res.per_impression.cpu().numpy(), res.status.cpu().numpy()
    twin, twin_status = E.metrics_from_ranks(want_ranks, labels, per_impression=True)
    assert status.tolist() == twin_status.tolist()
    worst = 0.0
    for i in range(n_imp):
        if status[i] == 0:
            one = np.array(E.scoring(*files([labels[i]], [want_ranks[i]])))
            worst = max(worst, float(np.abs(per[i] - one).max()))
        else:
            assert (per[i] == 0).all()
    print('per impression: max |kernel - scoring| %.3e, max |kernel - host twin| %.3e' % (worst, float(np.abs(per - twin).max())))
    assert worst <= ATOL and np.allclose(per, twin, rtol=0, atol=ATOL)
    counted = int((status == 0).sum())
    assert int(res.count.cpu()[0]) == counted
    if counted and not (status >= 2).any():
        want = np.array(E.scoring(*files(labels, want_ranks)))
        print('means: max |kernel - scoring| %.3e' % float(np.abs(np.array(res.means()) - want).max()))
        assert np.allclose(res.means(), want, rtol=0, atol=ATOL)
    return per, status


@pytest.mark.parametrize('name', ['eval_plain', 'eval_ties'])
def test_goldens_ranks_exact_and_metrics_within_bound(name, tmp_path):
    g = golden(name)
    labels = truth_of(g)
    res = run_op(g['scores'], g['indices'], labels)
    check_against_host(g['scores'], g['indices'], labels, res, tmp_path, rank_file=g['rank_file'])
    print(name, 'means - golden: %.3e' % float(np.abs(np.array(res.means()) - np.array(g['metrics'])).max()))
    assert np.allclose(res.means(), g['metrics'], rtol=0, atol=ATOL)
    metrics, ranks = E.device_scoring(torch.tensor(g['scores'], dtype=torch.float32).cuda(), g['indices'], labels)
    assert torch.equal(ranks, res.ranks) and metrics == res.means()
    assert all(isinstance(v, float) for v in metrics)


def test_signed_zeros_ties_and_tiny_impressions(tmp_path):
    """The tie example of tests/test_eval_harness.py, an impression with one row, one with no rows."""
    scores = [0.0, -0.0, 1.0, 0.0, 1.0, -3.0] + [2.0] + [1.0, 5.0]
    indices = [0] * 6 + [1] + [3, 3]
    labels = [[0, 1, 0, 0, 1, 0], [1], [], [1, 0]]
    res = run_op(scores, indices, labels)
    assert U.ranks_to_lists(res.ranks, indices) == [[3, 4, 1, 5, 2, 6], [1], [], [2, 1]]
    _, status = check_against_host(scores, indices, labels, res, tmp_path)
    assert status.tolist() == [0, 2, 1, 0]
    # no impressions at all / no rows at all
    empty = ops.rank_metrics(torch.empty(0).cuda(), torch.empty(0, dtype=torch.uint8).cuda(), [0])
    assert empty.ranks.numel() == 0 and int(empty.count.cpu()[0]) == 0 and (empty.sums.cpu() == 0).all()
    empty = ops.rank_metrics(torch.empty(0).cuda(), torch.empty(0, dtype=torch.uint8).cuda(), [0, 0, 0])
    assert empty.status.cpu().tolist() == [1, 1] and int(empty.count.cpu()[0]) == 0


def test_both_sides_of_the_wave_workgroup_switch_and_a_long_impression(tmp_path):
    """Impressions of 63 .. 65 rows (one or two row blocks of a wave), 511 .. 513 rows (the last a wave takes, the first the workgroup
    takes), 2049 rows (two j tiles) and 5000 rows (five row blocks of the workgroup, three j tiles), with heavy ties."""
    rng = np.random.default_rng(5)
    scores, indices, labels = [], [], []
    for i, n in enumerate([63, 64, 65, 511, 512, 513, 3, 2049, 5000, 40]):
        s = np.round(rng.normal(size=n), 1).astype(np.float32)
        s[rng.random(n) < 0.1] = 0.0
        s[rng.random(n) < 0.05] = -0.0
        y = (rng.random(n) < 0.2).astype(np.int64)
        y[0], y[n - 1] = 1, 0
        scores += s.tolist()
        indices += [i] * n
        labels.append(y.tolist())
    res = run_op(scores, indices, labels)
    _, status = check_against_host(scores, indices, labels, res, tmp_path)
    assert (status == 0).all()


def test_status_codes_and_the_errors_of_device_scoring():
    scores = [0.3, 0.1, 0.2, 0.9, 0.8, 0.5, 0.4, 0.7, 0.6, 0.2]
    indices = [0, 0, 0, 1, 1, 2, 2, 3, 3, 3]
    labels = [[1, 0, 0], [], [0, 1], [0, 1, 0]]
    res = run_op(scores, indices, labels)
    assert res.status.cpu().tolist() == [0, 1, 0, 0]
    # the skipped impression is ranked, and left out of the means as scoring leaves it out
    ranks = U.ranks_to_lists(res.ranks, indices)
    assert ranks == U.rank_impressions(scores, indices) and ranks[1] == [1, 2]
    want = E.scoring(*files(labels, ranks))
    assert int(res.count.cpu()[0]) == 3 and np.allclose(res.means(), want, rtol=0, atol=ATOL)
    dev_scores = torch.tensor(scores, dtype=torch.float32).cuda()
    got, _ = E.device_scoring(dev_scores, indices, labels)
    assert np.allclose(got, want, rtol=0, atol=ATOL)
    # one class only: status 2, the error of roc_auc_score from device_scoring (scoring raises it as well)
    one_class = [[1, 0, 0], [], [1, 1], [0, 1, 0]]
    assert run_op(scores, indices, one_class).status.cpu().tolist() == [0, 1, 2, 0]
    with pytest.raises(ValueError, match='Only one class'):
        E.device_scoring(dev_scores, indices, one_class)
    with pytest.raises(ValueError, match='Only one class'):
        E.scoring(*files(one_class, ranks))
    # a NaN score, a label outside {0, 1}: status 3
    nan_scores = list(scores)
    nan_scores[8] = float('nan')
    assert run_op(nan_scores, indices, labels).status.cpu().tolist() == [0, 1, 0, 3]
    with pytest.raises(ValueError, match='NaN'):
        E.device_scoring(torch.tensor(nan_scores, dtype=torch.float32).cuda(), indices, labels)
    assert run_op(scores, indices, [[1, 0, 0], [], [0, 1], [0, 2, 0]]).status.cpu().tolist() == [0, 1, 0, 3]


def test_wrong_dtypes_and_shapes_are_refused():
    s, y = torch.zeros(4).cuda(), torch.zeros(4, dtype=torch.uint8).cuda()
    with pytest.raises(TypeError):
        ops.rank_metrics(s.double(), y, [0, 4])
    with pytest.raises(TypeError):
        ops.rank_metrics(s, y.long(), [0, 4])
    with pytest.raises(TypeError):
        ops.rank_metrics(s, y.cpu(), [0, 4])
    with pytest.raises(ValueError):
        ops.rank_metrics(s, y[:3], [0, 4])
    with pytest.raises(ValueError):
        ops.rank_metrics(s, y, [0, 2, 4], skip=torch.zeros(3, dtype=torch.uint8).cuda())
    with pytest.raises(TypeError):
        ops.rank_metrics(s, y, torch.tensor([0, 4]).cuda())                      # int64 offsets on the device
    with pytest.raises(ValueError, match='non-decreasing'):
        ops.rank_metrics(s, y, torch.tensor([0, 3, 2, 4], dtype=torch.int32).cuda())
    ok = ops.rank_metrics(s, y, torch.tensor([0, 4], dtype=torch.int32).cuda())
    assert ok.status.cpu().tolist() == [2] and ok.ranks.cpu().tolist() == [1, 2, 3, 4]


def test_bitwise_reproducible_and_independent_of_the_grids():
    scores, indices, labels = ragged_case(7, n_imp=3000, max_rows=120)
    for i in (100, 2000):                                                        # two impressions for the workgroup form
        extra = 700
        at = indices.index(i)
        scores[at:at] = [0.5] * extra
        indices[at:at] = [i] * extra
        labels[i] = [0, 1] * (extra // 2) + labels[i]
    a = run_op(scores, indices, labels)
    b = run_op(scores, indices, labels)
    c = run_op(scores, indices, labels, rank_blocks=3, reduce_blocks=1)
    d = run_op(scores, indices, labels, rank_blocks=97, reduce_blocks=2)
    assert int(a.count.cpu()[0]) == 3000
    for other in (b, c, d):
        assert torch.equal(a.sums, other.sums) and torch.equal(a.count, other.count)        # bitwise: fp64 compared for equality
        assert torch.equal(a.per_impression, other.per_impression) and torch.equal(a.ranks, other.ranks)
        assert torch.equal(a.status, other.status)
    want = E.metrics_from_ranks(U.rank_impressions(scores, indices), labels)
    assert np.allclose(a.means(), want, rtol=0, atol=ATOL)


# ---- the whole pass on the toy corpus ---------------------------------------------------------------------------------------------
def toy(content, user, batch_size=16, **kw):
    g = json.load(open(os.path.join(GOLDEN_DIR, 'formats.json')))
    L = g['lines']
    cfg = make_config(content_encoder=content, user_encoder=user, max_history_num=g['max_history_num'], max_title_length=g['max_title_length'],
                      max_abstract_length=g['max_abstract_length'], vocabulary_size=len(g['word_dict']), negative_sample_num=2,
                      category_num=len(g['category_dict']) + 1, subCategory_num=len(g['subCategory_dict']) + 1,
                      user_num=len(g['user_ID_dict']), batch_size=batch_size, **kw)
    corpus = formats.build_corpus(cfg, [L['train_news'], L['dev_news'], L['test_news']],
                                  [L['train_behaviors'], L['dev_behaviors'], L['test_behaviors']], g['news_ID_dict'],
                                  g['user_ID_dict'], g['category_dict'], g['subCategory_dict'], g['word_dict'], dataset='adressa')
    torch.manual_seed(0)
    model = Model(cfg)
    model.initialize()
    torch.nn.init.normal_(model.news_encoder.base_news_encoder.word_embedding.weight, std=0.1)
    return cfg, corpus, model.cuda(), formats.truth_labels(L['dev_behaviors'])


def chunk_scores(model, dev, per):
    """The scores of compute_scores_cached, which keeps them to itself: its own loop, one forward per chunk of ``per`` rows."""
    model.eval()
    cache = model.build_news_cache(dev.corpus)
    out = []
    for r0 in range(0, dev.num, per):
        rows = list(range(r0, min(dev.num, r0 + per)))
        out.append(model.score_behaviors(dev, rows, cache, n_src=len(rows)).float().cpu())
    model.train()
    return torch.cat(out).numpy()


@pytest.mark.parametrize('content,user', [('CROWN', 'CROWN'), ('NAML', 'ATT')])
def test_device_pass_agrees_with_the_cached_host_pass(content, user, tmp_path):
    cfg, corpus, model, labels = toy(content, user, batch_size=6)
    assert labels == corpus.dev_labels
    dev = DeviceBehaviors.from_devtest(DeviceCorpus(corpus), corpus, 'dev')
    truth = formats.write_truth_file(str(tmp_path / 'truth.txt'), labels)
    per = cfg.batch_size
    assert dev.num >= 3 * per and dev.num % per, 'the toy dev split must give several full chunks and a short one'
    model.train()
    host = U.compute_scores_cached(model, dev, corpus.dev_indices, str(tmp_path / 'host.txt'), truth, rows_per_forward=per)
    # rows_per_pass == rows_per_forward: the same forwards -- scores, rank file and metrics identical
    same = U.evaluate_cached_on_device(model, dev, corpus.dev_indices, labels, result_file=str(tmp_path / 'same.txt'),
                                       rows_per_forward=per, rows_per_pass=per)
    assert model.training                                                        # mode restored
    assert (tmp_path / 'same.txt').read_text() == (tmp_path / 'host.txt').read_text()
    print(content, user, 'metrics, device - host:', np.abs(np.array(same) - np.array(host)).max())
    assert np.allclose(same, host, rtol=0, atol=ATOL)
    host_scores = chunk_scores(model, dev, per)
    assert U.rank_impressions(host_scores.tolist(), corpus.dev_indices) == [json.loads(l.split(' ', 1)[1]) for l in open(tmp_path / 'host.txt')]
    _, same_scores = U.evaluate_cached_on_device(model, dev, corpus.dev_indices, labels, rows_per_forward=per, rows_per_pass=per,
                                                 return_scores=True)
    assert np.array_equal(same_scores.cpu().numpy(), host_scores)
    # many chunks per pass (the default): every score within the kernel-level bound of the chunk-by-chunk scores
    big, big_scores = U.evaluate_cached_on_device(model, dev, corpus.dev_indices, labels, result_file=str(tmp_path / 'big.txt'),
                                                  rows_per_forward=per, return_scores=True)
    big_scores = big_scores.cpu().numpy()
    assert big_scores.shape == host_scores.shape == (dev.num,)
    e = rel_err(big_scores, host_scores)
    print(content, user, 'scores, many chunks a pass against one: rel err %.3e over %d rows' % (e, dev.num))
    assert e < KTOL
    want_ranks = U.rank_impressions(big_scores.tolist(), corpus.dev_indices)
    assert [json.loads(l.split(' ', 1)[1]) for l in open(tmp_path / 'big.txt')] == want_ranks
    assert np.allclose(big, E.scoring(open(truth), open(tmp_path / 'big.txt')), rtol=0, atol=ATOL)
    if user == 'CROWN':                                                          # the GraphSAGE node-slot bound is kept
        with pytest.raises(ValueError, match='node slots'):
            U.evaluate_cached_on_device(model, dev, corpus.dev_indices, labels, rows_per_forward=cfg.max_history_num + cfg.batch_size + 1)
    cfg.lifetime_type = 'nope'
    with pytest.raises(ValueError, match='lifetime_type'):
        U.evaluate_cached_on_device(model, dev, corpus.dev_indices, labels)


def test_trainer_with_device_eval_writes_the_same_rank_file(tmp_path):
    from lime_cikm25_amd.trainer import Trainer
    d = str(tmp_path)
    cfg, corpus, model, labels = toy('CROWN', 'CROWN', batch_size=8, epoch=1, lr=1e-3, dataset='adressa', model_dir=d + '/models',
                                     best_model_dir=d + '/best', dev_res_dir=d + '/dev/res', result_dir=d + '/results')
    np.random.seed(0)
    plain = Trainer(model, cfg, corpus, run_index=1)
    fused = Trainer(model, cfg, corpus, run_index=2, device_eval=True)
    assert plain.device_eval is False and fused.device_eval is True and fused.cached_eval
    a = plain.evaluate(1)
    b = fused.evaluate(1)
    name = model.model_name
    assert open(os.path.join(fused.dev_res_dir, '%s-1.txt' % name)).read() == open(os.path.join(plain.dev_res_dir, '%s-1.txt' % name)).read()
    print('trainer metrics, device - host:', np.abs(np.array(a) - np.array(b)).max())
    assert np.allclose(a, b, rtol=0, atol=ATOL) and all(isinstance(v, float) for v in b)
    assert fused.train() == 1 and len(fused.results['auc']) == 1                 # the loop runs on the device pass
