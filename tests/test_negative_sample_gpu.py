"""Negative sampling on the MI355X: lime_negative_sample (csrc/negative_sample.hip, ops.negative_sample) behind
DeviceBehaviors.train_resident / resample against its host twin device_data.counter_negative_sampling, bit for bit; the tables refilled
in place under plans that stay valid; the launch inside a HIP graph; and whole epochs of Trainer(device_sampling=True) against the same
epoch stepped by hand over from_train(twin)."""
import json
import os

import numpy as np
import pytest
import torch

import negative_sample_cases as cases
from helpers import GOLDEN_DIR
from lime_cikm25_amd import DeviceBehaviors, DeviceCorpus, Model, distributed, formats, make_config, ops, synth
from lime_cikm25_amd import device_data, trainer as trainer_mod
from lime_cikm25_amd.device_data import counter_negative_sampling
from lime_cikm25_amd.training import TrainStep

pytestmark = pytest.mark.gpu

BIG = 100003                    # records of the large split: 391 workgroups of 256 threads, the last one partly filled


def small_cfg(**kw):
    return make_config(max_history_num=6, max_title_length=8, max_abstract_length=16, batch_size=4, vocabulary_size=3000, **kw)


_SPLITS = {}


def split(name):
    """(cfg, corpus, DeviceCorpus) of the three sizes: one record, the 40-record toy corpus, BIG records with 1 .. 71 non-clicked news."""
    if name not in _SPLITS:
        cfg = small_cfg()
        if name == 'one':
            corpus = cases.split(cfg, [9])
        elif name == 'toy':
            corpus = synth.synth_corpus(cfg, n_train=40, n_neg_max=9)
            assert len(corpus.train_behaviors) == 40
        else:
            corpus = cases.split(cfg, cases.mixed_counts(BIG, seed=2), seed=2)
        _SPLITS[name] = (cfg, corpus, DeviceCorpus(corpus))
    return _SPLITS[name]


def same_tables(beh, want):
    idx, fr, lt = (torch.from_numpy(a) for a in cases.tables(*want))
    return (torch.equal(beh.cand_index.cpu(), idx) and torch.equal(beh.cand_freshness.cpu(), fr) and torch.equal(beh.cand_lifetime.cpu(), lt))


@pytest.mark.parametrize('name', ['one', 'toy', 'big'])
@pytest.mark.parametrize('K', [1, 4, 8])
def test_kernel_equals_the_host_twin_bit_for_bit(name, K):
    cfg, corpus, dc = split(name)
    beh = DeviceBehaviors.train_resident(dc, corpus, K)
    assert beh.cand_index.shape == (len(corpus.train_behaviors), 1 + K) and beh.cand_index.dtype == torch.int32
    for inclusive in (False, True):
        beh.resample(3, 5, inclusive)
        assert beh.sampled == (3, 5, inclusive)
        assert same_tables(beh, counter_negative_sampling(corpus.train_behaviors, K, 3, 5, inclusive)), (name, K, inclusive)
    if name == 'big':                                              # the draws do differ between the two modes and between epochs
        a = beh.cand_index.clone()
        assert not torch.equal(beh.resample(3, 5, False).cand_index, a) and not torch.equal(beh.resample(3, 6, True).cand_index, a)


def test_wrapper_allocates_when_no_output_is_given_and_checks_shapes():
    cfg, corpus, dc = split('toy')
    beh = DeviceBehaviors.train_resident(dc, corpus, 4).resample(1, 1)
    g = beh._neg
    idx, fr, lt = ops.negative_sample(g['offsets'], g['index'], g['lifetime'], g['pos_index'], g['pos_lifetime'], g['freshness'], 4, 1, 1)
    assert torch.equal(idx, beh.cand_index) and torch.equal(fr, beh.cand_freshness) and torch.equal(lt, beh.cand_lifetime)
    with pytest.raises(ValueError):
        ops.negative_sample(g['offsets'], g['index'], g['lifetime'], g['pos_index'], g['pos_lifetime'], g['freshness'], 3, 1, 1,
                            cand_index=beh.cand_index)
    with pytest.raises(ValueError):
        ops.negative_sample(g['offsets'], g['index'], g['lifetime'], g['pos_index'], g['pos_lifetime'], g['freshness'], 17, 1, 1)
    with pytest.raises(ValueError):
        ops.negative_sample(g['offsets'][:-1], g['index'], g['lifetime'], g['pos_index'], g['pos_lifetime'], g['freshness'], 4, 1, 1)
    with pytest.raises(ValueError, match='train_resident'):
        DeviceBehaviors.from_devtest(dc, corpus, 'dev').resample(1, 1)
    with pytest.raises(ValueError, match='resample'):
        DeviceBehaviors.train_resident(dc, corpus, 4).assemble([0, 1])
    bad = cases.split(cfg, [3, 4, 5])
    bad.train_behaviors[1][4], bad.train_behaviors[1][8] = [], []
    with pytest.raises(ValueError, match=r'record 1\b'):
        DeviceBehaviors.train_resident(dc, bad, 4)


def test_fixed_tables_equal_from_train():
    """train_resident builds the history tables in one vectorised pass: the same bits as from_train's per-record build."""
    cfg, corpus, dc = split('toy')
    K = cfg.negative_sample_num
    twin = counter_negative_sampling(corpus.train_behaviors, K, 2, 1)
    a, b = DeviceBehaviors.train_resident(dc, corpus, K).resample(2, 1), DeviceBehaviors.from_train(dc, corpus, *twin)
    for name in ('user_id', 'hist_index', 'hist_mask', 'user_freshness', 'user_lifetime', 'cand_index', 'cand_freshness', 'cand_lifetime'):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), name


def test_resample_is_in_place_and_first_epoch_plans_stay_valid():
    cfg, corpus, dc = split('toy')
    K = cfg.negative_sample_num
    beh = DeviceBehaviors.train_resident(dc, corpus, K).resample(9, 1)
    names = ('cand_index', 'cand_freshness', 'cand_lifetime', 'hist_index', 'hist_mask', 'user_freshness', 'user_lifetime', 'user_id')
    ptrs = [getattr(beh, n).data_ptr() for n in names]
    rows = [5, 0, 39, 17, 17, 22, 8]
    first = [t.clone() for t in beh.assemble(rows)]                # creates the plans of this batch size, in epoch 1
    beh.assemble(rows)                                             # ... both workspaces of the ring
    plans = [id(p) for p in beh._plans[len(rows)]]
    epoch1 = beh.cand_index.clone()
    beh.resample(9, 2)
    assert not torch.equal(beh.cand_index, epoch1), 'epoch 2 drew what epoch 1 drew'
    assert [getattr(beh, n).data_ptr() for n in names] == ptrs
    got = beh.assemble(rows)
    assert [id(p) for p in beh._plans[len(rows)]] == plans
    want = DeviceBehaviors.from_train(dc, corpus, *counter_negative_sampling(corpus.train_behaviors, K, 9, 2)).assemble(rows)
    assert len(got) == len(want) == 25
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), 'output %d' % k
    assert all(torch.equal(a, b) for a, b in zip(first[:15], got[:15])), 'the history side of a batch does not depend on the epoch'


def test_the_launch_neither_allocates_nor_synchronises():
    """Graph safety: resample records into a HIP graph on one stream (an allocation or a synchronise inside the capture would fail
    it), and the replay gives the eager bits."""
    cfg, corpus, dc = split('big')
    beh = DeviceBehaviors.train_resident(dc, corpus, 4)
    eager = [t.clone() for t in (beh.resample(4, 7).cand_index, beh.cand_freshness, beh.cand_lifetime)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            beh.resample(4, 7)
    for t in (beh.cand_index, beh.cand_freshness, beh.cand_lifetime):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((beh.cand_index, beh.cand_freshness, beh.cand_lifetime), eager))


# ---- whole epochs on the toy dataset of tests/test_end_to_end_gpu.py -------------------------------------------------------------------
def toy_dataset(tmp, tag):
    g = json.load(open(os.path.join(GOLDEN_DIR, 'formats.json')))
    L = g['lines']
    d = os.path.join(str(tmp), tag)
    cfg = make_config(max_history_num=g['max_history_num'], max_title_length=g['max_title_length'],
                      max_abstract_length=g['max_abstract_length'], vocabulary_size=len(g['word_dict']), negative_sample_num=2,
                      category_num=len(g['category_dict']) + 1, subCategory_num=len(g['subCategory_dict']) + 1,
                      user_num=len(g['user_ID_dict']), batch_size=4, epoch=3, lr=1e-3, dataset='adressa',
                      model_dir=d + '/models', best_model_dir=d + '/best', dev_res_dir=d + '/dev/res', result_dir=d + '/results')
    corpus = formats.build_corpus(cfg, [L['train_news'], L['dev_news'], L['test_news']],
                                  [L['train_behaviors'], L['dev_behaviors'], L['test_behaviors']], g['news_ID_dict'],
                                  g['user_ID_dict'], g['category_dict'], g['subCategory_dict'], g['word_dict'], dataset='adressa')
    torch.manual_seed(0)
    np.random.seed(0)
    model = Model(cfg)
    model.initialize()
    torch.nn.init.normal_(model.news_encoder.base_news_encoder.word_embedding.weight, std=0.1)
    return cfg, corpus, model.cuda()


def run_trainer(tmp, tag, **kw):
    cfg, corpus, model = toy_dataset(tmp, tag)
    t = trainer_mod.Trainer(model, cfg, corpus, run_index=1, **kw)
    losses, inner = [], t.train_epoch
    t.train_epoch = lambda e: losses.append(inner(e)) or losses[-1]
    best = t.train()
    return t, losses, best


def test_trainer_with_device_sampling_runs_and_repeats_bitwise(tmp_path, monkeypatch):
    calls = []
    host = device_data.negative_sampling
    monkeypatch.setattr(trainer_mod, 'negative_sampling', lambda *a, **k: calls.append(1) or host(*a, **k))
    a, losses_a, best = run_trainer(tmp_path, 'a', device_sampling=True)
    assert a.device_sampling and a.train_split is not None and a.train_split.sampled == (0, 3, False)
    assert not calls, 'device_sampling=True still sampled on the host'
    assert len(losses_a) == 3 and all(np.isfinite(losses_a)) and 1 <= best <= 3
    assert len(a.results['auc']) == 3 and all(0.0 <= v <= 1.0 for k in a.results for v in a.results[k])
    assert len(a.train_split._plans) <= 2                          # one full batch size (+ the tail's), built once for the run
    b, losses_b, _ = run_trainer(tmp_path, 'b', device_sampling=True)
    assert losses_a == losses_b, (losses_a, losses_b)              # Python floats of fp32 means: equality is bitwise
    assert a.results == b.results

    # epoch 1 by hand over from_train(twin): the same permutation, the same batches, the same step -> the same loss, bit for bit
    cfg, corpus, model = toy_dataset(tmp_path, 'c')
    dc = DeviceCorpus(corpus)
    train = DeviceBehaviors.from_train(dc, corpus, *counter_negative_sampling(corpus.train_behaviors, cfg.negative_sample_num, cfg.seed, 1))
    step = TrainStep(model, lr=cfg.lr, weight_decay=cfg.weight_decay, gradient_clip_norm=cfg.gradient_clip_norm)
    order = np.random.RandomState(cfg.seed + 1).permutation(train.num)
    rows = distributed.sampler_rows(train.num, 0, 1, order)
    model.train()
    total, seen = 0.0, 0
    for i in range(0, len(rows), cfg.batch_size):
        chunk = [int(r) for r in rows[i:i + cfg.batch_size]]
        batch = train.assemble(chunk)
        total += float(step.step(*batch, batch[24] - batch[23])) * len(chunk)
        seen += len(chunk)
    assert total / seen == losses_a[0], (total / seen, losses_a[0])


def test_trainer_without_the_flag_samples_on_the_host_as_before(tmp_path, monkeypatch):
    calls = []
    host = device_data.negative_sampling
    monkeypatch.setattr(trainer_mod, 'negative_sampling', lambda *a, **k: calls.append(1) or host(*a, **k))
    t, losses, _ = run_trainer(tmp_path, 'plain')
    assert not t.device_sampling and t.train_split is None
    assert len(calls) == 3 == len(losses) and all(np.isfinite(losses))
