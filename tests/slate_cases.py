"""Generators the slate-metrics tests share (tests/test_slate_metrics_cpu.py, test_slate_metrics_gpu.py, test_slate_eval_gpu.py): seeded
operands of ops.slate_metrics / recommend.slate_metrics, the ragged impressions of tests/test_rank_metrics_cpu.py (stated again here: a
test module is not imported for its generator), and the synthetic dev splits and tiny models of the end-to-end tests."""
import json
import os

import numpy as np

from helpers import GOLDEN_DIR
from user_cases import _TINY

N_NEWS = 60


def ragged_case(seed, n_imp=400, max_rows=299):
    """Seeded ragged impressions with heavy ties (scores rounded to one decimal, +0.0 / -0.0 planted); every impression has at least
    two rows, at least one positive and at least one negative.  (tests/test_rank_metrics_cpu.py's generator, draw for draw.)"""
    rng = np.random.default_rng(seed)
    scores, indices, labels = [], [], []
    for i in range(n_imp):
        n = int(rng.integers(2, max_rows + 1))
        s = np.round(rng.normal(size=n), 1).astype(np.float32)
        s[rng.random(n) < 0.1] = 0.0
        s[rng.random(n) < 0.05] = -0.0
        y = (rng.random(n) < rng.choice([0.05, 0.3, 0.7])).astype(np.int64)
        a, b = rng.choice(n, 2, replace=False)
        y[a], y[b] = 1, 0
        assert 0 < y.sum() < n
        scores += s.tolist()
        indices += [i] * n
        labels.append(y.tolist())
    return scores, indices, labels


def slate_case(seed, R, k, ldp=None, E=64, n=50, n_keys=7, pool=False, max_len=30, lens=None, labels=True, skip=True, value=True,
               table=True, keys=True):
    """Seeded operands of slate_metrics as a dict of numpy arrays (an absent optional one: None).  List form: R lists of 0 ..
    ``max_len`` rows (``lens``: the first lists' lengths, the rest drawn), positions a random order of each list's rows cut at
    ``ldp`` with -1 behind the list's end; pool form (``pool``): one pool of ``max_len`` rows.  Planted: slates of -1 alone, a -1 in
    the middle of a slate, a position twice in a slate, a zero row (news 0) and two equal rows (news 1, 2) in the table, a news id
    outside [0, n), labels of value 2, impressions of one class, skipped slates, keys outside [0, n_keys)."""
    rng = np.random.default_rng(seed)
    ldp = k if ldp is None else ldp
    if pool:
        P, offsets = max_len, None
        length = np.full(R, P, dtype=np.int64)
    else:
        length = rng.integers(0, max_len + 1, size=R).astype(np.int64)
        if lens is not None:
            length[:min(R, len(lens))] = lens[:R]
        offsets = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
        P = int(offsets[-1])
    W = max(int(length.max()) if R else 0, ldp, 1)
    order = np.argsort(rng.random((R, W)) + 2.0 * (np.arange(W)[None, :] >= length[:, None]), axis=1)
    positions = np.where(np.arange(W)[None, :] < length[:, None], order, -1)[:, :ldp].astype(np.int32)
    if R:
        hole = rng.random(R) < 0.2
        positions[hole, rng.integers(0, k, size=int(hole.sum()))] = -1                   # a -1 in the middle keeps its slot
        twice = (rng.random(R) < 0.2) & (length > 0)
        if k > 1:
            positions[twice, k - 1] = positions[twice, 0]                                 # one row in two slots
        positions[rng.random(R) < 0.05] = -1                                              # a slate of -1 alone
    news = rng.integers(0, n, size=max(P, 1)).astype(np.int32)[:P]
    if P > 3:
        news[rng.integers(0, P, size=max(1, P // 50))] = n + 3                            # an id outside the tables: an empty slot
        news[rng.integers(0, P, size=max(1, P // 50))] = -2
    case = dict(positions=positions, k=k, offsets=offsets, news=news, labels=None, skip=None, value=None, table=None, keys=None, n=n,
                n_keys=n_keys, R=R, P=P, E=E)
    if labels and not pool:
        y = (rng.random(P) < 0.3).astype(np.uint8)
        for r in np.flatnonzero(rng.random(R) < 0.05):                                    # a label outside {0, 1}
            if length[r]:
                y[offsets[r] + rng.integers(0, length[r])] = 2
        for r in np.flatnonzero(rng.random(R) < 0.1):                                     # one class only
            y[offsets[r]:offsets[r + 1]] = rng.integers(0, 2)
        case['labels'] = y
    if skip:
        case['skip'] = (rng.random(R) < 0.1).astype(np.uint8)
    if value:
        case['value'] = (rng.normal(size=P) * 1000.0).astype(np.float32)
    if table:
        t = rng.normal(size=(n, E)).astype(np.float32)
        t[0] = 0.0
        if n > 2:
            t[2] = t[1]
        case['table'] = t
    if keys:
        key = rng.integers(0, n_keys, size=n).astype(np.int32)
        if n > 4:
            key[3], key[4] = -1, n_keys
        case['keys'] = key
    return case


def host_metrics(case, k=None):
    """recommend.slate_metrics on a case's arrays -> (per_slate, status, sums, counts)."""
    from lime_cikm25_amd import recommend
    return recommend.slate_metrics(case['positions'], case['k'] if k is None else k, case['offsets'], case['news'], case['labels'], case['skip'],
                                   case['value'], case['table'], case['keys'], n=case['n'], n_keys=case['n_keys'])


# ---- the end-to-end splits ---------------------------------------------------------------------------------------------------------
MODELS = {'lime_crown_crown': dict(content_encoder='CROWN', user_encoder='CROWN'),      # LIME over CROWN
          'naml_att': dict(news_encoder='NAML', user_encoder='ATT')}                     # a baseline: no LIME


def dev_split(name, seed=71, n_imp=40, one_class=False):
    """A synthetic dev split of ``n_imp`` impressions with 2 .. 30 candidates over 60 news and the tiny model MODELS[name] ->
    (corpus, model on the device, indices, labels).  Several positives an impression; impression 3 has a label-less truth line.
    ``one_class``: also impression 5 with a single row and impression 7 without a positive -- the impressions ``evaluate.scoring``
    (and with it the device dev pass) raises for."""
    import torch
    from lime_cikm25_amd import Model, make_config, synth
    cfg = make_config(**{**_TINY, **MODELS[name]})
    corpus = synth.synth_corpus(cfg, n_news=N_NEWS, n_train=1, n_dev=n_imp, seed=seed)
    rng = np.random.default_rng(seed)
    beh, indices, labels = [], [], []
    for i, b in enumerate(corpus.dev_behaviors):
        n = int(rng.integers(2, 31))
        if one_class and i == 5:
            n = 1
        for cand in rng.permutation(np.arange(1, N_NEWS))[:n]:
            fresh = float(np.float32(np.exp(rng.uniform(np.log(60.0), np.log(3 * 86400.0)))))
            beh.append([b[0], b[1], b[2], int(cand), i, fresh, fresh + float(rng.uniform(-8.0, 8.0)), b[7], b[8]])
            indices.append(i)
        y = (rng.random(n) < 0.3).astype(int)
        if n > 1:
            a, c = rng.choice(n, 2, replace=False)
            y[a], y[c] = 1, 0
        if one_class and i == 7:
            y[:] = 0
        labels.append([] if i == 3 else y.tolist())
    corpus.dev_behaviors = beh
    torch.manual_seed(0)
    model = Model(cfg)
    model.initialize()
    synth.fill_state_dict(model, seed=43)
    return corpus, model.cuda().eval(), indices, labels


def toy(content, user, batch_size=16, **kw):
    """The toy corpus of tests/golden/formats.json with a model on the device -> (cfg, corpus, model)."""
    import torch
    from lime_cikm25_amd import Model, formats, make_config
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
    return cfg, corpus, model.cuda()
