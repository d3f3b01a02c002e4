"""lime_cached_occurrence_f32 (csrc/cached_occurrence_f32.hip, ops.cached_occurrence) and the per-news content cache of all three
fusion methods on the MI355X: the kernel against torch on the same fp32 operands, LIME.encode_cached against LIME.encode_flat, cached
scoring of 'add' / 'gated' models against the uncached forward and the oracle, and the agreement of the two cached passes."""
import json
import os

import numpy as np
import pytest
import torch

import golden_cases
from helpers import GOLDEN_DIR, load_golden, rel_err
from lime_cikm25_amd import Model, formats, make_config, newsEncoders, ops, synth
from lime_cikm25_amd import util as U
from lime_cikm25_amd.device_data import DeviceBehaviors, DeviceCorpus
from oracle import lime_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-3                      # the project's bound against the oracle (tests/test_model_gpu.py)
KTOL = 2e-5                     # two layouts of one function: the same sums in another order (tests/test_model_gpu.py)
ATOL = 1e-12                    # device metrics against the host's (tests/test_rank_metrics_gpu.py)
U24 = 2.0 ** -24                # unit roundoff of fp32

CUTS = np.array(golden_cases._CUTS, dtype=np.uint32)           # bit patterns of the nine cut points of num_buckets = 10


def edge_values():
    """Both neighbours of every cut point and the cut point itself, 0, NaN and a few ordinary values."""
    return np.concatenate([(CUTS - 1).view(np.float32), CUTS.view(np.float32), (CUTS + 1).view(np.float32),
                           np.array([0.0, np.nan, 0.5, 1.0, 2854.0, 86400.0, 3e38], dtype=np.float32)])


def operands(D, R, n=37, nb=10, seed=0, strided=True):
    """Random A, P [n, D] and T, Q [nb^2, D] (column views of wider tensors when ``strided``), ids that include 0 and n - 1,
    freshness / lifetime over the edge values in two different orders."""
    g = torch.Generator().manual_seed(seed)
    wide = lambda rows, off: torch.randn(rows, 2 * D + 8, generator=g).cuda()[:, off:off + D]
    if strided:
        cache = torch.randn(n, 2 * D, generator=g).cuda()
        A, P = cache[:, :D], cache[:, D:]                        # the layout of the gated cache
        T, Q = wide(nb * nb, 4), wide(nb * nb, D + 8)
    else:
        A, P, T, Q = (torch.randn(r, D, generator=g).cuda() for r in (n, n, nb * nb, nb * nb))
    idx = torch.randint(0, n, (R,), generator=g, dtype=torch.int32)
    idx[0], idx[-1] = 0, n - 1
    v = edge_values()
    fr = torch.from_numpy(v[np.arange(R) % v.size])
    lt = torch.from_numpy(v[(np.arange(R) * 7 + 3) % v.size])
    return A, P, T, Q, idx.cuda(), fr.cuda(), lt.cuda()


def pairs(fr, lt, nb=10, cuts=None):
    return (ops.bucketize(fr, cuts).long() * nb + ops.bucketize(lt, cuts).long())


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
def test_bucket_pairs_are_bit_exact_against_the_reference_golden():
    """The freshness / lifetime values of the 'bucket_edges' golden case (both sides of every cut point) through the kernel with
    A = 0 and T[pair, :] = pair: the kernel's bucket pair is the reference's own bucketize, read from tests/golden/bucket_edges.npz."""
    cfg, batch, c = golden_cases.build_case('bucket_edges')
    g = load_golden('bucket_edges')
    T = torch.arange(100, dtype=torch.float32).view(100, 1).expand(100, 4).contiguous().cuda()
    for f, l, fb, lb in ((batch['news_freshness'], batch['news_user_topic_lifetime'], g['cand_f_bucket'], g['cand_l_bucket']),
                         (batch['user_freshness'], batch['user_user_topic_lifetime'], g['hist_f_bucket'], g['hist_l_bucket'])):
        R = f.numel()
        out = ops.cached_occurrence('add', torch.zeros(R, dtype=torch.int32).cuda(), f.reshape(-1).float().cuda(), l.reshape(-1).float().cuda(),
                                    torch.zeros(1, 4).cuda(), T)
        assert np.array_equal(out[:, 0].cpu().numpy().astype(np.int64), (fb * 10 + lb).reshape(-1))
    v = torch.from_numpy(edge_values()).cuda()                 # NaN -> bucket 0, like 0; the neighbours as the oracle buckets them
    out = ops.cached_occurrence('add', torch.zeros(v.numel(), dtype=torch.int32).cuda(), v, torch.zeros_like(v), torch.zeros(1, 4).cuda(), T)
    want = O.bucketize(torch.nan_to_num(v.cpu(), nan=0.0)) * 10
    assert torch.equal(out[:, 0].cpu().long(), want)
    assert out[28, 0].item() == 0.0 and bool(torch.isnan(v[28]))


@pytest.mark.parametrize('D', [300 + 100, 400, 500, 900])
@pytest.mark.parametrize('strided', [True, False])
@pytest.mark.parametrize('mode', ['concat', 'add'])
def test_concat_and_add_are_one_fp32_addition(D, strided, mode):
    """out[r] = A[idx[r]] + T[pair[r]]: each element is ONE fp32 addition of the same two operands torch adds -- torch.equal."""
    A, P, T, Q, idx, fr, lt = operands(D, 257, seed=D, strided=strided)
    out = ops.cached_occurrence(mode, idx, fr, lt, A, T)
    assert torch.equal(out, A[idx.long()] + T[pairs(fr, lt)])
    view = torch.full((257, D + 12), 7.0).cuda()                # a strided destination: the columns beside it stay untouched
    ops.cached_occurrence(mode, idx, fr, lt, A, T, out=view[:, 4:4 + D])
    assert torch.equal(view[:, 4:4 + D], out) and bool((view[:, :4] == 7).all()) and bool((view[:, 4 + D:] == 7).all())


@pytest.mark.parametrize('D', [300 + 100, 400, 500, 900])
@pytest.mark.parametrize('strided', [True, False])
def test_gated_against_fp64_on_the_same_operands(D, strided):
    """g = sigmoid(P[idx] + Q[pair]), out = g A[idx] + (1 - g) T[pair], against the fp64 evaluation of the same expression on the
    fp32 operands; element bound 8 * 2^-24 * (|A| + |T|).

    Derivation, u = 2^-24, from the kernel's instruction sequence  s = p + q;  e = expf(-s);  d = 1 + e;  g = 1 / d  (lime_sigmoid:
    exp, add, divide)  then  h = 1 - g;  m = h * t;  out = fma(g, a, m):
      * s carries one rounding, |ds| <= u |s|; expf is accurate to 1 ulp = 2 u, so e has relative error <= (2 + |s|) u; the add
        and the correctly rounded divide add u each.  With dg / g = -(1 - g) de / e the absolute error of g is
        |dg| <= [g (1 - g) (2 + |s|) + 2 g] u, and g (1 - g) |s| <= 0.23, g (1 - g) <= 1 / 4, g < 1:  |dg| <= 2.73 u;
      * the exact expression has d out / d g = a - t, so dg costs at most 2.73 u (|a| + |t|);
      * the four roundings behind g -- the subtraction 1 - g and the product h t (each <= u (1 - g) |t|) and the one rounding of the
        fma (<= u |out| <= u (|a| + |t|)), plus h inheriting dg, counted above -- add at most 3 u (|a| + |t|).
    Total <= 5.73 u (|a| + |t|) < 8 u (|a| + |t|) for every s where expf neither overflows nor flushes (|s| < 87; here |s| < 12)."""
    A, P, T, Q, idx, fr, lt = operands(D, 513, seed=100 + D, strided=strided)
    out = ops.cached_occurrence('gated', idx, fr, lt, A, T, P, Q)
    i, p = idx.long(), pairs(fr, lt)
    a, t, s = A[i].double(), T[p].double(), P[i].double() + Q[p].double()
    g = 1.0 / (1.0 + torch.exp(-s))
    want = g * a + (1.0 - g) * t
    bound = 8 * U24 * (a.abs() + t.abs())
    frac = ((out.double() - want).abs() / bound).max().item()
    print('gated D=%d strided=%s: max |err| / bound = %.3f (|s| max %.1f)' % (D, strided, frac, s.abs().max().item()))
    assert frac <= 1.0


@pytest.mark.parametrize('mode', ['add', 'gated'])
def test_bitwise_deterministic_and_independent_of_the_row_count(mode):
    """Two runs give equal bits; a row computed alone, inside R = 7 and inside R = 8192 * 51 has the same bits."""
    D, R = 900, 8192 * 51
    A, P, T, Q, idx, fr, lt = operands(D, R, n=301, seed=5)
    run = lambda sl: ops.cached_occurrence(mode, idx[sl].contiguous(), fr[sl].contiguous(), lt[sl].contiguous(), A, T, P, Q)
    big = run(slice(0, R))
    assert torch.equal(big, run(slice(0, R)))
    for r0 in (0, 12345, R - 7):
        seven = run(slice(r0, r0 + 7))
        assert torch.equal(seven, big[r0:r0 + 7])
        for k in (0, 3, 6):
            assert torch.equal(run(slice(r0 + k, r0 + k + 1)), big[r0 + k:r0 + k + 1])


def test_another_bucket_count_takes_the_cut_table():
    nb = 7
    cuts = newsEncoders.bucket_cut_points(nb).cuda()
    A, P, T, Q, idx, fr, lt = operands(400, 129, nb=nb, seed=9)
    bits = cuts.cpu().numpy().view(np.uint32)
    v = torch.from_numpy(np.concatenate([(bits - 1).view(np.float32), bits.view(np.float32), (bits + 1).view(np.float32)])).cuda()
    fr[:v.numel()] = v
    out = ops.cached_occurrence('add', idx, fr, lt, A, T, cuts=cuts)
    assert torch.equal(out, A[idx.long()] + T[pairs(fr, lt, nb, cuts)])
    with pytest.raises(Exception, match='num_buckets'):          # the default 100-row table against a 6-cut table: refused before the launch
        ops.cached_occurrence('add', idx, fr, lt, A, torch.zeros(100, 400).cuda(), cuts=cuts)


# ---- LIME.occurrence_tables / encode_cached against encode_flat ---------------------------------------------------------------
@pytest.mark.parametrize('content', ['CROWN', 'CNN', 'NAML', 'MHSA'])
@pytest.mark.parametrize('fusion', ['concat', 'add', 'gated'])
def test_encode_cached_agrees_with_encode_flat(content, fusion):
    """Every news of a synthetic batch once through build_content_cache + encode_cached (the kernel) and once through encode_flat.
    The GEMM kernel that serves a table of 100 rows may order its k sums differently from the one serving M rows: KTOL."""
    cfg = make_config(content_encoder=content, fusion_method=fusion, max_history_num=6, max_title_length=16, max_abstract_length=32,
                      batch_size=8, vocabulary_size=3000)
    torch.manual_seed(3)
    model = Model(cfg)
    model.initialize()
    synth.fill_state_dict(model, 71)
    model = model.cuda().eval()
    ne = model.news_encoder
    batch = synth.make_batch(cfg, 6, 5, seed=72)
    b = {k: v.cuda() for k, v in batch.items()}
    tt, tm, ct, cat, sub = newsEncoders._flat_inputs(b['news_title_text'], b['news_title_mask'], b['news_content_text'], b['news_category'],
                                                     b['news_subCategory'])
    M = tt.shape[0]
    v = torch.from_numpy(edge_values()[:M].copy()).cuda()
    fr = b['news_freshness'].float().reshape(-1).clone()
    lt = b['news_user_topic_lifetime'].float().expand_as(b['news_freshness']).reshape(-1).contiguous()
    fr[:v.numel()] = torch.nan_to_num(v, nan=0.0)               # both sides of every cut point on the way
    with torch.no_grad():
        want = ne.encode_flat(tt, tm, ct, cat, sub, fr, lt)
        cache = ne.build_content_cache(tt, tm, ct, cat, sub, rows_per_pass=16)       # two passes over the 30 news
        T, Q = ne.occurrence_tables()
        got = ne.encode_cached(cache, torch.arange(M).cuda(), fr, lt, fused=True)
    c = ne.base_news_encoder.news_embedding_dim
    assert cache.shape == (M, {'concat': cfg.lime_output_dim, 'add': c, 'gated': 2 * c}[fusion])
    assert T.shape == (100, ne.output_dim) and (Q is None) == (fusion != 'gated')
    e = rel_err(got.cpu().numpy(), want.cpu().numpy())
    print('%s %s: encode_cached vs encode_flat %.2e' % (content, fusion, e))
    assert got.shape == want.shape == (M, ne.output_dim) and e < KTOL


# ---- cached scoring on the toy corpus ----------------------------------------------------------------------------------------------
def toy(content, user, fusion, batch_size=16, **kw):
    """The toy corpus of tests/golden/formats.json with a model on it, built as tests/test_model_gpu.py builds it."""
    g = json.load(open(os.path.join(GOLDEN_DIR, 'formats.json')))
    L = g['lines']
    cfg = make_config(content_encoder=content, user_encoder=user, fusion_method=fusion, max_history_num=g['max_history_num'],
                      max_title_length=g['max_title_length'], max_abstract_length=g['max_abstract_length'], vocabulary_size=len(g['word_dict']),
                      negative_sample_num=2, category_num=len(g['category_dict']) + 1, subCategory_num=len(g['subCategory_dict']) + 1,
                      user_num=len(g['user_ID_dict']), batch_size=batch_size, **kw)
    corpus = formats.build_corpus(cfg, [L['train_news'], L['dev_news'], L['test_news']],
                                  [L['train_behaviors'], L['dev_behaviors'], L['test_behaviors']], g['news_ID_dict'],
                                  g['user_ID_dict'], g['category_dict'], g['subCategory_dict'], g['word_dict'], dataset='adressa')
    torch.manual_seed(0)
    model = Model(cfg)
    model.initialize()
    torch.nn.init.normal_(model.news_encoder.base_news_encoder.word_embedding.weight, std=0.1)
    if hasattr(model.user_encoder, 'user_node_embedding'):
        torch.nn.init.normal_(model.user_encoder.user_node_embedding, std=0.1)     # zeros at initialisation: make the node term count
    return cfg, corpus, model.cuda(), formats.truth_labels(L['dev_behaviors'])


@pytest.mark.parametrize('content,user', [('CROWN', 'CROWN'), ('NAML', 'ATT')])
@pytest.mark.parametrize('fusion', ['add', 'gated'])
def test_cached_scoring_agrees_with_the_uncached_forward_and_the_oracle(content, user, fusion):
    """Model.score_behaviors over all dev rows against Model.forward on the assembled rows in eval mode (KTOL), and against the oracle
    (TOL) where the oracle covers the pairing (LIME-CROWN-CROWN; it has no NAML / ATT).  Two candidates get an expired lifetime far
    past saturation: their score is an exact zero whose sign is the sign of the dot product, in both passes.  Rank files are not
    compared here: a near-tie may flip between two summation orders on so few rows."""
    cfg, corpus, model, _ = toy(content, user, fusion)
    dev = DeviceBehaviors.from_devtest(DeviceCorpus(corpus), corpus, 'dev')
    dev.cand_freshness[:2] = 1e9                                 # remaining lifetime -1e9: sigmoid(alpha r) is exactly 0
    dev.cand_lifetime[:2] = 0.0
    rows = list(range(dev.num))
    model.eval()
    with torch.no_grad():
        batch = dev.assemble(rows)
        remaining = batch[24] - batch[23]
        want = model(*batch, remaining).squeeze(1).float().cpu().numpy()
        cache = model.build_news_cache(dev.corpus)
        got = model.score_behaviors(dev, rows, cache).float().cpu().numpy()
    c = model.news_encoder.base_news_encoder.news_embedding_dim
    assert cache.shape[1] == (2 * c if fusion == 'gated' else c)
    e = rel_err(got, want)
    print('%s-%s %s: cached vs uncached %.2e over %d rows' % (content, user, fusion, e, dev.num))
    assert got.shape == want.shape == (dev.num,) and e < KTOL
    z = want == 0
    assert z[:2].all() and np.all(got[z] == 0) and np.array_equal(np.signbit(got[z]), np.signbit(want[z]))
    if (content, user) == ('CROWN', 'CROWN'):
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        inputs = [t.cpu() for t in batch] + [remaining.cpu()]
        ref = O.model_forward(sd, cfg, inputs, eval_shape=True).reshape(-1).numpy()
        e_o = rel_err(got, ref)
        print('%s-%s %s: cached vs oracle %.2e' % (content, user, fusion, e_o))
        assert e_o < TOL
        assert np.all(got[ref == 0] == 0) and np.array_equal(np.signbit(got[ref == 0]), np.signbit(ref[ref == 0]))


@pytest.mark.parametrize('fusion', ['concat', 'add', 'gated'])
def test_host_and_device_cached_passes_agree(fusion, tmp_path):
    """util.compute_scores_cached and util.evaluate_cached_on_device with rows_per_pass == rows_per_forward run the same forwards: the
    same scores, rank file and metrics, for every fusion method."""
    cfg, corpus, model, labels = toy('CROWN', 'CROWN', fusion, batch_size=6)
    dev = DeviceBehaviors.from_devtest(DeviceCorpus(corpus), corpus, 'dev')
    truth = formats.write_truth_file(str(tmp_path / 'truth.txt'), labels)
    per = cfg.batch_size
    host = U.compute_scores_cached(model, dev, corpus.dev_indices, str(tmp_path / 'host.txt'), truth, rows_per_forward=per)
    same, scores = U.evaluate_cached_on_device(model, dev, corpus.dev_indices, labels, result_file=str(tmp_path / 'same.txt'),
                                               rows_per_forward=per, rows_per_pass=per, return_scores=True)
    assert (tmp_path / 'same.txt').read_text() == (tmp_path / 'host.txt').read_text()
    assert np.allclose(same, host, rtol=0, atol=ATOL)
    model.eval()
    cache = model.build_news_cache(dev.corpus)
    chunks = [model.score_behaviors(dev, list(range(r0, min(dev.num, r0 + per))), cache, n_src=min(per, dev.num - r0)) for r0 in range(0, dev.num, per)]
    assert torch.equal(torch.cat(chunks).float(), scores)


def test_trainer_takes_the_cached_device_pass_for_a_gated_model(tmp_path):
    from lime_cikm25_amd.trainer import Trainer
    d = str(tmp_path)
    cfg, corpus, model, labels = toy('CROWN', 'CROWN', 'gated', batch_size=8, epoch=1, lr=1e-3, dataset='adressa', model_dir=d + '/models',
                                     best_model_dir=d + '/best', dev_res_dir=d + '/dev/res', result_dir=d + '/results')
    plain = Trainer(model, cfg, corpus, run_index=1)
    fused = Trainer(model, cfg, corpus, run_index=2, device_eval=True)
    assert plain.cached_eval and not plain.device_eval and fused.cached_eval and fused.device_eval
    a, b = plain.evaluate(1), fused.evaluate(1)
    name = model.model_name
    assert open(os.path.join(fused.dev_res_dir, '%s-1.txt' % name)).read() == open(os.path.join(plain.dev_res_dir, '%s-1.txt' % name)).read()
    assert np.allclose(a, b, rtol=0, atol=ATOL)
    uncached = Trainer(model, cfg, corpus, run_index=3, cached_eval=False)
    assert not uncached.cached_eval
    c = uncached.evaluate(1)                                     # the only pass before: same metrics up to near-ties on 2e-5 scores
    print('gated trainer metrics, cached - uncached:', np.abs(np.array(a) - np.array(c)).max())


# ---- concat with the flag on -------------------------------------------------------------------------------------------------------
def test_concat_with_the_kernel_agrees_with_the_default_path(monkeypatch):
    assert ops.FUSED_OCCURRENCE is (os.environ.get('LIME_FUSED_OCCURRENCE', '0') == '1')
    cfg, corpus, model, _ = toy('CROWN', 'CROWN', 'concat')
    dev = DeviceBehaviors.from_devtest(DeviceCorpus(corpus), corpus, 'dev')
    rows = list(range(dev.num))
    model.eval()
    cache = model.build_news_cache(dev.corpus)
    monkeypatch.setattr(ops, 'FUSED_OCCURRENCE', False)
    off = model.score_behaviors(dev, rows, cache)
    assert torch.equal(off, model.score_behaviors(dev, rows, cache))
    ne = model.news_encoder
    r_off = ne.encode_cached(cache, dev.hist_index[rows], dev.user_freshness[rows], dev.user_lifetime[rows])
    assert torch.equal(r_off, ne.encode_cached(cache, dev.hist_index[rows], dev.user_freshness[rows], dev.user_lifetime[rows], fused=False))
    r_on = ne.encode_cached(cache, dev.hist_index[rows], dev.user_freshness[rows], dev.user_lifetime[rows], fused=True)
    monkeypatch.setattr(ops, 'FUSED_OCCURRENCE', True)
    on = model.score_behaviors(dev, rows, cache)
    assert torch.equal(r_on, ne.encode_cached(cache, dev.hist_index[rows], dev.user_freshness[rows], dev.user_lifetime[rows]))
    e_rep, e = rel_err(r_on.cpu().numpy(), r_off.cpu().numpy()), rel_err(on.cpu().numpy(), off.cpu().numpy())
    print('concat, kernel against the default launches: representations %.2e, scores %.2e' % (e_rep, e))
    assert e_rep < KTOL and e < KTOL


def test_concat_with_identity_project_is_left_as_it_was(monkeypatch):
    """lime_output_dim = 0: `project` is the identity, there is no table form; the cached representation is cat(content, freshness)
    whatever the flag says."""
    cfg = make_config(lime_output_dim=0, max_history_num=6, max_title_length=16, max_abstract_length=32, batch_size=8, vocabulary_size=3000)
    torch.manual_seed(3)
    model = Model(cfg)
    model.initialize()
    synth.fill_state_dict(model, 73)
    ne = model.cuda().eval().news_encoder
    b = {k: v.cuda() for k, v in synth.make_batch(cfg, 4, 3, seed=74).items()}
    tt, tm, ct, cat, sub = newsEncoders._flat_inputs(b['news_title_text'], b['news_title_mask'], b['news_content_text'], b['news_category'],
                                                     b['news_subCategory'])
    fr = b['news_freshness'].float().reshape(-1).contiguous()
    lt = b['news_user_topic_lifetime'].float().expand_as(b['news_freshness']).reshape(-1).contiguous()
    idx = torch.arange(tt.shape[0]).cuda()
    with torch.no_grad():
        cache = ne.build_content_cache(tt, tm, ct, cat, sub)
        monkeypatch.setattr(ops, 'FUSED_OCCURRENCE', False)
        off = ne.encode_cached(cache, idx, fr, lt)
        monkeypatch.setattr(ops, 'FUSED_OCCURRENCE', True)
        on = ne.encode_cached(cache, idx, fr, lt)
        want = ne.encode_flat(tt, tm, ct, cat, sub, fr, lt)
    c = ne.base_news_encoder.news_embedding_dim
    assert cache.shape[1] == c and on.shape == (tt.shape[0], 2 * c) and torch.equal(on, off)
    assert rel_err(on.cpu().numpy(), want.cpu().numpy()) < KTOL


def test_the_kernel_neither_allocates_nor_synchronises():
    """Graph safety: ops.cached_occurrence with ``out`` given records into a HIP graph (an allocation or a synchronise inside the
    capture would fail it), and the replay gives the eager bits."""
    A, P, T, Q, idx, fr, lt = operands(900, 1000, seed=11)
    out = torch.empty(1000, 900).cuda()
    eager = ops.cached_occurrence('gated', idx, fr, lt, A, T, P, Q)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ops.cached_occurrence('gated', idx, fr, lt, A, T, P, Q, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
