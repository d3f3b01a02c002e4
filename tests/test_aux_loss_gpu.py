"""The category-prediction loss of the bare CROWN baselines on the MI355X (``config.alpha``; reference newsEncoders.py:358-364,
trainer.py:137-139) against the reference goldens of tests/aux_cases.py (tests/golden/grad_aux_*.npz, tools/make_aux_goldens.py: the
reference trained with ``nll + model.news_encoder.auxiliary_loss.mean()``).  The bar is the project's parity bound TOL = 1e-3, the
gradients by ``compare_grads``; the observed values are printed.  The kernel itself: tests/test_linear_xent_gpu.py."""
import json
import math

import pytest
import torch

import aux_cases
import plain_cases
from helpers import load_golden, rel_err
from test_naml_gpu import compare_grads, unique_named_parameters
from lime_cikm25_amd import Model, synth
from lime_cikm25_amd.training import TrainStep, negative_log_softmax

pytestmark = pytest.mark.gpu
TOL = 1e-3


def gpu_model(cfg, seed=aux_cases.WEIGHT_SEED):
    m = Model(cfg)
    m.initialize()
    synth.fill_state_dict(m, seed)
    return m.cuda()


def train_forward(model, batch):
    model.eval()
    model.training = True                       # the [B, K] shape on the differentiable path, children in eval mode (no dropout)
    return model(*[v.cuda() for v in batch.values()])


@pytest.mark.parametrize('name', list(aux_cases.CASES))
def test_loss_attribute_and_gradients_match_the_reference(name):
    g = load_golden('grad_' + name)
    cfg, batch, c = aux_cases.build_case(name)
    bare = name in aux_cases.BARE_CASES
    model = gpu_model(cfg)
    assert model.news_encoder.auxiliary_loss is None
    logits = train_forward(model, batch)
    assert logits.requires_grad
    e = rel_err(logits.detach().cpu().numpy(), g['logits'])
    loss = negative_log_softmax(logits)
    nll = loss.detach().clone()
    aux = model.news_encoder.auxiliary_loss
    if bare:
        assert isinstance(aux, torch.Tensor) and aux.dim() == 0 and aux.requires_grad
        if model.news_encoder.auxiliary_loss is not None:               # the reference loop's lines, as written (trainer.py:137-139)
            loss += model.news_encoder.auxiliary_loss.mean()
        print('%s: logits %.2e, nll %.6f (reference %.6f), auxiliary loss %.6f (reference %.6f; the candidate rows would give %.6f)' % (
            name, e, float(nll), float(g['nll']), float(aux.detach()), float(g['aux']), float(g['aux_candidates'])))
        assert abs(float(aux.detach()) - float(g['aux'])) < TOL * float(g['aux'])
        assert abs(float(aux.detach()) - float(g['aux_candidates'])) > 50 * TOL * float(g['aux'])       # not the candidates' value
    else:
        assert aux is None and bool(g['aux_none'])
    assert e < TOL
    assert abs(float(nll) - float(g['nll'])) < TOL * max(1.0, abs(float(g['nll'])))
    assert abs(float(loss.detach()) - float(g['loss'])) < TOL * max(1.0, abs(float(g['loss'])))
    loss.backward()
    named = dict(unique_named_parameters(model))
    with_grad = json.loads(str(g['with_grad']))
    for k in json.loads(str(g['without_grad'])):
        assert named[k].grad is None, '%s: the reference leaves this gradient at None' % k
    assert all((k in with_grad) == bare for k in aux_cases.FC)
    if not bare:
        assert all(p.grad is None for k, p in named.items() if 'category_predictor.' in k)
    worst = compare_grads(g, named)
    print('%s: loss %.6f (reference %.6f), worst gradient %s rel err %.2e' % (name, float(loss.detach()), float(g['loss']), *worst))
    # the bucket holds category_predictor.fc exactly where the reference gives it a gradient
    names = TrainStep.bucket_names(model)
    assert names == with_grad and all((k in names) == bare for k in aux_cases.FC)


@pytest.mark.parametrize('name', list(aux_cases.CASES))
def test_no_stale_term_survives_a_forward_off_the_differentiable_path(name):
    cfg, batch, c = aux_cases.build_case(name)
    bare = name in aux_cases.BARE_CASES
    model = gpu_model(cfg)
    b = [v.cuda() for v in batch.values()]
    train_forward(model, batch)
    first = model.news_encoder.auxiliary_loss
    assert (first is not None) == bare
    model.eval()
    with torch.no_grad():                       # the eval forward (the reference computes the value here too; nothing reads it)
        model(*[v.cuda() for v in synth.make_batch(cfg, c['B'], 1, seed=c['seed'], eval_shape=True).values()])
    assert model.news_encoder.auxiliary_loss is None
    train_forward(model, batch)
    second = model.news_encoder.auxiliary_loss
    assert (second is not None) == bare
    if bare:
        assert second is not first and torch.equal(second.detach(), first.detach())
    model.eval()
    model.training = True
    with torch.no_grad():                       # the [B, K] shape on the scoring kernels
        model(*b)
    assert model.news_encoder.auxiliary_loss is None
    if bare:
        train_forward(model, batch)
        assert model.news_encoder.auxiliary_loss is not None
        d = {k: v for k, v in zip(batch.keys(), b)}
        model.eval()
        model.score_impressions(d['user_category'], d['user_subCategory'], d['user_title_text'], d['user_title_mask'], d['user_content_text'],
                                d['user_freshness'], d['user_user_topic_lifetime'], d['user_history_mask'], d['news_category'],
                                d['news_subCategory'], d['news_title_text'], d['news_title_mask'], d['news_content_text'], d['news_freshness'],
                                d['news_user_topic_lifetime'], d['remaining_lifetime'])
        assert model.news_encoder.auxiliary_loss is None


@pytest.mark.parametrize('name', list(aux_cases.CASES))
def test_training_step_is_bitwise_reproducible_and_adds_the_term(name):
    cfg, batch, c = aux_cases.build_case(name)
    g = load_golden('grad_' + name)
    bare = name in aux_cases.BARE_CASES
    b = [v.cuda() for v in batch.values()]

    def train(steps=2):
        torch.manual_seed(0)
        model = gpu_model(cfg).train()          # config.dropout_rate 0.2 and the layer's own p = 0.2: counter-based masks
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        step = TrainStep(model, lr=1e-4, gradient_clip_norm=4.0)
        assert step.names == json.loads(str(g['with_grad']))
        losses = [float(step.step(*b)) for _ in range(steps)]
        return losses, before, {k: v.detach().clone() for k, v in model.state_dict().items()}, step.names

    l1, s0, s1, names = train()
    l2, _, s2, _ = train()
    assert all(math.isfinite(x) for x in l1) and l1 == l2
    assert all(torch.equal(s1[k], s2[k]) for k in s1)
    moved = [k for k in aux_cases.FC if k in s0 and not torch.equal(s0[k], s1[k])]
    assert moved == (list(aux_cases.FC) if bare else [])
    assert all(torch.equal(s0[k], s1[k]) for k in s0 if k not in names and not k.startswith('user_encoder.news_encoder.'))


def test_the_returned_loss_is_the_sum():
    """``TrainStep.step`` returns nll + the auxiliary loss, as the reference's printed loss is; children in eval mode (the layer's own
    p = 0.2 dropout off), so the first step's value is the golden's."""
    name = 'aux_crown_crown'
    cfg, batch, c = aux_cases.build_case(name)
    g = load_golden('grad_' + name)
    model = gpu_model(cfg)
    model.eval()
    model.training = True
    step = TrainStep(model, lr=1e-4, gradient_clip_norm=4.0)
    loss = float(step.step(*[v.cuda() for v in batch.values()]))
    print('%s: step loss %.6f, reference nll + aux %.6f (nll alone %.6f)' % (name, loss, float(g['loss']), float(g['nll'])))
    assert abs(loss - float(g['loss'])) < TOL * float(g['loss'])
    assert abs(loss - float(g['nll'])) > 0.5 * float(g['aux'])


def test_alpha_zero_is_the_model_without_the_option():
    """plain_crown_crown's batch with alpha = 0 and alpha = 0.0 spelled out: no attribute, the bucket of the golden, and the same bits
    as the default configuration after two steps."""
    g = load_golden('grad_plain_crown_crown')
    out = []
    for alpha in (None, 0, 0.0):
        cfg, batch, c = plain_cases.build_case('plain_crown_crown')
        if alpha is not None:
            cfg.alpha = alpha
        torch.manual_seed(0)
        model = gpu_model(cfg, seed=plain_cases.WEIGHT_SEED)
        logits = train_forward(model, batch)
        assert model.news_encoder.auxiliary_loss is None
        assert rel_err(logits.detach().cpu().numpy(), g['logits']) < TOL
        step = TrainStep(model, lr=1e-4, gradient_clip_norm=4.0)
        assert step.names == json.loads(str(g['with_grad'])) and not set(aux_cases.FC) & set(step.names)
        b = [v.cuda() for v in batch.values()]
        losses = [float(step.step(*b)) for _ in range(2)]
        assert model.news_encoder.auxiliary_loss is None
        out.append((losses, {k: v.detach().clone() for k, v in model.state_dict().items()}))
    for losses, sd in out[1:]:
        assert losses == out[0][0] and all(torch.equal(sd[k], out[0][1][k]) for k in sd)
