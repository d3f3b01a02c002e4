"""lime_nll_softmax_f32 on confident rows of LARGE logits against float64.

The click logits are dot products of unnormalised 400- to 900-wide vectors and reach 100 (tests/aux_cases.py's aux_crown_mhsa: rows
like [102.08, 9.61, 97.98]).  The gradient of such a row is 1 - softmax[0] and its mirror on the other candidates, a few 1e-3 to 1e-2.
Formed as exp(x - (max + log s)) - 1 it carries the rounding of a number near 100 (half an ulp: 4e-6), i.e. 1e-4 to 1e-3 of itself, and
every parameter gradient of the step inherits that; with every difference taken against the row's maximum -- exp(x - max) / s, and
log s - (x[0] - max) for the loss -- what is left is the rounding of 1 / s (6e-8 absolute) and of exp's argument (6e-8 |x - max|).

The bound: rows are built with 1 - softmax[0] >= 1e-2 and x - max >= -16 where it matters, so a row's gradient is good to
6e-8 / 1e-2 + 6e-8 * 16 = 7e-6 of its largest entry; the test asks the project's kernel bound KTOL = 2e-5, per row."""
import pytest
import torch

pytestmark = pytest.mark.gpu
KTOL = 2e-5


@pytest.fixture(scope='module')
def ops():
    from lime_cikm25_amd import ops as o
    return o


@pytest.mark.parametrize('level', [0.0, 100.0, -100.0, 1000.0])
def test_confident_rows_of_large_logits(ops, level):
    B, K = 37, 5
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, K, generator=g) * 2.0
    x[:, 0] = x[:, 1:].max(dim=1).values + 1.0 + 3.0 * torch.rand(B, generator=g)      # 1 - softmax[0] between 1.7e-2 and 0.6
    x = (x + level).float()
    xd = x.double().requires_grad_()
    loss = (-torch.log_softmax(xd, dim=1).select(dim=1, index=0)).mean()
    loss.backward()
    want = xd.grad
    assert float((-want[:, 0] * B).min()) >= 1e-2
    got_loss, got = ops.nll_softmax(x.cuda())
    torch.cuda.synchronize()
    got = got.cpu().double()
    rows = (got - want).abs().max(dim=1).values / want.abs().max(dim=1).values
    e_loss = abs(float(got_loss) - float(loss.detach())) / float(loss.detach())
    print('level %g: worst row of dlogits %.2e of its largest entry, loss %.2e' % (level, float(rows.max()), e_loss))
    assert float(rows.max()) < KTOL and e_loss < KTOL
    # a row of softmax - onehot sums to zero: K - 1 roundings in s, one in 1 / s, one per product, one per subtraction and scaling
    # -- under (K + 3) 6e-8 = 4.8e-7 of the row's unit mass; 1e-6 asked
    assert float(got.sum(dim=1).abs().max()) * B < 1e-6
