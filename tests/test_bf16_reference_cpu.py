"""The fp64 statements of tests/bf16_cases.py against fp32 evaluations of the SAME statements (torch on the CPU, the k axis of every
product in natural and in a permuted order), on every case the GPU module runs (the persistent-loop cases sized for 256 CUs): a
correct fp32-accumulating implementation stays inside ``assert_bf16_matches`` on these inputs, and the largest pre-rounding deviation
of the multi-rounding statements is where bf16_cases.ALLOWANCE_ULPS comes from.  Also pins the criterion itself.  CPU only; run
with -s for the per-kernel figures quoted in the bf16_cases docstring."""
import functools
import math

import pytest
import torch

import bf16_cases as C

ORDERS = (None, 11)             # natural k order, one permuted order
N_CU = C.NOMINAL_CUS


class Tally:
    def __init__(self, name):
        self.name, self.share, self.worst, self.dev = name, [], 0.0, 0.0

    def add(self, eval32, want64, single_rounding, what):
        share, worst = C.assert_bf16_matches(eval32.to(torch.bfloat16), want64, single_rounding, what)
        self.share.append(share)
        self.worst = max(self.worst, worst)
        self.dev = max(self.dev, float(((eval32.double() - want64).abs() / C.ulp_scale(want64)).max()))    # BEFORE the final rounding

    def report(self):
        print('%s: fp32 CPU evaluations differ from bf16(fp64) in %.4f-%.4f %% of the elements, worst %.3f ulp; largest pre-rounding '
              'deviation %.3f ulp' % (self.name, 100 * min(self.share), 100 * max(self.share), self.worst, self.dev))
        return self


@functools.lru_cache(maxsize=None)
def measure_inproj():
    t = Tally('in_proj')
    for M, K, N, S in C.INPROJ:
        M = C.inproj_m(M, N_CU)
        d = C.inproj_inputs(M, K, N, S)
        rows = d['table'][d['ids'].long()]
        for period, scattered in (((S, True),) if M > 1000 else ((1, False), (1, True), (S, False), (S, True))):
            want, bound = C.inproj_want(M, K, N, S, period, scattered)
            out_row = d['c_ids'].long() if scattered else torch.arange(M)
            for perm in ORDERS:
                got = C.inproj64(rows, d['w'], d['adds'][period], out_row, dt=torch.float32, perm=perm)
                t.add(got, want, bound, 'in_proj %s period %d scattered %d order %s' % ((M, K, N), period, scattered, perm))
    return t.report()


@functools.lru_cache(maxsize=None)
def measure_linear():
    t = Tally('linear')
    for M in C.LINEAR_M:
        d = C.linear_inputs(M)
        a = d['table'][d['ids'].long()]
        res = d['res'][d['c_ids'].long() % d['S']]
        want, bound = C.linear64(a, d['w'], res=res), C.linear_acc_bound(a, d['w'], res=res)
        for perm in ORDERS:
            t.add(C.linear64(a, d['w'], res=res, dt=torch.float32, perm=perm), want, bound, 'linear M=%d order %s' % (M, perm))
    return t.report()


@functools.lru_cache(maxsize=None)
def measure_attn():
    t = Tally('attention')
    shapes = sorted({c[:4] for c in C.ATTN_DENSE} | set(C.attn_loop_cases(N_CU)) | {(S, 5, 10, hd) for S in (32, 64, 128) for hd in (30, 32)})
    for S, n_seq, h, hd in shapes:
        qkv, scale, want = C.attn_inputs(S, n_seq, h, hd)
        W = h * 32
        for perm in ORDERS:
            got = C.attn64(qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:], n_seq, S, h, hd, scale, dt=torch.float32, perm=perm)
            t.add(got, want, None, 'attention %s order %s' % ((S, n_seq, h, hd), perm))
    return t.report()


@functools.lru_cache(maxsize=None)
def measure_ffn():
    t = Tally('ffn')
    cases = [(E, F, M) for E in C.FFN_E for F in C.FFN_F for M in C.FFN_M] + [C.FFN_BIG + (C.big_m(N_CU),), (300, 512, C.M_DEV_ROWS)]
    for E, F, M in cases:
        x, w, want = C.ffn_inputs(E, F, M)
        for perm in ORDERS:
            got = C.ffn64(x, w['w1'], w['b1'], w['w2'], w['b2'], w['g'], w['beta'], w['eps'], E, dt=torch.float32, perm=perm)
            t.add(got, want, None, 'ffn %s order %s' % ((E, F, M), perm))
    return t.report()


@functools.lru_cache(maxsize=None)
def measure_block():
    t = Tally('block')
    cases = [(E, kind, per, C.BLOCK_M) for E in (292, 296, 300) for kind in (2, 3) for per in (1, C.BLOCK_S)]
    cases += [C.BLOCK_BIG + (C.big_m(N_CU),), (300, 2, C.BLOCK_S, C.M_DEV_ROWS)]
    for E, kind, per, M in cases:
        d = C.block_inputs(E, kind, per, M)
        for perm in ORDERS:
            t.add(C.block_want(d, E, dt=torch.float32, perm=perm), d['want'], None, 'block %s order %s' % ((E, kind, per, M), perm))
    return t.report()


@pytest.mark.parametrize('measure', [measure_inproj, measure_linear], ids=['in_proj', 'linear'])
def test_single_rounding_statements_hold_for_an_fp32_evaluation(measure):
    """0.5 ulp + the derived accumulation bound, and the 1 % cap, in both k orders (the assertions are in Tally.add)."""
    t = measure()
    assert t.worst <= 0.5 + 1e-2                  # the accumulation term is a sliver: fp32 against bf16


@pytest.mark.parametrize('measure', [measure_attn, measure_ffn, measure_block], ids=['attention', 'ffn', 'block'])
def test_multi_rounding_statements_hold_for_an_fp32_evaluation(measure):
    t = measure()
    assert 2 * t.dev <= C.ALLOWANCE_ULPS


def test_allowance_is_twice_the_largest_measured_deviation():
    """bf16_cases.ALLOWANCE_ULPS covers 2 x the largest pre-rounding deviation over every multi-rounding case (it was set to that figure
    rounded up to 0.1 ulp; the deviation is a rare discrete event -- one intermediate rounding the other way -- so another BLAS may find
    a smaller one, never a reason to raise the constant without looking)."""
    dev = max(m().dev for m in (measure_attn, measure_ffn, measure_block))
    print('largest pre-rounding deviation %.3f ulp -> allowance %.3f, carried as %.1f' % (dev, 2 * dev, C.ALLOWANCE_ULPS))
    assert 2 * dev <= C.ALLOWANCE_ULPS


# ---------------------------------------------------------------------------------------------------
# the criterion itself
# ---------------------------------------------------------------------------------------------------
def _ulp_step(t_bf16, steps):
    """bf16 tensor moved by ``steps`` representable values (away from zero for steps > 0)."""
    return (t_bf16.view(torch.int16) + steps).view(torch.bfloat16)


def test_the_criterion_passes_the_rounded_statement_and_fails_small_damage():
    _, _, want = C.ffn_inputs(300, 128, 129)
    exact = C.round_bf16(want).to(torch.bfloat16)
    assert torch.equal(exact.double(), C.round_bf16(want))                     # the fp64 rounding lands on bf16 values
    share, worst = C.assert_bf16_matches(exact, want, None, 'bf16(want64)')
    assert share == 0.0 and worst <= 0.5
    zero_bound = torch.zeros_like(want)
    C.assert_bf16_matches(exact, want, zero_bound, 'bf16(want64), single rounding')
    flat = want.abs().reshape(-1)
    big = int(flat.argmax())                                                   # an element above its row's mean: the floor does not help it
    # ONE element moved by 2 ulps: over the hard bound of a single-rounding result; moved past 0.5 + ALLOWANCE_ULPS (+ 0.5 for where
    # inside its rounding interval the statement lies): over that of a multi-rounding one
    for steps, single in ((2, zero_bound), (math.ceil(C.ALLOWANCE_ULPS + 1.0) + 1, None)):
        bad = exact.clone()
        bad.view(-1)[big] = _ulp_step(bad.view(-1)[big:big + 1], steps)[0]
        with pytest.raises(AssertionError, match='over its bound'):
            C.assert_bf16_matches(bad, want, single, 'one element moved by %d ulps' % steps)
    # 2 % of the elements moved by ONE ulp: inside the hard bound of a multi-rounding result, over the share cap
    idx = torch.randperm(want.numel(), generator=C.gen(5))[:want.numel() // 50 + 1]
    bad = exact.clone()
    bad.view(-1)[idx] = _ulp_step(bad.view(-1)[idx], 1)
    with pytest.raises(AssertionError, match='at most 1 %'):
        C.assert_bf16_matches(bad, want, None, '2 % of the elements moved by 1 ulp')
    # one lane of 64 moved by one ulp (the damage the cap is sized for)
    bad = exact.clone()
    bad[:, 5::64] = _ulp_step(bad[:, 5::64], 1)
    with pytest.raises(AssertionError, match='at most 1 %'):
        C.assert_bf16_matches(bad, want, None, 'every 64th column moved by 1 ulp')
    bad = exact.clone()
    bad[0, 0] = float('nan')
    with pytest.raises(AssertionError, match='non-finite'):
        C.assert_bf16_matches(bad, want, None, 'a NaN')


def test_fp64_rounding_is_round_to_nearest_even():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, -1.0 - 2.0 ** -8 - 2.0 ** -40, 0.0, 3e-39,
                      1.0 + 2.0 ** -8 - 2.0 ** -30], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0 - 2.0 ** -7, 0.0, float(torch.tensor(3e-39).bfloat16()), 1.0],
                        dtype=torch.float64)
    assert torch.equal(C.round_bf16(x), want)
    # where a conversion through fp32 rounds twice (down to the tie, then to even = down to 1.0): the direct rounding goes up
    y = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30], dtype=torch.float64)
    assert float(C.round_bf16(y)) == 1.0 + 2.0 ** -7
    f = C.rnd(1000, seed=1, scale=3.0)
    assert torch.equal(C.round_bf16(f.double()), f.bfloat16().double())


def test_ulp_scale_uses_the_row_mean_as_floor():
    want = torch.tensor([[1.0, 1e-6, 3.0, 0.0]], dtype=torch.float64)         # row mean 1.0
    assert C.ulp_scale(want).tolist() == [[2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -7]]
