"""The host model of the dropout mask (tests/dropout_cases.py) pinned without a GPU: known answers for the mixer, the threshold and
wrapping rules of lime_make_dropout, the keep rate, the coverage of the case lists, and the comparison helpers failing when they should.
tests/test_dropout_kernels_gpu.py holds every mask-drawing kernel to this model."""
import math

import numpy as np
import pytest
import torch

import dropout_cases as dc
from helpers import rel_err


def test_mixer_gives_the_published_splitmix64_outputs():
    """splitmix64 seeded with 1234567: the state advances by the golden-ratio constant, the mixer is the output function."""
    x = 1234567
    got = []
    for _ in range(3):
        x = (x + dc.GOLDEN) & 0xFFFFFFFFFFFFFFFF
        got.append(int(dc.mixer(np.array([x], dtype=np.uint64))[0]))
    assert got == [6457827717110365317, 3203168211198807973, 9817491932198370423]


def test_threshold_and_scale_rule():
    assert dc.thresh(0.0) == 0 and dc.thresh(-0.5) == 0
    assert dc.scale(0.0) == np.float32(1.0)
    assert dc.keep_mask(0.0, 99, 4, 1000).all()
    assert dc.thresh(0.2) == 13107
    assert dc.thresh(0.5) == 32768 and dc.thresh(0.1) == 6554
    assert dc.thresh(1.0 - 2.0 ** -17) == 0xFFFF                      # 65536 - 0.5 + 0.5 clamps
    assert dc.thresh(1.0 - 2.0 ** -16) == 0xFFFF
    assert dc.thresh(1.0 - 2.0 ** -15) == 65534                       # the last value below the clamp
    s = dc.scale(0.2)
    assert s.dtype == np.float32 and s == np.float32(1.0) / (np.float32(1.0) - np.float32(0.2))
    assert dc.scale(0.5) == np.float32(2.0)


def test_key_wraps_as_the_c_code_wraps():
    M64 = (1 << 64) - 1
    for seed, site in ((0, 0), (1234, 3), ((1 << 63) + 5, 7), ((1 << 64) - 1, 0xFFFFFFFF), (5, 0xFFFFFFFF)):
        want = (seed * dc.GOLDEN + ((site + 1) & 0xFFFFFFFF) * dc.SITE_MUL) & M64
        assert int(dc.make_key(seed, site)) == want, (seed, site)
    assert int(dc.make_key(5, 0xFFFFFFFF)) == (5 * dc.GOLDEN) & M64      # site + 1 wraps to 0 in 32 bits: the site term vanishes
    # element by element against the scalar statement in Python integers, at a wrapping seed and site
    seed, site, p = (1 << 63) + 5, 0xFFFFFFFF, 0.2
    key = (seed * dc.GOLDEN + ((site + 1) & 0xFFFFFFFF) * dc.SITE_MUL) & M64
    got = dc.keep_mask(p, seed, site, 41, start=3)
    for i, e in enumerate(range(3, 44)):
        z = ((e >> 2) + key) & M64
        z = ((z ^ (z >> 30)) * dc.MIX1) & M64
        z = ((z ^ (z >> 27)) * dc.MIX2) & M64
        z ^= z >> 31
        assert bool(got[i]) == (((z >> (16 * (e & 3))) & 0xFFFF) >= 13107), e


def test_start_is_an_offset_into_one_stream():
    full = dc.keep_mask(0.3, 77, 1, 1000)
    for start, n in ((0, 5), (1, 7), (2, 9), (3, 401), (998, 2)):
        assert np.array_equal(dc.keep_mask(0.3, 77, 1, n, start=start), full[start:start + n])


@pytest.mark.parametrize('p', [0.1, 0.2, 0.5])
def test_keep_rate(p):
    """test_dropout_gpu.py's own bound on the kernel's rate; the model alone deviates by at most 5.7e-4 here."""
    kept = dc.keep_mask(p, 1234, 3, 4096 * 300).mean()
    print('p = %g: kept %.6f, deviation %.2e' % (p, kept, abs(kept - (1 - p))))
    assert abs(kept - (1 - p)) < 3e-3


def test_case_lists_reach_every_row_residue():
    """The attention mask row ((prob * S + i) * S) starts on a hash group of four only when its base is a multiple of 4; the one-pass
    forward and the wide heads take another branch otherwise.  Residues 1 and 3 need an odd S."""
    for cases in (dc.ATTN_FWD_CASES, dc.ATTN_BWD_CASES):
        for route in sorted({c[0] for c in cases}):
            if route == 'sp':                   # S = 32 / 64 / 128 or S % 4 == 0 by construction: every row base is a multiple of 4
                continue
            seen = set()
            for c in cases:
                if c[0] == route:
                    seen |= dc.row_residues(c[1])
            assert seen == {0, 1, 2, 3}, (route, seen)
    assert any(S % 2 for S in dc.ATTN_S)
    assert dc.row_residues(50) == {0, 2} and dc.row_residues(33) == {0, 1, 2, 3}
    B, N, H, nh, hd, p = dc.CAND_CASES[3]
    assert {(r * H) % 4 for r in range(B * nh * N)} == {0, 1, 2, 3}


def test_site_numbers_are_distinct():
    from lime_cikm25_amd import training as T
    sites = [T._SITE_EMB, T._SITE_PE, T._SITE_ATTN, T._SITE_DROP1, T._SITE_FF, T._SITE_DROP2]
    assert len(set(sites)) == 6


def _x(shape, seed):
    g = torch.Generator().manual_seed(seed)
    mag = torch.rand(*shape, generator=g) + 0.5
    return (mag * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).numpy()


def test_bitwise_comparison_fails_on_a_shifted_mask_and_on_the_neighbouring_site():
    p, seed, site, shape = 0.2, 987654321, 2, (37, 300)
    n = shape[0] * shape[1]
    x = _x(shape, 1)
    want = dc.dropped_f32(x, dc.keep_mask(p, seed, site, n).reshape(shape), p)
    assert np.array_equal((want == 0), ~dc.keep_mask(p, seed, site, n).reshape(shape))      # |x| >= 0.5: zero iff dropped
    shifted = dc.dropped_f32(x, dc.keep_mask(p, seed, site, n, start=1).reshape(shape), p)
    other = dc.dropped_f32(x, dc.keep_mask(p, seed, site + 1, n).reshape(shape), p)
    other_seed = dc.dropped_f32(x, dc.keep_mask(p, seed + 1, site, n).reshape(shape), p)
    assert not np.array_equal(want, shifted)
    assert not np.array_equal(want, other)
    assert not np.array_equal(want, other_seed)
    assert np.array_equal(want, dc.dropped_f32(x, dc.keep_mask(p, seed, site, n).reshape(shape), p))


def test_one_flipped_mask_bit_moves_the_attention_output_past_the_bound():
    n_seq, h, S, hd = 3, 2, 33, 30
    g = torch.Generator().manual_seed(7)
    vals = torch.rand(n_seq * S, 3, h, hd, generator=g, dtype=torch.float64) * 2 - 1
    keep = dc.keep_mask(dc.P, 987654321, 2, n_seq * h * S * S).reshape(n_seq, h, S, S)
    m = torch.from_numpy(keep.astype(np.float64) * float(dc.scale(dc.P)))
    want, _ = dc.attn_ref(vals, n_seq, S, h, hd, 1.0 / math.sqrt(hd), m=m)
    for pos in ((0, 0, 0, 0), (1, 1, 17, 5), (2, 1, 32, 32)):
        flipped = keep.copy()
        flipped[pos] = ~flipped[pos]
        m2 = torch.from_numpy(flipped.astype(np.float64) * float(dc.scale(dc.P)))
        got, _ = dc.attn_ref(vals, n_seq, S, h, hd, 1.0 / math.sqrt(hd), m=m2)
        e = rel_err(got.numpy(), want.numpy())
        print('flipped %s: rel err %.2e' % (pos, e))
        assert e > dc.TIGHT, (pos, e)
