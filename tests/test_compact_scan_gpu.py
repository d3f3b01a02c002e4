"""batch_scan_kernel (csrc/compact.hip, the one-workgroup pass of lime_compact_batch) at the boundaries of its work split: every thread
of the 1024 owns per = ceil(n / 1024) consecutive news, the five ordered scans go through one wave-level scan and one pass over the
16 wave totals.  Every output buffer of lime_compact_batch against the numpy ordered compaction of tests/test_compact_batch_gpu.py,
for n on both sides of per = 1 -> 2 -> 3 and for the live / padding patterns that put the scans' ones and zeros at the range ends."""
import numpy as np
import pytest
import torch

from test_compact_batch_gpu import np_news, np_sequences, news_outputs, run_batch, seq_outputs

pytestmark = pytest.mark.gpu

T = L = 32
SIZES = [1, 2, 1023, 1024, 1025, 2049]
PATTERNS = ['all_live', 'all_padding', 'alternating', 'padding_at_the_end', 'second_key_first']


def make_case(n, pattern):
    rng = np.random.default_rng(n)

    def texts(S):
        ids = rng.integers(1, 1000, size=(n, S)).astype(np.int32)
        lens = rng.integers(1, S + 1, size=n)
        ids[np.arange(S)[None, :] >= lens[:, None]] = 0
        return ids

    t, b = texts(T), texts(L)
    cat = rng.integers(1, 15, size=n).astype(np.int32)
    sub = rng.integers(1, 200, size=n).astype(np.int32)
    fresh = rng.uniform(60.0, 1e6, size=n).astype(np.float32)
    life = rng.uniform(600.0, 1e6, size=n).astype(np.float32)
    i = np.arange(n)
    pad = {'all_live': i < 0, 'all_padding': i >= 0, 'alternating': i % 2 == 1, 'padding_at_the_end': i == n - 1,
           'second_key_first': i % 2 == 0}[pattern]
    t[pad], b[pad], cat[pad], sub[pad], fresh[pad], life[pad] = 0, 0, 0, 0, 0.0, 0.0
    if pattern == 'second_key_first':
        # the first padded-looking news carries a second key: it is the representative, of itself alone, and the padding news behind
        # it (under the usual key) stay live -- the scan of live news counts every one of them
        cat[0] = 5
    return [t, b, cat, sub, fresh, life]


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('n', SIZES)
def test_every_buffer_against_the_ordered_compaction(n, pattern):
    arrays = make_case(n, pattern)
    ct, cb, w = run_batch(arrays)
    torch.cuda.synchronize()
    want = np_news(*arrays)
    got = news_outputs(w)
    for key in want:
        assert np.array_equal(got[key], want[key]), (n, pattern, key)
    n_news, n_live, first = (int(x) for x in want['counts'][[0, 2, 3]])
    if pattern == 'all_live':
        assert first == -1 and n_news == n_live == n
    if pattern == 'all_padding':
        assert first == 0 and n_news == 1 and n_live == 0
    if pattern == 'padding_at_the_end':
        assert first == n - 1 and n_live == n - 1 and n_news == n
    if pattern == 'second_key_first':
        assert first == 0 and n_live == n - 1 and n_news == n
    for c, ids in ((ct, arrays[0]), (cb, arrays[1])):
        for g, wnt in zip(seq_outputs(c), np_sequences(ids)):
            assert np.array_equal(g, wnt), (n, pattern)
