"""CNE's per-news recurrence cache, the parts that go without a GPU: the refusals under another content encoder, the new keyword
arguments and their defaults (which select the routes as they were), and the packed-size arithmetic."""
import inspect

import pytest
import torch

from lime_cikm25_amd import Model, make_config, newsEncoders, util
from lime_cikm25_amd.trainer import Trainer


@pytest.fixture(scope='module')
def cnn_model():
    cfg = make_config(content_encoder='CNN', vocabulary_size=200, max_history_num=3, max_title_length=8, max_abstract_length=16)
    return Model(cfg)


def test_a_model_without_cne_has_no_recurrence_cache(cnn_model):
    with pytest.raises(ValueError, match='CNN'):
        cnn_model.build_recurrence_cache(None)                      # refused before the corpus is looked at
    with pytest.raises(ValueError, match='CNN'):
        cnn_model.score_behaviors(None, [0], torch.empty(1, 0), recurrence_cache=object())


@pytest.mark.parametrize('fn,defaults', [
    (Model.score_behaviors, dict(recurrence_cache=None, rows_per_forward=None, n_src=None)),
    (Model.build_recurrence_cache, dict(news_per_pass=None)),
    (util.compute_scores_cached, dict(recurrence_cache=False, rows_per_forward=None)),
    (util.evaluate_cached_on_device, dict(recurrence_cache=False)),
    (Trainer.__init__, dict(cne_recurrence_cache=False, cached_eval=True, device_eval=False)),
    (newsEncoders.CNE.encode_cached_flat, dict(pair_groups=None)),
    (newsEncoders.CNE.build_recurrence_cache, dict(news_per_pass=None)),
])
def test_new_arguments_default_to_the_routes_as_they_were(fn, defaults):
    params = inspect.signature(fn).parameters
    for name, value in defaults.items():
        assert name in params, '%s lacks %s' % (fn.__qualname__, name)
        assert params[name].default is value or params[name].default == value, (fn.__qualname__, name, params[name].default)


def test_packed_size_arithmetic():
    """nbytes per text = 2 . sum(lens) . C . 4 (h, hh) + n . C . 4 (m) + n . 4 (lens) + (n + 1) . 8 (offsets), C = 2 hidden_dim."""
    lens_t, lens_b, h = [1, 7, 32, 12], [128, 1, 40, 99], 400
    C = 2 * h
    want = sum(2 * sum(l) * C * 4 + len(l) * C * 4 + len(l) * 4 + (len(l) + 1) * 8 for l in (lens_t, lens_b))
    assert newsEncoders.CNERecurrenceCache.packed_nbytes(lens_t, lens_b, h) == want
    # 6.4 KB per live token, against 1 MB per news for a dense cache at the defaults (32 + 128 slots)
    assert 2 * C * 4 == 6400 and (32 + 128) * 2 * C * 4 == 1024000
    per_token = (newsEncoders.CNERecurrenceCache.packed_nbytes([2], [2], h) - newsEncoders.CNERecurrenceCache.packed_nbytes([1], [1], h)) / 2
    assert per_token == 6400
    # the object adds up the tensors it holds to the same figure
    Text = newsEncoders.CNERecurrenceCache.Text
    def text(lens, S):
        n, rows = len(lens), sum(lens)
        return Text(S, torch.tensor(lens, dtype=torch.int32), torch.zeros(n + 1, dtype=torch.int64), torch.zeros(rows, C), torch.zeros(rows, C),
                    torch.zeros(n, C))
    cache = newsEncoders.CNERecurrenceCache(text(lens_t, 32), text(lens_b, 128), (), torch.zeros(0, dtype=torch.int64))
    assert cache.nbytes == want and cache.n_news == 4
