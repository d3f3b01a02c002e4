"""``kept.current`` while a stream capture is in progress: a stale holder steps aside -- nothing is computed, nothing recorded -- and is
refreshed in place by the first call after the capture.  The toy holder of tests/test_kept_cpu.py over a CUDA module; no model."""
import pytest
import torch
import torch.nn as nn

from test_kept_cpu import Toy

pytestmark = pytest.mark.gpu


def test_a_stale_holder_steps_aside_during_a_capture():
    toy = Toy(nn.Linear(4, 4).cuda())
    w = toy[0].weight
    h = toy.doubled()
    assert h.refreshes == 1 and torch.equal(h.twice, 2 * w)
    with torch.no_grad():
        w.add_(1.0)
    ptr, state, before = h.twice.data_ptr(), h.state, h.twice.clone()
    x = torch.zeros(8, device='cuda')
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x.add_(1.0)
        inside = toy.doubled(), toy.kept_key()
    assert inside == (None, (h.generation, False))
    assert h.refreshes == 1 and h.state == state and h.twice.data_ptr() == ptr and torch.equal(h.twice, before)
    assert toy.doubled() is h and h.refreshes == 2 and h.twice.data_ptr() == ptr and torch.equal(h.twice, 2 * w)
    assert not torch.equal(h.twice, before) and toy.kept_key() == (h.generation, True)
