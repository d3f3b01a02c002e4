"""The protocol of lime_cikm25_amd.kept -- ``current``, ``key``, ``forget`` and the one buffer rule of ``Kept`` -- through a toy holder
over a CPU module.  Host only: a ``torch.cuda`` call for CPU sources would fail on a machine without a GPU."""
import torch
import torch.nn as nn

from lime_cikm25_amd import kept, ops


class Doubled(kept.Kept):
    """Keeps 2 * weight in one buffer."""
    twice = None

    def refresh(self, owner, config):
        w = owner[0].weight
        self.twice = torch.mul(w, 2, out=self.buffer(self.twice, w.shape, w.dtype, w.device))


class Toy(nn.Sequential):
    """One hop (``self[0]``) to the sources, so that ``SourcePaths`` has a link to follow."""
    config = None

    def doubled(self, create=True):
        return kept.current(self, '_doubled', Doubled, kept.kept_sources(self, '_doubled_paths', lambda: [self[0].weight]), self.config,
                            create)

    def kept_key(self):
        return kept.key(self, '_doubled', self.doubled)

    def _apply(self, fn, *args, **kwargs):
        kept.forget(self, '_doubled', '_doubled_paths')
        return super()._apply(fn, *args, **kwargs)


def test_the_protocol_through_a_toy_holder():
    toy = Toy(nn.Linear(3, 2))
    w = toy[0].weight
    # no holder: none is built unless asked for, and the key says so
    assert toy.doubled(create=False) is None and toy.kept_key() == (None, False) and toy.__dict__.get('_doubled') is None
    # the first call builds it; the second finds it current
    h = toy.doubled()
    assert isinstance(h, Doubled) and toy.__dict__['_doubled'] is h and isinstance(toy.__dict__['_doubled_paths'], kept.SourcePaths)
    assert h.refreshes == 1 and torch.equal(h.twice, 2 * w)
    ptr, gen = h.twice.data_ptr(), h.generation
    assert toy.doubled() is h and toy.doubled(create=False) is h and h.twice.data_ptr() == ptr and h.refreshes == 1
    assert toy.kept_key() == (gen, True) and h.refreshes == 1
    # an in-place op: refreshed in place, the generation stays
    with torch.no_grad():
        w.add_(1.0)
    assert toy.doubled() is h and h.refreshes == 2 and h.twice.data_ptr() == ptr and h.generation == gen and torch.equal(h.twice, 2 * w)
    # a .data edit moves neither version nor address: nothing happens until somebody says so, then one refresh
    w.data.mul_(3.0)
    assert toy.doubled() is h and h.refreshes == 2 and not torch.equal(h.twice, 2 * w)
    ops.note_param_write()
    assert toy.doubled() is h and toy.doubled() is h and h.refreshes == 3 and torch.equal(h.twice, 2 * w)
    assert h.twice.data_ptr() == ptr and h.generation == gen
    # another config: one refresh (the key brings the holder up to date as well)
    toy.config = 'other'
    assert toy.kept_key() == (gen, True) and h.refreshes == 4 and toy.doubled() is h and h.refreshes == 4 and h.config == 'other'
    # a parameter of another shape: the buffer cannot be reused -- a new generation, and nobody else's
    other = Toy(nn.Linear(3, 2)).doubled()
    toy[0].weight = nn.Parameter(torch.ones(5, 3))
    assert toy.doubled() is h and h.refreshes == 5 and tuple(h.twice.shape) == (5, 3) and torch.equal(h.twice, 2 * toy[0].weight)
    assert len({gen, other.generation, h.generation}) == 3 and toy.kept_key() == (h.generation, True)
    # _apply: holder and paths are forgotten, and the next holder repeats no number
    seen = {gen, other.generation, h.generation}
    toy.double()
    assert toy.__dict__['_doubled'] is None and toy.__dict__['_doubled_paths'] is None and toy.kept_key() == (None, False)
    again = toy.doubled()
    assert again is not h and again.refreshes == 1 and again.twice.dtype == torch.float64 and again.generation not in seen
    assert toy.kept_key() == (again.generation, True)
