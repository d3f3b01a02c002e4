"""Results computed from weights alone and kept from one scoring forward to the next: the staleness rule, the per-forward fetch of
the sources, the holders' base class and the protocol every holder is asked through ("Kept across forwards").  Host only."""
import torch

from . import ops


def weight_state(sources, writes):
    """What a result derived from the tensors ``sources`` has to remember to know later whether it is still theirs: address, shape
    and version counter of each (an in-place torch op, ``load_state_dict`` or ``copy_`` moves the version; ``.to()`` / a re-pointed
    ``.data`` the address) and ``writes``, the count of writes torch does not see (``ops.PARAM_WRITES``: the native optimizer step
    goes through raw pointers).  An edit through ``tensor.data`` moves none of the three: ``Model.weights_changed()``.  Host only."""
    return tuple((t.data_ptr(), tuple(t.shape), t._version) for t in sources), int(writes)


def weight_state_stale(recorded, current):
    """The staleness rule of ``WeightProducts``: None while ``recorded`` (the ``weight_state`` a result was computed under) still
    describes the sources, else why not -- 'never' (nothing recorded), 'moved' (a source's address or shape differs, or their number),
    'version' (an in-place write torch counted), 'writes' (a raw-pointer write was announced).  Pure: two tuples in, a word out."""
    if recorded is None:
        return 'never'
    if recorded == current:                       # (one tuple comparison: the answer of nearly every forward)
        return None
    (rec, rec_writes), (cur, cur_writes) = recorded, current
    if len(rec) != len(cur) or any(a[:2] != b[:2] for a, b in zip(rec, cur)):
        return 'moved'
    if any(a[2] != b[2] for a, b in zip(rec, cur)):
        return 'version'
    return 'writes' if rec_writes != cur_writes else None


class SourcePaths:
    """Where the source tensors of a kept result live below ``root``, so that every forward can fetch them without walking the module
    tree through ``nn.Module.__getattr__`` (the walk cost more than the comparison it feeds: 8 us for LIME's six tensors, 26 us for
    CROWN's, in front of every graph replay).  ``leaves``: (the owning module's parameter or buffer dictionary, name) per source, in the
    order of the slow list they were found from; ``links``: (a module's child dictionary, name, child) for every hop on the way.
    ``tensors()`` returns the sources as they are now -- a re-assigned parameter is read from its dictionary like any other -- or None
    once a hop leads to another module than it did; the caller then asks the slow list again."""

    def __init__(self, links, leaves, tag):
        self.links, self.leaves, self.tag = links, leaves, tag

    @classmethod
    def find(cls, root, tensors, tag=None):
        """The paths of ``tensors`` (found by identity among root's parameters and buffers), or None when one of them is not there."""
        where = {}
        for prefix, mod in root.named_modules(remove_duplicate=False):
            for d in (mod._parameters, mod._buffers):
                for name, t in d.items():
                    if t is not None:
                        where.setdefault(id(t), (prefix, d, name))
        links, leaves, seen = [], [], set()
        for t in tensors:
            if id(t) not in where:
                return None
            prefix, d, name = where[id(t)]
            leaves.append((d, name))
            mod, path = root, ''
            for hop in (prefix.split('.') if prefix else []):
                child = mod._modules[hop]
                path += '.' + hop
                if path not in seen:
                    seen.add(path)
                    links.append((mod._modules, hop, child))
                mod = child
        return cls(links, leaves, tag)

    def tensors(self, tag=None):
        if tag != self.tag or any(d.get(name) is not child for d, name, child in self.links):
            return None
        return [d[name] for d, name in self.leaves]


def kept_sources(module, slot, slow, tag=None):
    """``slow()`` -- a module's list of source tensors -- through the ``SourcePaths`` kept in ``module.__dict__[slot]``: found at the
    first call, asked from then on, found again when a hop or ``tag`` changed.  The module drops the slot in ``_apply``."""
    paths = module.__dict__.get(slot)
    if paths is not None:
        ts = paths.tensors(tag)
        if ts is not None:
            return ts
    ts = slow()
    module.__dict__[slot] = SourcePaths.find(module, ts, tag)
    return ts


_GENERATION = [0]


def _next_generation():
    """Process-wide, so that no two sets of product buffers ever carry one number: a module that lost its ``WeightProducts``
    (``_apply``) and built another must not look unchanged to a holder of captured graphs."""
    _GENERATION[0] += 1
    return _GENERATION[0]


class Kept:
    """Base of a holder of kept results.  ``state`` / ``config``: the ``weight_state`` and whatever else they were computed under
    (recorded by ``current``); ``refreshes``: recomputations so far (tests, logs).  A subclass names its buffers and fills them in
    ``refresh(owner, config)`` -- IN PLACE, through ``buffer``: captured HIP graphs hold the addresses.  ``generation`` takes a new
    process-wide number whenever a buffer had to be (re)allocated or was let go instead; whoever holds graphs drops them then."""

    def __init__(self):
        self.state = self.config = None
        self.generation = _next_generation()
        self.refreshes = 0

    def buffer(self, old, shape, dtype, device):
        """``old`` where it still fits, else a new tensor and a new generation."""
        if old is not None and tuple(old.shape) == tuple(shape) and old.dtype == dtype and old.device == device:
            return old
        self.generation = _next_generation()
        return torch.empty(shape, dtype=dtype, device=device)

    def let_go(self):
        """The subclass dropped something it kept: a graph that reads it must not be replayed."""
        self.generation = _next_generation()


def current(owner, slot, make, sources, config=None, create=True):
    """The holder in ``owner.__dict__[slot]``, current for ``sources`` (fetched by the owner: ``kept_sources``) and ``config`` as they
    are now: a stale or new (``make()``) one is refreshed here, on the current stream and outside autograd.  None: there is none and
    ``create`` is false (nothing is built), or it is stale and a stream capture is in progress (nothing can be computed outside the
    graph then; the caller computes its own inside).  Whether the owner keeps anything at all is its gate, in front of this call."""
    holder = owner.__dict__.get(slot)
    if holder is None and not create:
        return None
    state = weight_state(sources, ops.PARAM_WRITES)
    if holder is not None and holder.state == state and holder.config == config:       # (nearly every forward ends here)
        return holder
    if sources[0].is_cuda and torch.cuda.is_current_stream_capturing():
        return None
    if holder is None:
        holder = owner.__dict__[slot] = make()
    with torch.no_grad():
        holder.refresh(owner, config)
    holder.state, holder.config = state, config
    holder.refreshes += 1
    return holder


def key(owner, slot, ask):
    """Changes whenever a graph captured over the owner's forward must not be replayed any more: a kept buffer was (re)allocated or
    let go, or the forward switched between the kept results and its own.  ``ask``: the owner's accessor -- with ``create=False`` it
    brings an existing holder up to date (in place) and builds none."""
    used = ask(create=False) is not None
    holder = owner.__dict__.get(slot)
    return (None if holder is None else holder.generation, used)


def forget(owner, slot, paths_slot):
    """For the owner's ``_apply``: parameter storage moves (and maybe the device), nothing kept stays valid."""
    owner.__dict__[slot] = owner.__dict__[paths_slot] = None
