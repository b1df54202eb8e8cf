"""Tensors derived from parameters (an fp32 copy, a packed or re-ordered weight, a sum of two biases, a batched plan): the ONE place
that decides whether such a value still belongs to the tensors it was made from.

A Signature of a tuple of source tensors and a hashable `extra` (a kernel's packing order, ...) holds for `sources` when
  * every source is the same live object (weak reference and `is`): Python reuses object ids and the caching allocator reuses
    addresses, so (id, data_ptr, version) of a freed model's parameter can all recur in the next model;
  * every source still has the same (data_ptr, _version, dtype, device, shape);
  * `extra` is equal.
derived(tag, sources, build, extra) keeps build()'s value in one process-wide table under (tag, the ids of the sources) for as long as
its signature holds; derived1 is the same for a single source without the loops (per-call host path of every kernel wrapper). The
table holds the derived value strongly and nothing else: never a source, and the entry leaves when any source dies (weak-reference
finaliser), so there is no size cap and nothing to clear. Values that must coexist for one source (per mode, per dtype) differ in `tag`.

The one known limit: a write through another alias of a source's storage (`p.data.add_(1)`, `buf.copy_(..)` for a parameter made
from `buf.data`) does not bump `p._version`, so it is not seen. Writes through the source itself (`p.add_`, `p.copy_`, an optimizer
step, load_state_dict) are.
"""
import weakref

_table = {}                   # (tag, (id(source), ...)) -> (Signature, value)  |  derived1, (tag, id(source)) -> (ref, (*state, extra), value)


def _state(s):
    return (s.data_ptr(), s._version, s.dtype, s.device, s.shape)


class Signature:
    """What `sources` (a sequence of tensors) and `extra` were when it was taken; compares by identity (a new signature is a new
    owner). on_death(ref): called when any source is freed."""
    __slots__ = ("refs", "state", "extra")

    def __init__(self, sources, extra=(), on_death=None):
        self.refs = tuple(weakref.ref(s, on_death) for s in sources)
        self.state = [_state(s) for s in sources]
        self.extra = extra

    def holds(self, sources, extra=()):
        if len(self.refs) != len(sources) or self.extra != extra:
            return False
        for r, s in zip(self.refs, sources):
            if r() is not s:
                return False
        return self.state == [(s.data_ptr(), s._version, s.dtype, s.device, s.shape) for s in sources]


def _finaliser(key, table=_table, ref_type=weakref.ref):
    """For the weak references of an entry's sources: the entry goes if the dying reference is (still) one of its own. Everything it
    needs is bound here, so it also runs while the interpreter shuts down."""
    def drop(ref):
        e = table.get(key)
        if e is not None and (e[0] is ref or (type(e[0]) is not ref_type and ref in e[0].refs)):
            del table[key]                  # (`ref` is dead: `in` compares dead references by identity)
    return drop


def derived(tag, sources, build, extra=()):
    """The cached build() for these sources: rebuilt when the entry's signature no longer holds."""
    key = (tag, tuple(map(id, sources)))
    e = _table.get(key)
    if e is not None and e[0].holds(sources, extra):
        return e[1]
    value = build()
    _table[key] = (Signature(sources, extra, _finaliser(key)), value)
    return value


def derived1(tag, source, build, extra=()):
    """derived(tag, (source,), lambda: build(source), extra) with Signature.holds written out for the one source."""
    key = (tag, id(source))
    e = _table.get(key)
    if e is not None and e[0]() is source and e[1] == (source.data_ptr(), source._version, source.dtype, source.device, source.shape, extra):
        return e[2]
    value = build(source)
    _table[key] = (weakref.ref(source, _finaliser(key)), (*_state(source), extra), value)
    return value
