"""What is remembered about a caller's object -- the uint8 twin of a label volume, the prior of an image, the shape a tensor
was checked against, the pointer block of a subject -- is remembered for the OBJECT: recognised by its `id()` and a weak
reference that must still resolve to it (a new tensor at a recycled address is a new object), so nothing here keeps a
caller's volume alive and the entry goes when the object dies.  An entry may carry a stamp (a tensor's in-place `_version`)
and is then found under that stamp only, and says how many bytes its value holds (`make_room` keeps them within a budget).
"""
from __future__ import annotations

import weakref


def _none():  # stands where the weak reference of the None in a pair would (a subject without a bank)
    return None


class IdentityCache:
    """A value per object, or per pair of objects `(a, b)` -- each recognised as above, either may be None."""

    def __init__(self, cap: int = 4096):
        self._entries = {}  # id | (id, id) -> [weak reference | (weak reference) x 2, stamp, value, nbytes], oldest first
        self._cap = cap     # an insert into a cache of more entries than this clears it first
        self.bytes = 0

    def __len__(self):
        return len(self._entries)

    def get(self, obj, stamp=None):
        """The value put for `obj` under `stamp`, or None.  An entry found stale (another object, another stamp) is dropped."""
        if type(obj) is not tuple:  # a dict lookup, a weak reference call, a compare
            key = id(obj)
            ent = self._entries.get(key)
            same = ent is not None and ent[0]() is obj
        else:
            a, b = obj
            key = (id(a), id(b))
            ent = self._entries.get(key)
            same = ent is not None and ent[0][0]() is a and ent[0][1]() is b
        if same and ent[1] == stamp:
            return ent[2]
        self._remove(key)
        return None

    def put(self, obj, value, nbytes: int = 0, stamp=None):
        """Remember `value`, which holds `nbytes`, for `obj`.  An object that has an entry keeps its place in the order
        (`drop` it first to make it the youngest).  No budget is looked at here: that is `make_room`, beforehand."""
        pair = type(obj) is tuple
        key = (id(obj[0]), id(obj[1])) if pair else id(obj)
        old = self._entries.get(key)
        if old is not None:
            self.bytes -= old[3]
        elif len(self._entries) > self._cap:
            self.clear()
        me = weakref.ref(self)  # the objects' death must find the cache, not keep it (and what it holds) alive

        def died(_ref):
            cache = me()
            if cache is not None:
                cache._remove(key)

        refs = tuple([weakref.ref(o, died) if o is not None else _none for o in obj]) if pair else weakref.ref(obj, died)
        self._entries[key] = [refs, stamp, value, nbytes]
        self.bytes += nbytes

    def make_room(self, nbytes: int, budget: int) -> bool:
        """Evict entries that hold bytes, oldest first, until `nbytes` more fit into `budget`; False if they still do not.
        Entries without bytes (what the caller owns and accounts for, plain facts) are never evicted."""
        while self.bytes + nbytes > budget:
            victim = next((k for k, e in self._entries.items() if e[3]), None)
            if victim is None:
                break
            self._remove(victim)
        return self.bytes + nbytes <= budget

    def drop(self, obj):
        self._remove((id(obj[0]), id(obj[1])) if type(obj) is tuple else id(obj))

    def _remove(self, key):
        ent = self._entries.pop(key, None)
        if ent is not None:
            self.bytes -= ent[3]

    def clear(self):
        self._entries.clear()
        self.bytes = 0
