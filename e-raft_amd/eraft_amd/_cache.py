"""The one cache of what is made from a module's parameter tensors for the kernels: the weight
packs of corr, gru, update, encoder and upsample, and an eval-mode batch norm's scale and shift.

An entry is keyed by its kind and the tensors' ids and holds weak references to them, so nothing
is attached to a Parameter (pickling and torch.save of the model are unaffected), the entry goes
when any of the tensors does, and another module's tensors never see it.  (A WeakKeyDictionary
cannot hold tensors: its key comparison calls Tensor.__eq__.)  With the references it keeps the
(data_ptr, _version)s the value was made from: an in-place update (an optimizer step,
load_state_dict's copy_) bumps _version and the value is made again.  Making one launches kernels
and allocates, so it is refused inside a graph capture.
"""
from __future__ import annotations

import weakref

import torch

_ENTRIES = {}  # (kind, ids of the tensors) -> (weakrefs to them, their (data_ptr, _version)s + extra, value)


def cached(kind, tensors, what, make, extra=()):
    """`make()`'s value for the parameter tensors `tensors`, made once per (kind, tensors) and again
    when one of them was replaced or updated in place, or `extra` (hashable values that the result
    depends on besides the tensors) changed.  `what` names the value in the error raised when it
    would have to be made inside a graph capture."""
    ids = (kind,) + tuple(id(t) for t in tensors)
    key = tuple((t.data_ptr(), t._version) for t in tensors) + tuple(extra)
    ent = _ENTRIES.get(ids)
    if ent is None or any(r() is not t for r, t in zip(ent[0], tensors)) or ent[1] != key:
        if tensors[0].is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{what} must be made before a graph capture "
                               "(run one forward outside the capture first)")
        drop = lambda _r, ids=ids: _ENTRIES.pop(ids, None)
        ent = (tuple(weakref.ref(t, drop) for t in tensors), key, make())
        _ENTRIES[ids] = ent
    return ent[2]
