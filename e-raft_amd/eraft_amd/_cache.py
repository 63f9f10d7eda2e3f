"""The one cache of what is made from a module's parameter tensors for the kernels: the weight
packs of corr, gru, update, encoder and upsample, and an eval-mode batch norm's scale and shift.

An entry is keyed by its kind and the tensors' ids and holds weak references to them, so nothing
is attached to a Parameter (pickling and torch.save of the model are unaffected), the entry goes
when any of the tensors does, and another module's tensors never see it.  (A WeakKeyDictionary
cannot hold tensors: its key comparison calls Tensor.__eq__.)  With the references it keeps the
(data_ptr, _version)s the value was made from: an in-place update (an optimizer step,
load_state_dict's copy_) bumps _version and the value is made again.  Making one launches kernels
and allocates, so it is refused inside a graph capture.

Streams.  A value is made by kernels on the stream that is current at the first call, and the
caller never sees it, so it cannot order a later use on another stream behind that work itself.
The entry therefore keeps the making stream and an event recorded on it after make(); a hit from
any other stream makes that stream wait for the event (no host synchronisation) and records the
stream on the value's tensors (Tensor.record_stream), so that the allocator does not hand their
memory out again, after a re-pack or when the module goes, while that stream may still read it.  A
hit on the making stream adds nothing, and neither does a hit inside a graph capture:
torch.cuda.graph synchronises the device before it captures, so every pack made before is complete.
"""
from __future__ import annotations

import weakref

import torch

# (kind, ids of the tensors) -> (weakrefs to them, their (data_ptr, _version)s + extra, value,
#                                the making stream and the event after make(), or None off the GPU)
_ENTRIES = {}


def _value_tensors(value):
    """The tensors of a cached value (a tensor, or a tuple or list of them)."""
    if isinstance(value, torch.Tensor):
        return (value,)
    if isinstance(value, (tuple, list)):
        return tuple(t for v in value for t in _value_tensors(v))
    return ()


def _order_after_make(made, value, device):
    """A hit on a value made on another stream: the current stream waits for the make and is
    recorded as a user of the value's memory."""
    stream, event = made
    cur = torch.cuda.current_stream(device)
    if cur == stream or torch.cuda.is_current_stream_capturing():
        return
    cur.wait_event(event)
    for t in _value_tensors(value):
        if t.is_cuda:
            t.record_stream(cur)


def cached(kind, tensors, what, make, extra=()):
    """`make()`'s value for the parameter tensors `tensors`, made once per (kind, tensors) and again
    when one of them was replaced or updated in place, or `extra` (hashable values that the result
    depends on besides the tensors) changed.  `what` names the value in the error raised when it
    would have to be made inside a graph capture.  On the GPU the value is safe to use on the
    stream that is current at this call, whichever stream made it."""
    ids = (kind,) + tuple(id(t) for t in tensors)
    key = tuple((t.data_ptr(), t._version) for t in tensors) + tuple(extra)
    ent = _ENTRIES.get(ids)
    if ent is None or any(r() is not t for r, t in zip(ent[0], tensors)) or ent[1] != key:
        made = None
        if tensors[0].is_cuda:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{what} must be made before a graph capture "
                                   "(run one forward outside the capture first)")
            made = (torch.cuda.current_stream(tensors[0].device), torch.cuda.Event())
        drop = lambda _r, ids=ids: _ENTRIES.pop(ids, None)
        value = make()
        if made is not None:
            made[1].record(made[0])
        ent = (tuple(weakref.ref(t, drop) for t in tensors), key, value, made)
        _ENTRIES[ids] = ent
    elif ent[3] is not None:
        _order_after_make(ent[3], ent[2], tensors[0].device)
    return ent[2]
