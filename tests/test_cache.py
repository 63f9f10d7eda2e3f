"""The parameter cache behind every weight pack (eraft_amd/_cache.py): CPU tensors and a counting
`make`, no library call.  What the GPU tests of the packs check through a kernel (a re-pack after
an in-place update, one entry per kind of pack, the refusal inside a graph capture) rests on these
properties."""
import gc

import torch

from eraft_amd import _cache
from eraft_amd._cache import cached


class _Make:
    """make() returns a fresh object and counts its calls."""

    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return object()


def _params():
    return torch.zeros(3), torch.ones(2)


def test_same_tensors_make_once():
    ts, make = _params(), _Make()
    first = cached("t_once", ts, "the value", make)
    assert cached("t_once", ts, "the value", make) is first
    assert cached("t_once", list(ts), "the value", make) is first  # the tensors count, not their container
    assert make.calls == 1


def test_in_place_update_makes_again():
    ts, make = _params(), _Make()
    first = cached("t_inplace", ts, "the value", make)
    ts[1].add_(1.0)
    second = cached("t_inplace", ts, "the value", make)
    assert second is not first and make.calls == 2
    assert cached("t_inplace", ts, "the value", make) is second and make.calls == 2
    ts[0].data = torch.zeros(3)  # new storage under the same tensor object
    assert cached("t_inplace", ts, "the value", make) is not second and make.calls == 3


def test_equal_values_in_another_tensor_have_their_own_entry():
    a, b, make = _params(), _params(), _Make()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    va, vb = cached("t_other", a, "the value", make), cached("t_other", b, "the value", make)
    assert va is not vb and make.calls == 2
    assert cached("t_other", a, "the value", make) is va and cached("t_other", b, "the value", make) is vb
    assert cached("t_other", (a[0], b[1]), "the value", make) not in (va, vb)  # one tensor differs
    assert make.calls == 3


def test_kinds_do_not_share_an_entry():
    ts, m1, m2 = _params(), _Make(), _Make()
    v1, v2 = cached("t_kind_1", ts, "one value", m1), cached("t_kind_2", ts, "another value", m2)
    assert v1 is not v2 and (m1.calls, m2.calls) == (1, 1)
    assert cached("t_kind_1", ts, "one value", m1) is v1 and cached("t_kind_2", ts, "another value", m2) is v2
    assert (m1.calls, m2.calls) == (1, 1)


def test_entries_go_with_their_tensors():
    gc.collect()
    before = dict(_cache._ENTRIES)
    ts, make = _params(), _Make()
    cached("t_gone_1", ts, "the value", make)
    cached("t_gone_2", ts[:1], "the value", make)
    assert len(_cache._ENTRIES) == len(before) + 2
    del ts
    gc.collect()
    assert _cache._ENTRIES == before
    # one dead tensor of two is enough
    keep, make = torch.zeros(1), _Make()
    ts = (keep, torch.ones(1))
    cached("t_gone_3", ts, "the value", make)
    del ts
    gc.collect()
    assert _cache._ENTRIES == before


def test_extra_makes_again():
    ts, make = _params(), _Make()
    first = cached("t_extra", ts, "the value", make, extra=(1e-5,))
    assert cached("t_extra", ts, "the value", make, extra=(1e-5,)) is first and make.calls == 1
    second = cached("t_extra", ts, "the value", make, extra=(1e-3,))
    assert second is not first and make.calls == 2
    assert cached("t_extra", ts, "the value", make, extra=(1e-3,)) is second and make.calls == 2


def test_cpu_tensors_take_no_part_in_the_stream_ordering(monkeypatch):
    """Off the GPU an entry keeps no stream and no event, and neither a make nor a hit asks torch.cuda
    for anything (the ordering of a hit behind the make on another stream is tests/test_family_discipline.py's)."""
    def refuse(*a, **k):
        raise AssertionError("torch.cuda was asked about streams for CPU tensors")
    for name in ("current_stream", "is_current_stream_capturing", "Event"):
        monkeypatch.setattr(torch.cuda, name, refuse)
    ts, make = _params(), _Make()
    first = cached("t_cpu_streams", ts, "the value", make)
    assert cached("t_cpu_streams", ts, "the value", make) is first and make.calls == 1
    ent = _cache._ENTRIES[("t_cpu_streams",) + tuple(id(t) for t in ts)]
    assert ent[2] is first and ent[3] is None


def test_the_tensors_of_a_value():
    """What a hit from another stream records the stream on: the value itself, or the tensors of a
    (nested) tuple or list; anything else holds no device memory of its own."""
    a, b = _params()
    assert _cache._value_tensors(a) == (a,)
    assert _cache._value_tensors((a, b)) == (a, b) and _cache._value_tensors([a, (b, a)]) == (a, b, a)
    assert _cache._value_tensors(object()) == () and _cache._value_tensors((1.0, None)) == ()
