"""Sentinel-guarded buffers for the buffer-discipline tests (plain torch, no library call).

A window handed to a kernel lies inside one larger allocation that is filled with a quiet NaN
carrying a payload.  The guards on both sides are as large as the window itself, so a store that
overshoots by a whole plane or batch item still lands in memory this module owns: a test built
on it can fail, it cannot fault.  Afterwards
  check_guards   no word outside the window changed (a write out of bounds),
  check_written  no word inside a pure output is still the sentinel (an element skipped),
  check_clean    no word of a result carries the sentinel's payload (a read out of bounds that
                 reached the arithmetic: NaN * 0 is NaN, and the payload survives).
"""
import torch

SENTINEL = 0x7FC5A5A5          # a quiet NaN with a payload; not the canonical 0x7FC00000
PAYLOAD_MASK = 0x003FFFFF      # the payload below the quiet bit
SENTINEL64 = 0x7FF8A5A5A5A5A5A5  # the same for float64 windows (the MVSEC event rows)
MIN_GUARD = 1024               # words on each side, at least
ALIGN_WORDS = 64               # the aligned window starts on a multiple of 256 bytes


def _sentinel(t):
    """The sentinel of a buffer or window, by its element size."""
    return SENTINEL if t.element_size() == 4 else SENTINEL64


def _bits(t):
    """A float or integer tensor as integer words of its own width (flat)."""
    return t.reshape(-1).view(torch.int32 if t.element_size() == 4 else torch.int64)


def guarded(n, device, align16=True, dtype=torch.float32):
    """(big, view): `view` is a window of n elements of `dtype` inside the integer buffer `big`
    (int32 for float32; int64 for the float64 variant), every word of which is the sentinel.  At
    least max(MIN_GUARD, n) sentinel words lie on each side.  align16: the window starts on a
    256-byte boundary of the allocation (which satisfies every 16-byte contract); otherwise one
    element further, so that it has its dtype's own alignment and nothing more."""
    if dtype not in (torch.float32, torch.float64):
        raise TypeError(f"guarded: float32 or float64 windows only (got {dtype})")
    word = torch.int32 if dtype == torch.float32 else torch.int64
    guard = -(-max(MIN_GUARD, n) // ALIGN_WORDS) * ALIGN_WORDS
    lead = guard if align16 else guard + 1
    big = torch.full((lead + n + guard + 1,), SENTINEL if word == torch.int32 else SENTINEL64, dtype=word,
                     device=device)
    view = big[lead:lead + n].view(dtype)
    assert view.numel() == n and view.data_ptr() == big.data_ptr() + big.element_size() * lead
    return big, view


def _lead(big, view):
    """The window's first word in `big`."""
    off, es = view.data_ptr() - big.data_ptr(), big.element_size()
    assert view.element_size() == es and off % es == 0 and 0 < off // es, "view is not a window of big"
    assert off // es + view.numel() < big.numel(), "view is not a window of big"
    return off // es


def _describe(idx, base):
    """Offsets (in words of the buffer, relative to the window's first word) of the touched words."""
    idx = idx + base
    return f"{idx.numel()} word(s) at window offset {int(idx[0])} .. {int(idx[-1])}"


def guard_damage(big, view):
    """None, or a description of the guard words that no longer hold the sentinel."""
    lead, nw, sentinel = _lead(big, view), view.numel(), _sentinel(big)
    msgs = []
    before = (big[:lead] != sentinel).nonzero().flatten()
    if before.numel():
        msgs.append("before the window: " + _describe(before, -lead))
    after = (big[lead + nw:] != sentinel).nonzero().flatten()
    if after.numel():
        msgs.append(f"past the window's {nw} words: " + _describe(after, nw))
    return "; ".join(msgs) or None


def check_guards(big, view, name="buffer"):
    """Both guards still hold the sentinel, bit for bit."""
    damage = guard_damage(big, view)
    assert damage is None, f"{name}: written outside the window, {damage}"


def check_written(view, name="output"):
    """No word of a pure, fully written output still equals the sentinel."""
    w = _bits(view)
    left = (w == _sentinel(view)).nonzero().flatten()
    assert left.numel() == 0, f"{name}: not written, {_describe(left, 0)} of {w.numel()}"


def carries_sentinel(t):
    """Indices of the words of the float32 tensor `t` that are NaNs with the sentinel's payload."""
    w = _bits(t.contiguous())
    hit = ((w & 0x7F800000) == 0x7F800000) & ((w & PAYLOAD_MASK) == (SENTINEL & PAYLOAD_MASK))
    return hit.nonzero().flatten()


def check_clean(t, name="output"):
    """No word of a result carries the sentinel's payload: nothing outside the inputs was read
    into the arithmetic."""
    hit = carries_sentinel(t)
    assert hit.numel() == 0, f"{name}: the sentinel reached the result, {_describe(hit, 0)}"
