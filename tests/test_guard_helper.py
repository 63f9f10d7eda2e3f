"""tests/_guard.py against fake "kernels" made of torch ops on CPU tensors: a helper that cannot
fail is worth nothing, so each way it must fail is pinned here, with the offset it reports."""
import numpy as np
import pytest
import torch

import _guard
from _util import bit_equal


def _as_int(v):
    return v.view(torch.int32)


def test_sentinel_is_a_quiet_nan_with_a_payload():
    f = np.array([_guard.SENTINEL], np.uint32).view(np.float32)[0]
    assert np.isnan(f)
    assert _guard.SENTINEL & 0x00400000, "quiet bit"
    assert _guard.SENTINEL != 0x7FC00000 and _guard.SENTINEL & _guard.PAYLOAD_MASK


@pytest.mark.parametrize("n", [1, 7, 1000, 5000])
@pytest.mark.parametrize("align16", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_layout(n, align16, dtype):
    big, view = _guard.guarded(n, "cpu", align16, dtype)
    es = view.element_size()
    sentinel = _guard.SENTINEL if es == 4 else _guard.SENTINEL64
    lead = (view.data_ptr() - big.data_ptr()) // es
    assert big.element_size() == es and not big.dtype.is_floating_point
    assert view.dtype == dtype and view.numel() == n and view.is_contiguous()
    assert lead >= max(1024, n) and big.numel() - lead - n >= max(1024, n)
    assert big.data_ptr() % 64 == 0
    if align16:
        assert view.data_ptr() % 256 == big.data_ptr() % 256       # every 16-byte contract holds
    else:
        assert (view.data_ptr() - big.data_ptr()) % 16 == es       # the dtype's own alignment and no more
    assert bool((big == sentinel).all())
    assert bool(torch.isnan(view).all())
    # the view aliases the buffer
    view.fill_(1.0)
    assert int((big != sentinel).sum()) == n
    _guard.check_guards(big, view)
    _guard.check_written(view)
    if es == 4:
        _guard.check_clean(view)


def test_in_bounds_kernel_passes():
    big, view = _guard.guarded(37, "cpu")
    view.copy_(torch.arange(37, dtype=torch.float32))
    _guard.check_guards(big, view)
    _guard.check_written(view)
    _guard.check_clean(view)


@pytest.mark.parametrize("align16", [True, False])
def test_write_one_float_past_the_end_is_reported(align16):
    n = 37
    big, view = _guard.guarded(n, "cpu", align16)
    lead = (view.data_ptr() - big.data_ptr()) // 4
    big[lead:lead + n + 1].view(torch.float32).fill_(2.0)   # a ragged tail that stores one too many
    _guard.check_written(view)
    with pytest.raises(AssertionError, match=rf"past the window's {n} words: 1 word\(s\) at window offset {n} \.\. {n}"):
        _guard.check_guards(big, view, "out")


def test_write_one_float_before_the_start_is_reported():
    n = 37
    big, view = _guard.guarded(n, "cpu")
    lead = (view.data_ptr() - big.data_ptr()) // 4
    big[lead - 1:lead + n].view(torch.float32).fill_(2.0)
    with pytest.raises(AssertionError, match=r"out: .*before the window: 1 word\(s\) at window offset -1 \.\. -1"):
        _guard.check_guards(big, view, "out")


def test_a_whole_plane_overshoot_lands_in_the_guard_and_is_reported():
    n = 3000                                                   # larger than the minimum guard
    big, view = _guard.guarded(n, "cpu")
    lead = (view.data_ptr() - big.data_ptr()) // 4
    big[lead + n:lead + 2 * n].view(torch.float32).fill_(0.0)  # the wrong batch stride: one plane on
    with pytest.raises(AssertionError, match=rf"{n} word\(s\) at window offset {n} \.\. {2 * n - 1}"):
        _guard.check_guards(big, view)


def test_a_guard_word_rewritten_with_another_nan_is_reported():
    big, view = _guard.guarded(8, "cpu")
    lead = (view.data_ptr() - big.data_ptr()) // 4
    big[lead + 8 + 5] = 0x7FC00000                             # a NaN, but not the sentinel's bits
    with pytest.raises(AssertionError, match=r"window offset 13 \.\. 13"):
        _guard.check_guards(big, view)


def test_one_skipped_output_element_is_reported():
    big, view = _guard.guarded(37, "cpu")
    src = torch.arange(37, dtype=torch.float32)
    view[:20].copy_(src[:20])
    view[21:].copy_(src[21:])                                  # element 20 is never stored
    _guard.check_guards(big, view)
    with pytest.raises(AssertionError, match=r"dflow: not written, 1 word\(s\) at window offset 20 \.\. 20 of 37"):
        _guard.check_written(view, "dflow")


def test_float64_window():
    big, view = _guard.guarded(5, "cpu", dtype=torch.float64)
    view[:4] = 1.0
    with pytest.raises(AssertionError, match=r"1 word\(s\) at window offset 4 \.\. 4 of 5"):
        _guard.check_written(view)
    view[4] = 1.0
    _guard.check_written(view)
    _guard.check_guards(big, view)
    big[(view.data_ptr() - big.data_ptr()) // 8 + 5] = 0
    with pytest.raises(AssertionError, match=r"past the window's 5 words: 1 word\(s\) at window offset 5 \.\. 5"):
        _guard.check_guards(big, view)


def test_a_guard_word_multiplied_by_zero_reaches_the_result_and_is_reported():
    """A masked-by-multiply tail: the fake op reads one float past its input and gives it the
    weight 0.  With finite memory behind the input the answer is right; behind a guarded input it
    is NaN, which the comparison with the plain call and the payload check both report."""
    n = 16
    x = torch.arange(1, n + 1, dtype=torch.float32)
    w = torch.cat([torch.ones(n), torch.zeros(1)])

    def fake(buf, lead):                                       # sum_k w[k] * in[k] over n + 1 taps
        taps = buf[lead:lead + n + 1].view(torch.float32)
        return (taps * w).cumsum(0)[n - 1:]

    plain = torch.zeros(4 * n, dtype=torch.int32)
    plain[n:2 * n].view(torch.float32).copy_(x)
    ref = fake(plain, n)                                       # finite neighbours: the right answer
    assert float(ref[1]) == float(x.sum())

    big, view = _guard.guarded(n, "cpu")
    view.copy_(x)
    got = fake(big, (view.data_ptr() - big.data_ptr()) // 4)
    _guard.check_guards(big, view)                             # nothing was written out of bounds
    assert bit_equal(got[:1].numpy(), ref[:1].numpy())         # the in-bounds prefix is untouched
    assert not bit_equal(got.numpy(), ref.numpy())             # the NaN shows against the plain call
    assert _as_int(got)[1] & _guard.PAYLOAD_MASK == _guard.SENTINEL & _guard.PAYLOAD_MASK
    with pytest.raises(AssertionError, match=r"sentinel reached the result, 1 word\(s\) at window offset 1 \.\. 1"):
        _guard.check_clean(got, "out")


def test_check_clean_ignores_other_nans():
    t = torch.tensor([float("nan"), float("inf"), 0.0, 1.0])
    _guard.check_clean(t)
    assert _guard.carries_sentinel(t).numel() == 0
