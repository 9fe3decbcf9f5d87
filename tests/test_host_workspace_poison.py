"""CPU tests of the poisoning helper (tests/_poison.py) the GPU workspace tests stand on: every pattern in every dtype the library
allocates, the restored allocators, and the ONE pattern on a byte count that is no multiple of 4."""
import numpy as np
import pytest
import torch

import _poison
from _poison import HUGE, NAN, ONE, PATTERNS, ZERO, poison, poisoned_allocations

DTYPES = [torch.uint8, torch.int16, torch.int32, torch.int64, torch.float32, torch.float64]


def _raw(t):
    return t.reshape(-1).view(torch.uint8).numpy()


def _expected_bytes(n, pattern):
    if pattern == ONE:
        b = np.zeros(n, dtype=np.uint8)
        b[0::4] = 1
        return b
    return np.full(n, {ZERO: 0x00, NAN: 0xFF, HUGE: 0x7F}[pattern], dtype=np.uint8)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[1] for d in DTYPES])
def test_both_helpers_fill_every_dtype_with_the_pattern(dtype, pattern):
    with poisoned_allocations(pattern):
        fresh = [torch.empty(3, 5, dtype=dtype), torch.empty((), dtype=dtype), torch.empty_like(torch.zeros(7, dtype=dtype)),
                 torch.zeros(2, dtype=torch.float32).new_empty((4, 3), dtype=dtype), torch.empty(0, dtype=dtype)]
    reused = [poison(torch.zeros(3, 5, dtype=dtype), pattern), poison(torch.zeros((), dtype=dtype), pattern)]
    for t in fresh + reused:
        assert t.dtype == dtype
        assert np.array_equal(_raw(t), _expected_bytes(t.numel() * t.element_size(), pattern)), (tuple(t.shape), pattern)


def test_the_patterns_mean_what_the_gpu_tests_take_them_for():
    f32 = {p: poison(torch.zeros(4), p) for p in PATTERNS}
    f64 = {p: poison(torch.zeros(4, dtype=torch.float64), p) for p in PATTERNS}
    i32 = {p: poison(torch.zeros(4, dtype=torch.int32), p) for p in PATTERNS}
    f16 = poison(torch.zeros(4, dtype=torch.float16), NAN)
    assert torch.isnan(f32[NAN]).all() and torch.isnan(f64[NAN]).all() and torch.isnan(f16).all() and (i32[NAN] == -1).all()
    assert (f32[HUGE] > 3.3e38).all() and torch.isfinite(f32[HUGE]).all() and torch.isfinite(f64[HUGE]).all()
    assert (i32[HUGE] == 0x7F7F7F7F).all()
    assert (i32[ONE] == 1).all() and (f32[ONE] > 0).all() and (f32[ONE] < 1e-44).all()
    assert (f32[ZERO] == 0).all() and (i32[ZERO] == 0).all()
    assert (poison(torch.zeros(3, dtype=torch.int64), ONE) == (1 << 32) + 1).all()


@pytest.mark.parametrize("nbytes", [1, 2, 3, 5, 6, 7, 4099])
def test_one_handles_a_byte_count_that_is_no_multiple_of_four(nbytes):
    with poisoned_allocations(ONE):
        a = torch.empty(nbytes, dtype=torch.uint8)
    b = poison(torch.full((nbytes,), 9, dtype=torch.uint8), ONE)
    for t in (a, b):
        assert np.array_equal(t.numpy(), _expected_bytes(nbytes, ONE))
    if nbytes == 6:                                                   # int16 x 3: one whole word and a cut-off one
        assert poison(torch.zeros(3, dtype=torch.int16), ONE).tolist() == [1, 0, 1]


def test_a_view_is_refilled_without_touching_its_neighbours():
    flat = torch.zeros(64)
    poison(flat[8:24].view(4, 4), NAN)
    assert torch.isnan(flat[8:24]).all() and (flat[:8] == 0).all() and (flat[24:] == 0).all()
    with pytest.raises(ValueError):
        poison(torch.zeros(4, 4).t(), NAN)
    with pytest.raises(ValueError):
        poison(torch.zeros(4), "garbage")


def test_the_allocators_are_restored_after_normal_exit_and_after_an_exception():
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    assert _poison._EMPTY is before[0]
    with poisoned_allocations(NAN):
        assert torch.empty is not before[0] and torch.empty_like is not before[1] and torch.Tensor.new_empty is not before[2]
        assert torch.isnan(torch.empty(5)).all()
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
    with pytest.raises(KeyError):
        with poisoned_allocations(HUGE):
            assert (torch.empty(5) > 3.3e38).all()
            raise KeyError("inside")
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
    with pytest.raises(ValueError):
        with poisoned_allocations("garbage"):
            pass
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
    with poisoned_allocations(ONE):                                    # nesting: the inner pattern inside, the outer one after it
        with poisoned_allocations(NAN):
            assert torch.isnan(torch.empty(3)).all()
        assert (torch.empty(3, dtype=torch.int32) == 1).all()
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
