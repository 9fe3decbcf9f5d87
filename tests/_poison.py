"""Poisoned memory for the workspace tests (tests/test_gpu_workspace_poison.py, tests/test_host_workspace_poison.py).

Every entry point of the library works in memory the caller hands it -- workspaces, output tensors, the key/value cache, the
gradient buffer, the derived weight copies -- and on the Python side all of it comes from ``torch.empty``.  The library is
correct only if each call writes every byte it later reads (include/r4d.h, "What a buffer may hold on entry").  In a fresh
process the caching allocator mostly hands out zeroed pages or the previous call's identical values, so a read of unwritten
memory stays invisible; these helpers make the content of such memory a test parameter instead.

``poisoned_allocations(pattern)`` covers the FIRST allocation of a buffer (while it is active ``torch.empty``,
``torch.empty_like`` and ``Tensor.new_empty`` return memory filled with the pattern; the library's Python side looks these up at
call time), ``poison(tensor, pattern)`` the REUSE of a buffer that already exists (the entries of ``ops._WS``, a trainer's
``_ws``, ``flat_grads``, a key/value cache, the greedy decoder's ``ws`` and ``logits``).

Patterns (bytes, so one pattern serves every dtype):

    ZERO   zero bytes                the baseline
    NAN    0xFF bytes                NaN as f32, f64 and f16; -1 as an integer; a saturated counter
    HUGE   0x7F bytes                3.4e38 as f32, finite as f64; a large positive counter -- a NaN is invisible to fmaxf /
                                     fminf, to ``<``, to an absmax pre-pass and to the top-k keys; this one is not
    ONE    every 32-bit word = 1     a denormal as a float; a small valid index; a non-zero counter

NAN and HUGE may only go into memory none of whose words is ever used to form an address, a loop bound or a length (the GPU
test module's docstring classifies every workspace); ZERO and ONE may go anywhere.
"""
import contextlib

import torch

ZERO, NAN, HUGE, ONE = "zero", "nan", "huge", "one"
PATTERNS = (ZERO, NAN, HUGE, ONE)
_BYTE = {ZERO: 0x00, NAN: 0xFF, HUGE: 0x7F}
_EMPTY = torch.empty                      # the original: the helper's own zero-size handle never goes through the wrapper


def _fill_bytes(b, pattern):
    """``b``: a 1-D uint8 tensor.  ONE counts its 32-bit words from the first byte (little endian: 01 00 00 00), so a byte count
    that is no multiple of 4 ends in a cut-off word."""
    if pattern == ONE:
        b.zero_()
        b[0::4] = 1
    elif pattern in _BYTE:
        b.fill_(_BYTE[pattern])
    else:
        raise ValueError(f"poison pattern {pattern!r}: one of {PATTERNS}")


def poison(tensor, pattern):
    """Refill an existing buffer (a contiguous tensor or contiguous view, e.g. a slice of the flat gradient buffer) with
    ``pattern``; only the tensor's own bytes are touched.  Returns the tensor."""
    if tensor is None or tensor.numel() == 0:
        return tensor
    if not tensor.is_contiguous():
        raise ValueError("poison: the buffer must be contiguous")
    _fill_bytes(tensor.detach().reshape(-1).view(torch.uint8), pattern)
    return tensor


def _poison_fresh(t, pattern):
    """A tensor that ``torch.empty`` has just returned owns its whole storage: fill all of it (whatever its strides)."""
    if not isinstance(t, torch.Tensor) or t.device.type == "meta" or t.is_sparse or t.untyped_storage().nbytes() == 0:
        return t
    if t.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("poisoned_allocations: an allocation during HIP graph capture (allocate before the capture)")
    _fill_bytes(_EMPTY(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage()), pattern)
    return t


@contextlib.contextmanager
def poisoned_allocations(pattern):
    """While active, ``torch.empty``, ``torch.empty_like`` and ``Tensor.new_empty`` return memory filled with ``pattern``.  The
    originals are back on exit, also after an exception.  Not to be active while a HIP graph is captured (a fill is a launch)."""
    if pattern not in PATTERNS:
        raise ValueError(f"poison pattern {pattern!r}: one of {PATTERNS}")
    saved = (torch.empty, torch.empty_like, torch.Tensor.new_empty)

    def wrap(fn):
        def poisoned(*args, **kwargs):
            return _poison_fresh(fn(*args, **kwargs), pattern)
        poisoned.__wrapped__ = fn
        return poisoned

    torch.empty, torch.empty_like, torch.Tensor.new_empty = wrap(saved[0]), wrap(saved[1]), wrap(saved[2])
    try:
        yield
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = saved
