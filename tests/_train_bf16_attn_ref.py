"""The test-side reference of the training steps' bf16 ATTENTION products (the ``+attn`` precisions;
tests/test_gpu_train_bf16_attn.py, tests/test_host_train_bf16_attn.py).  It extends tests/_train_bf16_ref.py (``R``) and modifies
nothing of it.

"The emulation": the step oracles of ``R`` with ``gpt2_ref.attn_core`` replaced, while a context manager is active, by the same
function with both of its ``matmul``s going through a ``torch.autograd.Function`` that computes what the device's switched
products compute:

    forward   c = bf16(a) . bf16(b)
    backward  da = bf16(dc) . bf16(b)^T,   db = bf16(a)^T . bf16(dc)

The scale division, the mask, the softmax and the dropout stay in the dtype of the leaves.  Two modes:

    "bf16+attn"   that patch together with ``R.patched_conv1d`` (the layer GEMMs of precision "bf16")
    "fp32+attn"   that patch alone

Each case of ``R.CASES`` is run as in ``R``: "exact" (``R.references``: unpatched float64, shared), "emu64", "emu32".  Everything is
computed once per process and shared (callers must not modify it).
"""
import contextlib
import functools
import math

import torch

import _train_bf16_ref as R

gpt2_ref = R.gpt2_ref
bf16_round = R.bf16_round
MODES = ("bf16+attn", "fp32+attn")
MIN_GATED = 4                          # every case must gate at least this many quantities: a gate that gates nothing passes anything


class _ProductBf16(torch.autograd.Function):
    """c [..., M, N] = bf16(a [..., M, K]) @ bf16(b [..., K, N]) with the device's three backward products"""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return torch.matmul(bf16_round(a), bf16_round(b))

    @staticmethod
    def backward(ctx, dc):
        a, b = ctx.saved_tensors
        da = db = None
        if ctx.needs_input_grad[0]:
            da = torch.matmul(bf16_round(dc), bf16_round(b).transpose(-1, -2))
        if ctx.needs_input_grad[1]:
            db = torch.matmul(bf16_round(a).transpose(-1, -2), bf16_round(dc))
        return da, db


def product(a, b):
    return _ProductBf16.apply(a, b)


def attn_core_bf16(q, k, v, drop=None):
    """``gpt2_ref.attn_core`` line by line, with ``product`` for its two ``torch.matmul``s"""
    w = product(q, k)
    w = w / math.sqrt(v.size(-1))
    nd, ns = w.size(-2), w.size(-1)
    b = torch.tril(torch.ones(ns, ns, dtype=w.dtype))[ns - nd:ns, :ns].view(1, 1, nd, ns)
    w = w * b - 1e4 * (1 - b)
    w = torch.softmax(w, dim=-1)
    if drop is not None:
        w = drop(w)
    return product(w, v)


@contextlib.contextmanager
def patched_attention():
    orig = gpt2_ref.attn_core
    gpt2_ref.attn_core = attn_core_bf16
    try:
        yield
    finally:
        gpt2_ref.attn_core = orig


@contextlib.contextmanager
def patched(mode, M):
    """The emulation of ``mode`` for a step of M rows (``R.patched_conv1d`` wants them)"""
    assert mode in MODES, mode
    with contextlib.ExitStack() as st:
        if mode == "bf16+attn":
            st.enter_context(R.patched_conv1d(M))
        st.enter_context(patched_attention())
        yield


@functools.lru_cache(maxsize=None)
def references(c, mode):
    """-> (exact, emu64, emu32) of a case; exact is ``R``'s own (the same object)"""
    exact = R.references(c)[0]
    with patched(mode, R.rows_of(c)):
        e64, e32 = R._step(c, torch.float64), R._step(c, torch.float32)
    return exact, e64, e32


@functools.lru_cache(maxsize=None)
def error_table(c, mode):
    """name -> dict(emu64, emu32, ratio), as ``R.error_table``"""
    exact, e64, e32 = references(c, mode)
    a, b = R.errors(e64, exact), R.errors(e32, exact)
    out = {}
    for n in a:
        x, y = max(a[n], R.RATIO_FLOOR), max(b[n], R.RATIO_FLOOR)
        out[n] = dict(emu64=a[n], emu32=b[n], ratio=max(x / y, y / x))
    return out


def gated(c, mode):
    """name -> emu64 of the gated quantities of a case"""
    return {n: v["emu64"] for n, v in error_table(c, mode).items() if v["emu64"] >= R.GATE_FLOOR}


def worst_ratio(c, mode):
    t = error_table(c, mode)
    g = {n: t[n]["ratio"] for n in gated(c, mode)}
    if not g:
        return 1.0, None
    n = max(g, key=g.get)
    return g[n], n


@functools.lru_cache(maxsize=None)
def margin(mode):
    """K of the gate: 2 x the largest ratio over all cases, never below 2 (as ``R.margin``)"""
    return max(2.0, 2.0 * max(worst_ratio(c, mode)[0] for c in R.CASES))


def format_table(mode):
    lines = [f"[{mode}] case | gated quantities | e_emu64 min .. max | worst ratio (quantity) | loss emu64 / emu32"]
    for c in R.CASES:
        t = error_table(c, mode)
        g = list(gated(c, mode).values())
        r, n = worst_ratio(c, mode)
        lines.append(f"{R.case_id(c)} | {len(g)} of {len(t)} | {min(g):.1e} .. {max(g):.1e} | {r:.2f} ({n}) | "
                     f"{t['loss']['emu64']:.1e} / {t['loss']['emu32']:.1e}")
    lines.append(f"K = {margin(mode):.2f}")
    return "\n".join(lines)
