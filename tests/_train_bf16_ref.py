"""The test-side reference of the training steps' opt-in bf16 precision (tests/test_gpu_train_bf16.py,
tests/test_host_train_bf16.py).

"The emulation": the step oracles (the calculus of tests/_training_stress_cases.py::oracle) with ``gpt2_ref.conv1d`` replaced, while
a context manager is active, by a ``torch.autograd.Function`` that computes what the device's switched GEMMs compute:

    forward   addmm(b, bf16(x), bf16(W))
    backward  dx = bf16(dy) . bf16(W)^T,   dW = bf16(x)^T . bf16(dy),   db = dy.sum(0)   (the UNROUNDED dy)

with ONE FLAG PER PRODUCT, set as the library dispatches that product (``dispatched``): a weight gradient whose shape the TN
kernel does not take (d 64: every one of them) stays exact in the emulation as it stays on the default kernel on the device.
Everything else (LayerNorm, attention, gelu_new, the residual adds, the LM head, the GCN projection, the loss) stays in the dtype
of the leaves.  Each step is run three times: "exact" (unpatched, float64), "emu64" (emulated, float64: the arithmetic's own
error), "emu32" (emulated, float32: a second legitimate rounding of the same step).

Fixtures, references and tables are computed once per process and shared (callers must not modify them).
"""
import contextlib
import functools
import os
import sys
from collections import namedtuple

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import _encode_bf16_ref as E  # noqa: E402
from oracle import generator_ref, gpt2_ref  # noqa: E402

bf16_round = E.bf16_round


def dispatched(M, K, N):
    """(forward, data gradient, weight gradient) of a Conv1D [K, N] over M rows: which products the library sends to the bf16
    kernels (include/r4d.h: r4d_set_train_bf16).  Every layer of the fixtures carries its planes (K % 32 == 0 and N % 32 == 0)."""
    planes = K % 32 == 0 and N % 32 == 0
    return (planes, planes, K % 128 == 0 and N % 256 == 0 and M >= 32)


class _Conv1DBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2, weight, bias, flags):
        ctx.save_for_backward(x2, weight)
        ctx.flags = flags
        return torch.addmm(bias, bf16_round(x2), bf16_round(weight)) if flags[0] else torch.addmm(bias, x2, weight)

    @staticmethod
    def backward(ctx, dy):
        x2, weight = ctx.saved_tensors
        _f, dgrad, wgrad = ctx.flags
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = bf16_round(dy) @ bf16_round(weight).t() if dgrad else dy @ weight.t()
        if ctx.needs_input_grad[1]:
            dw = bf16_round(x2).t() @ bf16_round(dy) if wgrad else x2.t() @ dy
        if ctx.needs_input_grad[2]:
            db = dy.sum(0)
        return dx, dw, db, None


@contextlib.contextmanager
def patched_conv1d(M):
    """``M``: the rows of the step's launch sequence (all groups of an enc step form ONE sequence on the device, so the weight
    gradient's M >= 32 condition is about their sum, whatever rows one oracle call sees)."""
    orig = gpt2_ref.conv1d

    def conv1d(x, weight, bias):
        x2 = x.reshape(-1, x.shape[-1])
        y = _Conv1DBf16.apply(x2, weight, bias, dispatched(M, weight.shape[0], weight.shape[1]))
        return y.view(x.shape[:-1] + (weight.shape[1],))
    gpt2_ref.conv1d = conv1d
    try:
        yield
    finally:
        gpt2_ref.conv1d = orig


# ------------------------------------------------------------------------------------------------------------------ the cases
# weights: a fixture of _encode_bf16_ref (plain weight sets).  Bs / Ts as in _training_stress_cases.Entry: for gen* T is the
# length the transformer sees (tokens + the one fused row).
Case = namedtuple("Case", "weights kind Bs Ts")
WEIGHTS = ("L2_d64_T40", "L2_d256_T130", "L4_d512_T96", "g10_trained")
ENC_BS, ENC_TS = (2, 3, 1), (40, 17, 130)
KINDS = ("enc", "lm", "gen", "gen_tied")


def case(weights, kind):
    if kind == "enc":
        return Case(weights, kind, ENC_BS, ENC_TS)
    T = E.SEEDED[weights][6] if weights in E.SEEDED else 48
    return Case(weights, kind, (3,), (T,))


CASES = [case(w, k) for w in WEIGHTS for k in KINDS]
# Fixtures whose cases are GATED (the others are recorded): every plain weight set stays inside K <= 4 (profiles/train_bf16.md has
# the table test_host_train_bf16.py prints)
GATED = WEIGHTS


def case_id(c):
    return f"{c.weights}-{c.kind}"


def rows_of(c):
    return sum(b * t for b, t in zip(c.Bs, c.Ts))


def weights(name):
    """-> (state dict, H)"""
    sd, _L, H = E.fixture(name)[:3]
    return sd, H


def _ids(V, B, T, seed):
    """Random ids over V - 2 tokens, rows 1.. right-padded with V - 1 (as the ``_ids`` helpers of the step tests)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V - 2, (B, T), generator=g)
    for i in range(1, B):
        lo = min(max(3, T // 2), T)
        n = int(torch.randint(lo, T + 1, (1,), generator=g))
        ids[i, n:] = V - 1
    return ids


@functools.lru_cache(maxsize=None)
def inputs(c):
    """Everything one case's step needs beside the weights, as CPU tensors / lists (deterministic in the case)."""
    sd, _H = weights(c.weights)
    V, d = sd["transformer.wte.weight"].shape
    seed = 1000 * len(c.Ts) + sum(c.Ts) + 7 * sum(c.Bs) + d
    g = torch.Generator().manual_seed(seed + 1)
    if c.kind == "enc":
        ids = [_ids(V, B, T, seed + 10 * j) for j, (B, T) in enumerate(zip(c.Bs, c.Ts))]
        return {"ids": ids, "G": torch.randn(sum(c.Bs), d, generator=g)}
    if c.kind == "lm":
        return {"ids": _ids(V, c.Bs[0], c.Ts[0], seed)}
    B, T = c.Bs[0], c.Ts[0] - 1
    rng = np.random.default_rng(seed)
    src = [rng.integers(0, V - 2, int(rng.integers(5, 16))).tolist() for _ in range(40)]
    idx = [rng.choice(40, 7, replace=False).tolist() for _ in range(B)]
    out = {"tok": _ids(V, B, T, seed), "idx": idx, "src": src,
           "gcn_w": torch.randn(d, d, generator=g) * 0.05, "gcn_b": torch.randn(d, generator=g) * 0.05}
    if c.kind == "gen":
        out["head"] = torch.randn(V, d, generator=g) * 0.05               # the untied head of load_and_freeze_params
    return out


def _leaves(sd, dtype, grad=True):
    sdg = {k: v.detach().clone().to(dtype).requires_grad_(grad) for k, v in sd.items() if k != "lm_head.weight"}
    sdg["lm_head.weight"] = sdg["transformer.wte.weight"]
    return sdg


def _grads(sdg):
    return {k: v.grad.double().numpy() for k, v in sdg.items() if k != "lm_head.weight"}


def _step(c, dtype):
    """One case's step in ``dtype`` on the CPU (the calculus of _training_stress_cases.oracle): {"loss", "grads" (name -> float64
    numpy), "emb" / "hidden" where the device hands them out}."""
    sd, H = weights(c.weights)
    x = inputs(c)
    fwd = gpt2_ref.gpt2_forward.__wrapped__                                 # grad-enabled
    if c.kind == "enc":
        sdg = _leaves(sd, dtype)
        emb = torch.cat([fwd(sdg, ids, H, want_logits=False)["hidden"].mean(dim=1) for ids in x["ids"]])
        loss = (emb * x["G"].to(dtype)).sum()
        loss.backward()
        return {"loss": float(loss.detach()), "grads": _grads(sdg), "emb": emb.detach().double().numpy()}
    if c.kind == "lm":
        sdg = _leaves(sd, dtype)
        loss = gpt2_ref.lm_loss(fwd(sdg, x["ids"], H, want_logits=True)["logits"], x["ids"])
        loss.backward()
        return {"loss": float(loss.detach()), "grads": _grads(sdg)}
    freeze = c.kind == "gen"
    sdg = _leaves(sd, dtype, grad=not freeze)
    W = x["gcn_w"].detach().clone().to(dtype).requires_grad_(True)
    b = x["gcn_b"].detach().clone().to(dtype).requires_grad_(True)
    wte = sdg["transformer.wte.weight"]
    tok = x["tok"]
    rows = []
    for ix in x["idx"]:
        order, edges = generator_ref.star_union_graph(x["src"], ix[:7])
        a = generator_ref.gcn_norm_dense(len(order), edges).to(dtype)
        rows.append(generator_ref.gcn_conv(wte[torch.tensor(order)], a, W, b).mean(dim=0))
    Ht = wte[tok]
    H_aug = torch.cat([Ht[:, :2], torch.stack(rows)[:, None], Ht[:, 2:]], dim=1)
    head = None
    if freeze:
        head = x["head"].detach().clone().to(dtype).requires_grad_(True)
        sdg["lm_head.weight"] = head
    r = fwd(sdg, None, H, inputs_embeds=H_aug, want_logits=True)
    labels = torch.cat([tok[:, :2], torch.full((tok.shape[0], 1), -100), tok[:, 2:]], dim=1)
    lg = r["logits"][:, :-1].reshape(-1, r["logits"].shape[-1])
    loss = torch.nn.functional.cross_entropy(lg, labels[:, 1:].reshape(-1), ignore_index=-100)
    loss.backward()
    grads = {"gnn_fusion.convs.0.lin.weight": W.grad.double().numpy(), "gnn_fusion.convs.0.bias": b.grad.double().numpy()}
    if freeze:
        grads["lm_head.weight"] = head.grad.double().numpy()
    else:
        grads.update(_grads(sdg))
    return {"loss": float(loss.detach()), "grads": grads, "hidden": r["hidden"].detach().double().numpy()}


@functools.lru_cache(maxsize=None)
def references(c):
    """-> (exact, emu64, emu32) of a case"""
    exact = _step(c, torch.float64)
    with patched_conv1d(rows_of(c)):
        e64, e32 = _step(c, torch.float64), _step(c, torch.float32)
    return exact, e64, e32


def rel(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def errors(got, exact):
    """name -> max|g - g_exact| / max|g_exact| over the gradients, plus "loss", "emb", "hidden" where both sides carry them"""
    e = {n: rel(got["grads"][n], exact["grads"][n]) for n in exact["grads"]}
    for k in ("loss", "emb", "hidden"):
        if exact.get(k) is not None and got.get(k) is not None:
            e[k] = rel(got[k], exact[k])
    return e


GATE_FLOOR = 1e-4                     # a quantity is gated where the arithmetic's own error (emu64) reaches this
RATIO_FLOOR = 1e-6


@functools.lru_cache(maxsize=None)
def error_table(c):
    """name -> dict(emu64, emu32, ratio = max(emu32 / emu64, emu64 / emu32), both floored at RATIO_FLOOR)"""
    exact, e64, e32 = references(c)
    a, b = errors(e64, exact), errors(e32, exact)
    out = {}
    for n in a:
        x, y = max(a[n], RATIO_FLOOR), max(b[n], RATIO_FLOOR)
        out[n] = dict(emu64=a[n], emu32=b[n], ratio=max(x / y, y / x))
    return out


def worst_ratio(c):
    """(largest ratio over the GATED quantities of a case, its name)"""
    t = error_table(c)
    gated = {n: v["ratio"] for n, v in t.items() if v["emu64"] >= GATE_FLOOR}
    if not gated:
        return 1.0, None
    n = max(gated, key=gated.get)
    return gated[n], n


@functools.lru_cache(maxsize=None)
def margin():
    """K of the gate: 2 x the largest ratio over the gated fixtures' cases, never below 2 (the encode test's factor)"""
    return max(2.0, 2.0 * max(worst_ratio(c)[0] for c in CASES if c.weights in GATED))


def format_table():
    lines = ["case | gated quantities | e_emu64 min .. max | worst ratio (quantity) | loss emu64 / emu32"]
    for c in CASES:
        t = error_table(c)
        g = [v["emu64"] for v in t.values() if v["emu64"] >= GATE_FLOOR]
        r, n = worst_ratio(c)
        lines.append(f"{case_id(c)} | {len(g)} of {len(t)} | {min(g):.1e} .. {max(g):.1e} | {r:.2f} ({n}) | "
                     f"{t['loss']['emu64']:.1e} / {t['loss']['emu32']:.1e}" + ("" if c.weights in GATED else " | recorded, not gated"))
    lines.append(f"K = {margin():.2f}")
    return "\n".join(lines)
