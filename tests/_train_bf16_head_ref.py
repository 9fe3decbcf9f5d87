"""The test-side reference of the training steps' bf16 LM HEAD (``head_precision="bf16"``, ``r4d_set_train_head_bf16``;
tests/test_gpu_train_bf16_head.py, tests/test_host_train_bf16_head.py).  It extends tests/_train_bf16_ref.py (``R``) and
tests/_train_bf16_attn_ref.py (``A``) and modifies nothing of them.

"The emulation": the LM and generator step oracles of ``R`` (the calculus of ``R._step``, line by line) with the head
``logits = hidden . W^T`` computed by a ``torch.autograd.Function`` that does what the device's switched head does:

    forward   logits = bf16(h) . bf16(W)^T
    backward  dh = bf16(dlogits) . bf16(W),   dW = bf16(dlogits)^T . bf16(h)

with ONE FLAG PER PRODUCT, set as the library dispatches that product (``dispatched``).  The cross entropy and everything else
stay in the dtype of the leaves.  It composes with the layer and attention emulations: a mode is a ``precision`` of the
trainers, and the head patch is always on:

    "fp32"        the head alone
    "bf16+attn"   ``A.patched("bf16+attn")`` (layer GEMMs and attention products) and the head

Each case is run as in ``R``: "exact" (``R.references``: unpatched float64, shared), "emu64", "emu32".  Everything is computed once
per process and shared (callers must not modify it).

The generator cases carry one quantity more than in ``R``: "d_fused", the gradient of the spliced rows that
``r4d_rag_train_step_f32`` hands out (``d_fused_d``) -- the head's dh carried down through every block.  A frozen step has five
quantities in ``R``, and the head alone moves three of them (``hidden`` does not depend on the head at all, the loss moves by
1e-5): with d_fused there are four to gate.  Its exact value comes from this module's own unrounded float64 step.
``g10_trained-gen`` still gates three under the head alone (its lm_head.weight error stays below the floor) and is left to the
tables of ``R`` and ``A``: a gate with fewer than ``MIN_GATED`` quantities is none.
"""
import contextlib
import functools

import torch

import _train_bf16_attn_ref as A
import _train_bf16_ref as R

gpt2_ref, generator_ref = R.gpt2_ref, R.generator_ref
bf16_round = R.bf16_round
MODES = ("fp32", "bf16+attn")
MIN_GATED = 4
CE_CHUNK = 15872                      # r4d_lm_head_chunk_rows: one chunk up to this many padded rows, chunks of it beyond
# the steps with a head: the LM and generator cases of ``R`` but g10_trained-gen (the module's text says why)
CASES = [c for c in R.CASES if c.kind != "enc" and (c.weights, c.kind) != ("g10_trained", "gen")]


def padded_vocab(V):
    return (int(V) + 127) // 128 * 128


def chunks(ldV):
    C = ldV if ldV <= CE_CHUNK else CE_CHUNK
    return [(c0, min(C, ldV - c0)) for c0 in range(0, ldV, C)]


def _planes(M, K, N):                 # gemm_b1 (csrc/conv1d_route.h: gemm_planes_supported with 2 bytes per weight)
    return M >= 1 and K >= 32 and K % 32 == 0 and N >= 1 and N * K * 2 < 2 ** 31 and M * K < 2 ** 29 and 128 * N < 2 ** 29


def _b1tn(I, J, M):                   # gemm_b1tn (gemm_b1tn_supported with lda = I, ldb = J)
    return I >= 128 and I % 128 == 0 and J >= 256 and J % 256 == 0 and M >= 32 and (M + 64) * I < 2 ** 29 and (M + 64) * J < 2 ** 29


def dispatched(N, d, V, planes=True):
    """(logits, dh, dwte): which of the head's products the library sends to the bf16 kernels for N rows, width d and a
    vocabulary of V (include/r4d.h: r4d_set_train_head_bf16), per chunk -- and the fixtures' chunks all agree.  ``planes``: the
    head operand carries w3 / w3t (``HeadOperand`` builds them whenever d % 32 == 0)."""
    per = set()
    for _c0, cn in chunks(padded_vocab(V)):
        have = planes and d % 32 == 0
        per.add((have and _planes(N, d, cn), have and _planes(N, cn, d), _b1tn(cn, d, N)))
    assert len(per) == 1, per
    return per.pop()


class _HeadBf16(torch.autograd.Function):
    """logits [N, V] = h [N, d] . W [V, d]^T with the device's three products"""

    @staticmethod
    def forward(ctx, h, W, flags):
        ctx.save_for_backward(h, W)
        ctx.flags = flags
        return bf16_round(h) @ bf16_round(W).t() if flags[0] else h @ W.t()

    @staticmethod
    def backward(ctx, dl):
        h, W = ctx.saved_tensors
        _f, dgrad, wgrad = ctx.flags
        dh = dW = None
        if ctx.needs_input_grad[0]:
            dh = bf16_round(dl) @ bf16_round(W) if dgrad else dl @ W
        if ctx.needs_input_grad[1]:
            dW = bf16_round(dl).t() @ bf16_round(h) if wgrad else dl.t() @ h
        return dh, dW, None


def head(h, W, flags):
    return _HeadBf16.apply(h, W, flags)


def head_logits(hidden, W, rounded=True):
    """[B, T, d] -> [B, T, V]; the flags of the step's N = B T rows (``rounded`` False: no product is rounded)"""
    B, T, d = hidden.shape
    flags = dispatched(B * T, d, W.shape[0]) if rounded else (False, False, False)
    return head(hidden.reshape(B * T, d), W, flags).view(B, T, W.shape[0])


def _step(c, dtype, rounded=True):
    """``R._step`` for the kinds with a head, the transformer run without its logits and the head applied by ``head_logits``; the
    generator kinds also return grads["d_fused"] [B, 1, d]"""
    assert c.kind != "enc"
    sd, H = R.weights(c.weights)
    x = R.inputs(c)
    fwd = gpt2_ref.gpt2_forward.__wrapped__
    if c.kind == "lm":
        sdg = R._leaves(sd, dtype)
        hidden = fwd(sdg, x["ids"], H, want_logits=False)["hidden"]
        loss = gpt2_ref.lm_loss(head_logits(hidden, sdg["lm_head.weight"], rounded), x["ids"])
        loss.backward()
        return {"loss": float(loss.detach()), "grads": R._grads(sdg)}
    freeze = c.kind == "gen"
    sdg = R._leaves(sd, dtype, grad=not freeze)
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
    fused = torch.stack(rows)[:, None]
    fused.retain_grad()
    H_aug = torch.cat([Ht[:, :2], fused, Ht[:, 2:]], dim=1)
    hw = wte
    if freeze:
        hw = x["head"].detach().clone().to(dtype).requires_grad_(True)
    r = fwd(sdg, None, H, inputs_embeds=H_aug, want_logits=False)
    logits = head_logits(r["hidden"], hw, rounded)
    labels = torch.cat([tok[:, :2], torch.full((tok.shape[0], 1), -100), tok[:, 2:]], dim=1)
    lg = logits[:, :-1].reshape(-1, logits.shape[-1])
    loss = torch.nn.functional.cross_entropy(lg, labels[:, 1:].reshape(-1), ignore_index=-100)
    loss.backward()
    grads = {"gnn_fusion.convs.0.lin.weight": W.grad.double().numpy(), "gnn_fusion.convs.0.bias": b.grad.double().numpy(),
             "d_fused": fused.grad.double().numpy()}
    if freeze:
        grads["lm_head.weight"] = hw.grad.double().numpy()
    else:
        grads.update(R._grads(sdg))
    return {"loss": float(loss.detach()), "grads": grads, "hidden": r["hidden"].detach().double().numpy()}


@contextlib.contextmanager
def patched(mode, M):
    """The layer / attention emulation that goes with the head under ``precision`` = mode"""
    assert mode in MODES, mode
    with contextlib.ExitStack() as st:
        if mode != "fp32":
            st.enter_context(A.patched(mode, M))
        yield


@functools.lru_cache(maxsize=None)
def exact_of(c):
    """``R``'s exact oracle of a case (its arrays are the same objects); the generator kinds with "d_fused" beside its gradients,
    from this module's unrounded float64 step -- which must reproduce ``R``'s loss and gradients"""
    exact = R.references(c)[0]
    if c.kind == "lm":
        return exact
    mine = _step(c, torch.float64, rounded=False)
    assert abs(mine["loss"] - exact["loss"]) <= 1e-12 * abs(exact["loss"])
    for n, g in exact["grads"].items():
        assert R.rel(mine["grads"][n], g) <= 1e-10, n
    out = dict(exact)
    out["grads"] = dict(exact["grads"], d_fused=mine["grads"]["d_fused"])
    return out


@functools.lru_cache(maxsize=None)
def references(c, mode):
    """-> (exact, emu64, emu32) of a case; exact is ``exact_of``"""
    exact = exact_of(c)
    with patched(mode, R.rows_of(c)):
        e64, e32 = _step(c, torch.float64), _step(c, torch.float32)
    return exact, e64, e32


@functools.lru_cache(maxsize=None)
def error_table(c, mode):
    """name -> dict(emu64, emu32, ratio), as ``A.error_table``"""
    exact, e64, e32 = references(c, mode)
    a, b = R.errors(e64, exact), R.errors(e32, exact)
    out = {}
    for n in a:
        x, y = max(a[n], R.RATIO_FLOOR), max(b[n], R.RATIO_FLOOR)
        out[n] = dict(emu64=a[n], emu32=b[n], ratio=max(x / y, y / x))
    return out


def gated(c, mode):
    """name -> emu64 of the gated quantities of a case (``A``'s rule: the arithmetic's own error reaches ``R.GATE_FLOOR``)"""
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
    """K of the gate: 2 x the largest ratio over all cases, never below 2 (``A.margin``'s rule)"""
    return max(2.0, 2.0 * max(worst_ratio(c, mode)[0] for c in CASES))


def format_table(mode):
    lines = [f"[head bf16, precision {mode}] case | gated quantities | e_emu64 min .. max | worst ratio (quantity) | loss emu64 / emu32"]
    for c in CASES:
        t = error_table(c, mode)
        g = list(gated(c, mode).values())
        r, n = worst_ratio(c, mode)
        lines.append(f"{R.case_id(c)} | {len(g)} of {len(t)} | {min(g):.1e} .. {max(g):.1e} | {r:.2f} ({n}) | "
                     f"{t['loss']['emu64']:.1e} / {t['loss']['emu32']:.1e}")
    lines.append(f"K = {margin(mode):.2f}")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------- the head alone
def head_alone(h, W, labels_src, T, dtype, flags):
    """The head entry's calculus on the CPU: h [N, d], W [V, d], labels_src int64 [N] (the label of row r is labels_src[r + 1]
    inside a sequence of T rows, -100 not counted) -> dict(loss, dh, dW) as float64 numpy.  flags None: exact (no rounding)."""
    N, _d = h.shape
    hl = h.detach().clone().to(dtype).requires_grad_(True)
    Wl = W.detach().clone().to(dtype).requires_grad_(True)
    logits = head(hl, Wl, flags) if flags is not None else hl @ Wl.t()
    lab = torch.full((N,), -100, dtype=torch.int64)
    src = labels_src.view(N // T, T)
    lab.view(N // T, T)[:, :-1] = src[:, 1:]
    loss = torch.nn.functional.cross_entropy(logits, lab, ignore_index=-100)
    loss.backward()
    return {"loss": float(loss.detach()), "dh": hl.grad.double().numpy(), "dW": Wl.grad.double().numpy()}
