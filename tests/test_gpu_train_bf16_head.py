"""The training steps' opt-in bf16 LM head on the GPU (``head_precision="bf16"`` of the LM and generator trainers,
``r4d_set_train_head_bf16``, csrc/lm_head.hip on gemm_b1 / gemm_b1tn): the head alone through ``r4d_lm_head_train_f32`` against
float64 of the device's own rounded operands at a derived bound and against the exact head inside the emulations' margin, what it
writes, its counters, its fallbacks; the steps against the EXACT float64 oracle inside the margins of
tests/_train_bf16_head_ref.py; the chunked head inside a step; the independence of the three switches; a short training run.

The step helpers (``model_of``, ``snapshot`` ...) are those of tests/test_gpu_train_bf16.py.  Every test restores the switches it
found."""
import math

import pytest
import torch

import _train_modes
import _train_bf16_head_ref as Hd
import _train_bf16_ref as R
import test_gpu_train_bf16 as TB
from _poison import HUGE, NAN, ONE, ZERO, poison

pytestmark = pytest.mark.gpu

HEAD_PREFIX = "tuning:train_head_bf16:"
NO_HITS = {"logits": 0, "dgrad": 0, "wgrad": 0, "wgrad_fallback": 0}
SENTINEL = -7777.25
GUARD = 64
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


restore_switches = _train_modes.switches_restored(ops_too=True)


def head_hits():
    return TB.hits(HEAD_PREFIX)


def head_delta(before):
    return {n: v - before[n] for n, v in head_hits().items()}


# ------------------------------------------------------------------------------------------------------------- 1. the head alone
# (d, V, B, T).  d 64: the planes are there, gemm_b1tn refuses d % 256 -> the weight gradient ALONE falls back.  V 100 -> ldV 128 (one
# tile, 28 pad rows), 300 -> 384, 15,900 -> 16,000 = two chunks of 15,872 + 128 (the shortest a chunk can be; small N only).
# N = B T: 31 (below gemm_b1tn's 32 rows: fallback), 32, 130 (a clamped row tile), 2 x 65.
HEAD_SHAPES = [(256, 100, 1, 31), (256, 100, 2, 16), (256, 100, 1, 130), (256, 100, 2, 65), (256, 300, 1, 31), (256, 300, 2, 16),
               (256, 300, 2, 65), (256, 15900, 2, 16), (64, 100, 2, 16), (64, 300, 2, 65), (64, 15900, 2, 16)]


class Guarded:
    """[rows, cols] fp32 inside a flat buffer with GUARD sentinel floats on both sides"""

    def __init__(self, dev, rows, cols):
        self.raw = torch.full((GUARD + rows * cols + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        self.body = self.raw[GUARD:GUARD + rows * cols].view(rows, cols)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == SENTINEL).all()) and bool((self.raw[-GUARD:] == SENTINEL).all())


def head_inputs(dev, d, V, B, T):
    """h, W and the label source.  Row (b, t) is labelled by src[b, t + 1]; -100 (not counted) sits in a few rows of sequence 0
    and, where there is a second sequence, in ALL of it -- with one sequence that would leave nothing to count (a NaN loss, as
    torch), so the one-sequence shapes carry the -100 rows only."""
    g = torch.Generator().manual_seed(7 * d + V + 100 * B + T)
    N = B * T
    h = torch.randn(N, d, generator=g)
    W = torch.randn(V, d, generator=g) * 0.05
    src = torch.randint(0, V, (B, T), generator=g)
    src[0, 3::7] = -100
    if B > 1:
        src[1, :] = -100
    return h, W, src.reshape(-1)


def head_operand(dev, V, d, W):
    from rag4dyg_amd import ops
    from rag4dyg_amd.lm_training import HeadOperand
    op = HeadOperand(V, d, dev, ops.gemm_split3_enabled(), ops.gemm_mode() == "f16x2", head_bf16=True)
    op.refresh(W.to(dev))
    torch.cuda.synchronize()
    return op


def rn(x):
    return x.bfloat16().double()


def ce64(logits, lab):
    """float64 shifted cross entropy of [N, V] logits under labels [N] (-100 not counted) -> (loss, dlogits [N, V])"""
    lg = logits.detach().clone().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(lg, lab, ignore_index=-100)
    loss.backward()
    return float(loss.detach()), lg.grad


def labels_of(src, B, T):
    lab = torch.full((B, T), -100, dtype=torch.int64)
    lab[:, :-1] = src.view(B, T)[:, 1:]
    return lab.reshape(-1)


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=["d{}V{}B{}T{}".format(*s) for s in HEAD_SHAPES])
def test_01_the_head_alone(dev, shape):
    """With u = 2^-24 and every sum taken over the contraction index:
      * dh within (ldV + 2) u sum |RN dl| |RN W| of the float64 product of the DEVICE's rounded dlogits (the workspace begins with the
        last chunk's dlogits [N, Ck]: all of them in the one-chunk head) and the rounded table; dwte within (N + 2) u sum |RN dl|
        |RN h| likewise (the chunked head: the rows of its last chunk) -- bf16 x bf16 is exact in fp32, the roundings are the
        accumulation's (and the slices' sum's);
      * the loss within 2 max(logit bound) + 64 u (max |logit| + ln V + 1) of the float64 cross entropy of RN(h) . RN(W)^T: a row's
        term is 1-Lipschitz in each of the two places the logits enter it, the rest is the fp32 evaluation of exp, sum, log and the
        mean over the rows;
      * every product that took the bf16 route is NOT the product of the unrounded operands: at least one element of dh / dwte lies
        further than its bound from it, and for the logits (which the call overwrites) at least one dlogits element lies further from
        the float64 gradient at the unrounded logits than p ((e^(2 b) - 1) + 64 u) allows (b the largest logit bound: a softmax
        entry moves by at most that factor under logits moved by b; 64 u for the fp32 exp, sum and division; label column left out);
      * loss, dh and dwte inside e_emu64 / K <= e_gpu <= K max(e_emu32, e_emu64) against the exact float64 head where the
        emulation's own error reaches the gate's floor (K and the rule: the step protocol's, "fp32" table);
      * the four counters move as ``Hd.dispatched`` says (the logits twice per chunk in the chunked head), and not at all with the
        switch off; pad rows [V, ldV) of dwte are exact zeros; the guards around dh and dwte keep their sentinel; two calls on
        differently poisoned workspaces give identical bits; the loss-only call gives the same loss bits."""
    from rag4dyg_amd import _lib
    from rag4dyg_amd.lm_training import lm_head_train
    lib = _lib.load()
    d, V, B, T = shape
    N, ldV = B * T, Hd.padded_vocab(V)
    chunks = Hd.chunks(ldV)
    h, W, src = head_inputs(dev, d, V, B, T)
    op = head_operand(dev, V, d, W)
    hd, sd = h.to(dev), src.to(dev)
    flags = Hd.dispatched(N, d, V)
    assert flags == (True, True, d % 256 == 0 and N >= 32)

    def call(pattern, grads=True):
        dh, dw = Guarded(dev, N, d), Guarded(dev, ldV, d)
        ws = torch.empty(int(lib.r4d_lm_head_train_workspace_bytes(N, d, ldV)), dtype=torch.uint8, device=dev)
        poison(ws, pattern)
        loss, _ws = lm_head_train(op, hd, sd, T, 1.0, dh.body if grads else None, dw.body if grads else None, ws)
        torch.cuda.synchronize()
        return loss.clone(), dh, dw, ws

    lib.r4d_set_train_head_bf16(0)
    b0 = head_hits()
    loss_off, dh_off, _dw, _ws = call(NAN)
    assert head_delta(b0) == NO_HITS
    lib.r4d_set_train_head_bf16(1)
    b0 = head_hits()
    loss, dh, dw, ws = call(NAN)
    nc = len(chunks)
    want = {"logits": nc * (2 if nc > 1 else 1), "dgrad": nc, "wgrad": nc if flags[2] else 0, "wgrad_fallback": 0 if flags[2] else nc}
    assert head_delta(b0) == want, (head_delta(b0), want)
    assert dh.guards_intact() and dw.guards_intact()
    assert bool((dw.body[V:] == 0).all()) and bool(torch.isfinite(dh.body).all()) and bool(torch.isfinite(dw.body).all())
    assert not torch.equal(dh.body, dh_off.body) and float(loss) != float(loss_off)
    for pattern in (HUGE, ONE, ZERO):
        l2, dh2, dw2, _w = call(pattern)
        assert torch.equal(l2, loss) and torch.equal(dh2.raw, dh.raw) and torch.equal(dw2.raw, dw.raw), pattern
    b1 = head_hits()
    l3, _dh, _dw, _w = call(HUGE, grads=False)
    assert torch.equal(l3, loss)
    assert head_delta(b1) == {"logits": nc, "dgrad": 0, "wgrad": 0, "wgrad_fallback": 0}

    # ---- float64 of the device's own rounded operands
    lab = labels_of(src, B, T)
    Wp = torch.zeros(ldV, d)
    Wp[:V] = W
    h64, W64 = h.double(), Wp.double()
    lg_r = rn(h) @ rn(Wp).t()
    lg_bound = (d + 2) * U * (rn(h).abs() @ rn(Wp).abs().t())
    b = float(lg_bound.max())
    loss_r, _dl = ce64(lg_r[:, :V], lab)
    tol = 2 * b + 64 * U * (float(lg_r.abs().max()) + math.log(V) + 1)
    print(f"[train_bf16_head] {shape}: |loss - loss64| {abs(float(loss) - loss_r):.3e} (tolerance {tol:.3e})")
    assert abs(float(loss) - loss_r) <= tol
    c0, cn = chunks[-1]
    dl_dev = ws.view(torch.float32)[:N * cn].view(N, cn).cpu()                # the last chunk's dlogits
    assert bool((dl_dev[:, max(V - c0, 0):] == 0).all()) and bool((dl_dev[lab < 0] == 0).all())
    # the logits took the bf16 route: dlogits is not the gradient at the unrounded logits
    lg_x = h64 @ W64.t()
    _l, dl_x = ce64(lg_x[:, :V], lab)
    n_counted = int((lab >= 0).sum())
    real = min(cn, V - c0)
    p = torch.softmax(lg_x[:, :V], dim=-1)[:, c0:c0 + real]
    thr = p * ((math.exp(2 * b) - 1) + 64 * U) / n_counted
    far = (dl_dev[:, :real].double() - dl_x[:, c0:c0 + real]).abs() > thr
    far[lab < 0] = False
    cols = torch.arange(c0, c0 + real)
    far[lab[:, None] == cols[None, :]] = False                                # p - 1 at the label: an absolute error, left out
    assert int(far.sum()) >= 1, "dlogits is the exact-f32 head's"
    worst = {}
    dl_r = rn(dl_dev)
    if nc == 1:
        ref = dl_r @ rn(Wp)
        bound = (ldV + 2) * U * (dl_r.abs() @ rn(Wp).abs())
        got = dh.body.cpu().double()
        worst["dh"] = float(((got - ref).abs() / bound.clamp_min(1e-300)).max())
        assert int(((got - dl_dev.double() @ W64).abs() > bound).sum()) >= 1, "dh is the product of the unrounded operands"
    if flags[2]:
        ref = dl_r.t() @ rn(h)
        bound = (N + 2) * U * (dl_r.abs().t() @ rn(h).abs())
        got = dw.body[c0:c0 + cn].cpu().double()
        worst["dwte"] = float(((got - ref).abs() / bound.clamp_min(1e-300)).max())
        assert int(((got - dl_dev.double().t() @ h64).abs() > bound).sum()) >= 1, "dwte is the product of the unrounded operands"
    print(f"[train_bf16_head] {shape}: largest |error| / bound {worst}")
    assert all(v <= 1.0 for v in worst.values()), worst

    # ---- the step protocol's interval against the exact head
    K = Hd.margin("fp32")
    exact = Hd.head_alone(h, W, src, T, torch.float64, None)
    e64 = Hd.head_alone(h, W, src, T, torch.float64, flags)
    e32 = Hd.head_alone(h, W, src, T, torch.float32, flags)
    got = {"loss": float(loss), "dh": dh.body.cpu().double().numpy(), "dW": dw.body[:V].cpu().double().numpy()}
    gated = set()
    for n in ("loss", "dh", "dW"):
        a, c, e = R.rel(e64[n], exact[n]), R.rel(e32[n], exact[n]), R.rel(got[n], exact[n])
        on = a >= R.GATE_FLOOR
        print(f"[train_bf16_head] {shape} {n}: e_gpu {e:.3e} emu64 {a:.3e} emu32 {c:.3e}" + ("" if on else " (not gated)"))
        if on:
            gated.add(n)
            assert a / K <= e <= K * max(a, c), (n, a / K, e, K * max(a, c))
    # a product of two operands rounded to 8 bits sits around 2^-9 from exact: dh always takes the bf16 route, dW where gemm_b1tn
    # takes the shape (its fallback is the exact product of dlogits, which carry the rounded logits' 1e-4 .. 1e-5 only)
    assert "dh" in gated and (not flags[2] or "dW" in gated), gated


def test_01b_head_entry_refusals(dev):
    from rag4dyg_amd import _lib
    from rag4dyg_amd.lm_training import lm_head_train
    d, V, B, T = 256, 100, 2, 16
    h, W, src = head_inputs(dev, d, V, B, T)
    op = head_operand(dev, V, d, W)
    hd, sd = h.to(dev), src.to(dev)
    small = torch.empty(256, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.R4DError, match="workspace"):
        lm_head_train(op, hd, sd, T, workspace=small)
    with pytest.raises(_lib.R4DError):
        lm_head_train(op, hd, sd, 5)                                          # N is no multiple of T
    buf = torch.zeros(B * T * d + 4, device=dev)
    shifted = buf[1:1 + B * T * d].view(B * T, d)                             # contiguous, 4 bytes off a 16-byte boundary
    with pytest.raises(_lib.R4DError, match="16-byte"):
        lm_head_train(op, shifted, sd, T)


# ------------------------------------------------------------------------------------------------------------------ 2. the steps
def stepper(dev, c, precision, head_precision, dropout=None, attention=None, activations=None, freeze=None, seed=0, model=None):
    """``TB.stepper`` with the head precision; the generator kinds also hand out grads["d_fused"] (the trainer's own buffer)"""
    from rag4dyg_amd.generator_training import GeneratorTrainer, PreparedBags
    from rag4dyg_amd.lm_training import LMTrainer
    m = TB.model_of(dev, c) if model is None else model
    x = R.inputs(c)
    kw = dict(dropout=dropout, seed=seed, attention=attention, activations=activations, precision=precision, head_precision=head_precision)
    if c.kind == "lm":
        tr = LMTrainer(m, **kw)
        ids = x["ids"].to(dev)

        def step():
            return {"loss": tr.step(ids), "grads": tr.grads}
        return tr, step
    kw["dropout"] = (0.0, 0.0, 0.0) if dropout is None else dropout
    tr = GeneratorTrainer(m, freeze=(c.kind == "gen") if freeze is None else freeze, **kw)
    tok = x["tok"].to(dev)
    bags = PreparedBags(x["idx"], x["src"], 7).batch(range(len(x["idx"])), dev)
    hidden = torch.empty(c.Bs[0], c.Ts[0], m.config.n_embd, device=dev)

    def step(backward=True):
        loss = tr.step(tok, bags, hidden_out=hidden, backward=backward)
        return {"loss": loss, "grads": dict(tr.grads, d_fused=tr._scratch["d_fused"]) if backward else {}, "hidden": hidden}
    return tr, step


def step_errors(out, exact):
    got = {"loss": float(out["loss"]), "grads": {n: t.detach().cpu().double().numpy() for n, t in out["grads"].items()}}
    if out.get("hidden") is not None:
        got["hidden"] = out["hidden"].detach().cpu().double().numpy()
    assert set(got["grads"]) == set(exact["grads"])
    return R.errors(got, exact)


def gate(c, mode, e):
    """Every gated quantity inside e_emu64 / K <= e_gpu <= K max(e_emu32, e_emu64)"""
    K, tab = Hd.margin(mode), Hd.error_table(c, mode)
    assert set(e) == set(tab)
    bad, ratios = {}, []
    for n, t in tab.items():
        on = t["emu64"] >= R.GATE_FLOOR
        print(f"[train_bf16_head] {mode} {R.case_id(c)} {n}: e_gpu {e[n]:.3e} emu64 {t['emu64']:.3e} emu32 {t['emu32']:.3e}" + ("" if on else " (not gated)"))
        if not on:
            continue
        ratios.append(e[n] / t["emu64"])
        if not t["emu64"] / K <= e[n] <= K * max(t["emu32"], t["emu64"]):
            bad[n] = (t["emu64"] / K, e[n], K * max(t["emu32"], t["emu64"]))
    assert len(ratios) >= Hd.MIN_GATED, (mode, R.case_id(c), len(ratios))
    print(f"[train_bf16_head] {mode} {R.case_id(c)}: K {K:.2f}, {len(ratios)} gated, e_gpu / e_emu64 {min(ratios):.3f} .. {max(ratios):.3f}")
    assert not bad, f"{mode} {R.case_id(c)}: (e_emu64 / K, e_gpu, K max(e_emu32, e_emu64)) outside the gate: {bad}"


STEP_CASES = [R.case("L2_d256_T130", "lm"), R.case("g10_trained", "lm"), R.case("L4_d512_T96", "gen_tied"), R.case("L2_d256_T130", "gen")]
FROZEN = STEP_CASES[3]


@pytest.mark.parametrize("precision", Hd.MODES)
@pytest.mark.parametrize("c", STEP_CASES, ids=[R.case_id(c) for c in STEP_CASES])
def test_02_step_against_the_exact_oracle_inside_the_emulations_margin(dev, c, precision):
    """head bf16 with the layers and attention exact-accurate ("fp32") and on bf16 too ("bf16+attn"): all errors against the EXACT
    float64 step; K and the tables come from the emulation of that combination alone."""
    assert c in Hd.CASES
    _tr, step = stepper(dev, c, precision, "bf16")
    b0 = head_hits()
    out = step()
    dl = head_delta(b0)
    N, d, V = R.rows_of(c), R.weights(c.weights)[0]["transformer.wte.weight"].shape[1], R.weights(c.weights)[0]["transformer.wte.weight"].shape[0]
    flags = Hd.dispatched(N, d, V)
    assert flags[0] and flags[1]
    assert dl == {"logits": 1, "dgrad": 1, "wgrad": int(flags[2]), "wgrad_fallback": int(not flags[2])}, dl
    gate(c, precision, step_errors(out, Hd.exact_of(c)))


def test_02b_planes_are_built_and_used_in_exact_f32_gemm_mode(dev):
    """gemm mode f32 carries no planes by itself: head precision bf16 builds the head's, the three products take them, and the
    layers -- which have none -- stay on the exact-f32 kernels; a head-fp32 trainer in that mode builds none."""
    from rag4dyg_amd import ops
    ops.set_gemm_mode("f32")
    c = STEP_CASES[0]
    tr, step = stepper(dev, c, "fp32", "bf16")
    assert tr.head._w3 is not None and tr.head._w3t is not None and not tr.enc.use_planes
    b0, b1 = head_hits(), TB.hits()
    out = step()
    assert head_delta(b0) == {"logits": 1, "dgrad": 1, "wgrad": 1, "wgrad_fallback": 0} and TB.delta(b1) == {"fwd": 0, "dgrad": 0, "wgrad": 0, "wgrad_fallback": 0}
    gate(c, "fp32", step_errors(out, Hd.exact_of(c)))
    tr32, _s = stepper(dev, c, "fp32", "fp32")
    assert tr32.head._w3 is None


@pytest.mark.parametrize("precision", Hd.MODES)
def test_02c_frozen_step_equals_the_unfrozen_steps_bits_and_the_loss_only_call(dev, precision):
    """As tests/test_gpu_generator_training.py asserts for the default: loss, hidden, the head's and the fusion's gradients (and
    d_fused) of the frozen step are the unfrozen step's, bit for bit; and the loss-only call (the evaluation loss inside the
    training loop) reads the switch like the training call: the same loss bits, not the fp32 head's."""
    m = TB.model_of(dev, FROZEN)
    _t, frozen = stepper(dev, FROZEN, precision, "bf16", freeze=True, seed=5, model=m)
    f = TB.snapshot(frozen())
    _t, free = stepper(dev, FROZEN, precision, "bf16", freeze=False, seed=5, model=m)
    u = TB.snapshot(free())
    assert {"loss", "hidden", "grads:lm_head.weight", "grads:gnn_fusion.convs.0.lin.weight", "grads:gnn_fusion.convs.0.bias", "grads:d_fused"} <= set(f)
    for n in f:
        assert torch.equal(f[n], u[n]), n
    b0 = head_hits()
    only = frozen(backward=False)["loss"].clone()
    assert head_delta(b0) == {"logits": 1, "dgrad": 0, "wgrad": 0, "wgrad_fallback": 0}
    assert torch.equal(only, f["loss"])
    _t, plain = stepper(dev, FROZEN, precision, "fp32", freeze=True, seed=5, model=m)
    assert not torch.equal(plain(backward=False)["loss"], only)


# --------------------------------------------------------------------------------------------- 3. the chunked head inside a step
def chunked_model(dev):
    from oracle import gpt2_ref
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModel
    L, H, d, V = 1, 4, 256, 15900
    sd = gpt2_ref.make_state_dict(L, d, V, n_positions=64, seed=3, random_affine=True)
    sd.pop("lm_head.weight", None)
    m = GPT2LMHeadModel(GPT2Config(vocab_size=V, n_positions=64, n_ctx=64, n_embd=d, n_layer=L, n_head=H))
    m.load_state_dict(sd, strict=False)
    m.tie_weights()
    return m.to(dev).eval(), V


def test_03_chunked_head_inside_an_lm_step(dev):
    """L1, d 256, B 2, T 16, V 15,900 (two chunks, 15,872 + 128): the same bits over repeated steps, with the workspace refilled
    with each poison pattern, and under stored and recompute attention and activations; per step the logits GEMM runs twice per
    chunk, dh and dwte once."""
    from rag4dyg_amd.lm_training import LMTrainer
    m, V = chunked_model(dev)
    ids = torch.randint(0, V, (2, 16), generator=torch.Generator().manual_seed(9)).to(dev)
    base = None
    for attention in ("stored", "recompute"):
        for activations in ("stored", "recompute"):
            tr = LMTrainer(m, attention=attention, activations=activations, precision="bf16+attn", head_precision="bf16")
            b0 = head_hits()
            s = TB.snapshot({"loss": tr.step(ids), "grads": tr.grads})
            assert head_delta(b0) == {"logits": 4, "dgrad": 2, "wgrad": 2, "wgrad_fallback": 0}
            assert all(bool(torch.isfinite(t).all()) for t in s.values())
            if base is None:
                base = s
                TB.assert_same_bits(base, TB.snapshot({"loss": tr.step(ids), "grads": tr.grads}), "a repeated step")
                for pattern in (ZERO, NAN, HUGE, ONE):
                    poison(tr._ws, pattern)
                    TB.assert_same_bits(base, TB.snapshot({"loss": tr.step(ids), "grads": tr.grads}), ("workspace", pattern))
            else:
                TB.assert_same_bits(base, s, (attention, activations))
    tr = LMTrainer(m, precision="bf16+attn", head_precision="fp32")
    s = TB.snapshot({"loss": tr.step(ids), "grads": tr.grads})
    assert not torch.equal(s["loss"], base["loss"]) and not torch.equal(s["grads:transformer.wte.weight"], base["grads:transformer.wte.weight"])


# ------------------------------------------------------------------------------------------- 4. the independence of the switches
def test_04_each_switch_leaves_the_other_two_alone(dev):
    from rag4dyg_amd import _lib
    lib = _lib.load()
    sw = [(lib.r4d_set_train_bf16, lib.r4d_get_train_bf16), (lib.r4d_set_train_attention_bf16, lib.r4d_get_train_attention_bf16),
          (lib.r4d_set_train_head_bf16, lib.r4d_get_train_head_bf16)]
    for s, _g in sw:
        s(0)
    for others in ((0, 0), (1, 0), (0, 1), (1, 1)):
        for i, (s, g) in enumerate(sw):
            rest = [p for j, p in enumerate(sw) if j != i]
            for (so, _go), v in zip(rest, others):
                so(v)
            assert s(1) == 0 and g() == 1 and tuple(go() for _so, go in rest) == others
            assert s(0) == 1 and g() == 0 and tuple(go() for _so, go in rest) == others
            for so, _go in rest:
                so(0)


def test_04b_trainers_of_both_head_precisions_alternate_in_one_process(dev, monkeypatch):
    """Each trainer selects its own head precision before every call: alternating steps of a head-fp32 and a head-bf16 trainer on
    one model equal a fresh trainer of their kind bit for bit, the fp32 one counts no head launch, and the two differ.  The
    environment variable is honoured and an explicit argument wins; a bad name raises."""
    from rag4dyg_amd import _lib
    from rag4dyg_amd.generator_training import GeneratorTrainer
    from rag4dyg_amd.lm_training import LMTrainer
    lib = _lib.load()
    c = STEP_CASES[0]
    m = TB.model_of(dev, c)
    monkeypatch.delenv("R4D_TRAIN_HEAD_PRECISION", raising=False)
    fresh = {}
    for hp in ("fp32", "bf16"):
        _t, step = stepper(dev, c, "bf16+attn", hp, model=m)
        fresh[hp] = TB.snapshot(step())
        assert lib.r4d_get_train_head_bf16() == (hp == "bf16") and lib.r4d_get_train_bf16() == 1 and lib.r4d_get_train_attention_bf16() == 1
    assert not torch.equal(fresh["fp32"]["loss"], fresh["bf16"]["loss"])
    steps = {hp: stepper(dev, c, "bf16+attn", hp, model=m)[1] for hp in ("fp32", "bf16")}
    for hp in ("fp32", "bf16", "bf16", "fp32", "bf16", "fp32"):
        b0 = head_hits()
        TB.assert_same_bits(fresh[hp], TB.snapshot(steps[hp]()), hp)
        assert (head_delta(b0) == NO_HITS) == (hp == "fp32")
    # a trainer without a head leaves the head switch where it was
    lib.r4d_set_train_head_bf16(1)
    _t, enc = TB.stepper(dev, R.case("L2_d256_T130", "enc"), "fp32")
    b0 = head_hits()
    enc()
    assert lib.r4d_get_train_head_bf16() == 1 and head_delta(b0) == NO_HITS
    monkeypatch.setenv("R4D_TRAIN_HEAD_PRECISION", "bf16")
    assert LMTrainer(m).head_precision == "bf16" and LMTrainer(m, head_precision="fp32").head_precision == "fp32"
    gm = TB.model_of(dev, FROZEN)
    assert GeneratorTrainer(gm, freeze=True).head_precision == "bf16"
    assert GeneratorTrainer(gm, freeze=True, head_precision="fp32").head_precision == "fp32"
    monkeypatch.setenv("R4D_TRAIN_HEAD_PRECISION", "fp16")
    with pytest.raises(ValueError):
        LMTrainer(m)
    for bad in ("fp16", "BF16", "bf16+attn"):
        with pytest.raises(ValueError):
            LMTrainer(m, head_precision=bad)
        with pytest.raises(ValueError):
            GeneratorTrainer(gm, freeze=True, head_precision=bad)


def test_04c_off_means_off(dev):
    """Head precision fp32 gives the same bits before the head switch was ever used by this trainer's process and after, whatever
    planes a head-bf16 trainer built meanwhile; none of the four counters moves; the encoder forward keeps its bits with the
    switch on."""
    from rag4dyg_amd import _lib
    lib = _lib.load()
    c = STEP_CASES[0]
    m = TB.model_of(dev, c)
    ids = R.inputs(c)["ids"].to(dev)
    b0 = head_hits()
    steps = {p: stepper(dev, c, p, "fp32", model=m)[1] for p in ("fp32", "bf16+attn")}
    first = {p: TB.snapshot(s()) for p, s in steps.items()}
    g_first = TB.snapshot(stepper(dev, FROZEN, "fp32", "fp32")[1]())
    h0 = m.transformer(input_ids=ids)[0].clone()
    assert head_delta(b0) == NO_HITS and lib.r4d_get_train_head_bf16() == 0
    for p in ("fp32", "bf16+attn"):
        on = TB.snapshot(stepper(dev, c, p, "bf16", model=m)[1]())
        assert any(not torch.equal(on[n], first[p][n]) for n in on if n.startswith("grads:"))
    assert lib.r4d_get_train_head_bf16() == 1
    assert torch.equal(h0, m.transformer(input_ids=ids)[0])                   # with the head switch ON
    mid = head_hits()
    for p, s in steps.items():
        TB.assert_same_bits(first[p], TB.snapshot(s()), (p, "after the head mode"))
        assert lib.r4d_get_train_head_bf16() == 0
    TB.assert_same_bits(g_first, TB.snapshot(stepper(dev, FROZEN, "fp32", "fp32")[1]()), "frozen generator step")
    assert head_hits() == mid


# ------------------------------------------------------------------------------------------------------ 5. a short training run
def test_05_a_short_training_run(dev):
    """30 AdamW steps of LMTrainer on L2 d256, B 8, T 40, dropout 0.1, the same seed, under "bf16+attn" with the head in fp32 and in
    bf16: first and final loss of each, printed, not gated (the loss must fall and stay finite)."""
    from rag4dyg_amd import training
    from rag4dyg_amd.lm_training import LMTrainer
    c = R.case("L2_d256_T130", "lm")
    V = R.weights(c.weights)[0]["transformer.wte.weight"].shape[0]
    ids = torch.randint(0, V - 2, (8, 40), generator=torch.Generator().manual_seed(77)).to(dev)
    losses = {}
    for hp in ("fp32", "bf16"):
        tr = LMTrainer(TB.model_of(dev, c).train(), dropout=(0.1, 0.1, 0.1), seed=3, precision="bf16+attn", head_precision=hp)
        opt = training.AdamW(tr.params, tr.grads, lr=1e-3, weight_decay=0.01, flat_grads=tr.flat_grads)
        ls = []
        for _ in range(30):
            ls.append(tr.step(ids))
            opt.step(max_grad_norm=1.0)
        losses[hp] = [float(v) for v in torch.stack(ls).cpu()]
    a, b = losses["fp32"], losses["bf16"]
    print(f"[train_bf16_head] 30 steps under bf16+attn: head fp32 {a[0]:.4f} -> {a[-1]:.4f}, head bf16 {b[0]:.4f} -> {b[-1]:.4f}, "
          f"final difference {abs(a[-1] - b[-1]):.2e}")
    for ls in (a, b):
        assert all(v == v for v in ls) and ls[-1] < ls[0], ls
