"""The training steps' opt-in bf16 attention products on the GPU (the ``+attn`` precisions of the three trainers,
``r4d_set_train_attention_bf16``, csrc/gemm_b1h.hip): each of the six per-head products alone against float64 of the bf16-rounded
operands at a derived bound, what a product may write, its independence of the batch it rides in, the steps against the EXACT
float64 oracle inside the margins the emulations of tests/_train_bf16_attn_ref.py give, the isolation of everything the switch must
not touch, the recompute modes, the launch accounting, the refusals, and a short training run.

The step helpers (``stepper``, ``model_of``, ``snapshot`` ...) are those of tests/test_gpu_train_bf16.py.  Every test restores the
switches it found."""
import math

import pytest
import torch

import _train_modes
import _train_bf16_attn_ref as A
import _train_bf16_ref as R
import test_gpu_train_bf16 as TB
from _poison import NAN, HUGE, ONE, ZERO, poison

pytestmark = pytest.mark.gpu

ATTN_PREFIX = "tuning:train_bf16_attn:"
LM, ENC, GEN = TB.LM, TB.ENC, TB.GEN
SENTINEL = -7777.25
GUARD = 64               # floats in front of and behind every buffer the product may write


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


restore_switches = _train_modes.switches_restored(ops_too=True)


def attn_hits():
    return TB.hits(ATTN_PREFIX)


def attn_delta(before):
    return {n: v - before[n] for n, v in attn_hits().items()}


# ------------------------------------------------------------------------------------------------- the six products alone
# which -> (A layout, A slice, B layout, B slice, C layout, C slice, B given as [N, K]); a "qkv" operand is slice 0 / 1 / 2 (Q / K / V)
# of a [B, T, 3d] buffer, "merged" is [B, T, d], "probs" is [B*H, T, ld]
PRODUCTS = {
    "s": ("qkv", 0, "qkv", 1, "probs", 0, True),
    "pv": ("probs", 0, "qkv", 2, "merged", 0, False),
    "dp": ("merged", 0, "qkv", 2, "probs", 0, True),
    "dq": ("probs", 0, "qkv", 1, "qkv", 0, False),
    "dk": ("probs", 0, "qkv", 0, "qkv", 1, False),
    "dv": ("probs", 0, "merged", 0, "qkv", 2, False),
}
# (B, H, T, hd): every T of {1, 4, 17, 31, 32, 33, 127, 128, 129, 257} and every hd of {16, 48, 64, 96, 128, 256}, crossed sparsely:
# T below / at / above the 32-key k-tile, the 64-row tile and the 128-float P row; one and several tiles; one and several batches
SHAPES = [(1, 1, 1, 16), (2, 2, 4, 16), (2, 3, 17, 48), (1, 2, 33, 64), (2, 2, 129, 96), (1, 2, 257, 128), (1, 1, 130, 256),
          (1, 2, 31, 64), (1, 2, 32, 64), (1, 2, 127, 64), (1, 2, 128, 64)]


def up4(x):
    return (x + 3) // 4 * 4


class Buf:
    """One operand in the step's layout inside a guarded flat buffer: ``raw`` = GUARD floats, the operand, ``tail`` floats."""

    def __init__(self, dev, kind, sl, B, T, H, d, fill, tail=0):
        from rag4dyg_amd import ops
        self.kind, self.sl, self.dims = kind, sl, (B, T, H, d)
        self.ld = ops.train_attn_probs_ld(T)
        self.n = {"qkv": B * T * 3 * d, "merged": B * T * d, "probs": B * H * T * self.ld}[kind]
        self.raw = torch.full((GUARD + self.n + max(tail, GUARD),), fill, dtype=torch.float32, device=dev)
        self.body = self.raw[GUARD:GUARD + self.n]

    def blocks(self, body=None):
        """[B, H, T, columns] view of the (sequence, head) blocks: hd columns, or the ld columns of a P-shaped row (``body``: another
        flat tensor of the operand's size, viewed the same way)"""
        B, T, H, d = self.dims
        body = self.body if body is None else body
        if self.kind == "qkv":
            return body.view(B, T, 3, H, d // H)[:, :, self.sl].permute(0, 2, 1, 3)
        if self.kind == "merged":
            return body.view(B, T, H, d // H).permute(0, 2, 1, 3)
        return body.view(B, H, T, self.ld)

    def ptr(self):
        """a tensor whose first element is the (sequence 0, head 0) element of the operand"""
        return self.body[self.sl * self.dims[3]:] if self.kind == "qkv" else self.body


def make_operand(dev, name, which, kind, sl, B, T, H, d, g):
    """Random data where the product reads, NaN wherever the contract says it never does: behind the buffer (the rows past T of the
    last sequence's block lie there), and in the columns [up4(T), ld) of a P-shaped operand, whose columns [T, up4(T)) are zero as
    the softmax and its backward leave them.  The P of "pv" is lower-triangular like a causal softmax's output."""
    buf = Buf(dev, kind, sl, B, T, H, d, float("nan"), tail=4 * 3 * d)
    if kind == "probs":
        x = torch.randn(B, H, T, T, generator=g) * (0.05 if name == "a" and which != "pv" else 1.0)
        if which == "pv":
            x = torch.tril(x.abs())
        blk = buf.blocks()
        blk[..., :T] = x.to(dev)
        blk[..., T:up4(T)] = 0.0
    else:
        buf.body.copy_((torch.randn(buf.n, generator=g) * (1e-3 if kind == "merged" else 1.0)).to(dev))      # dO: a gradient's scale
    return buf


def run_product(dev, which, B, H, T, hd, seed=0):
    """-> (a, b, c) Bufs after the call; c was pre-filled with SENTINEL"""
    from rag4dyg_amd import ops
    d = H * hd
    ka, sa, kb, sb, kc, sc, _bt = PRODUCTS[which]
    g = torch.Generator().manual_seed(100000 * seed + 1000 * T + 10 * hd + B + H + 7 * ops.TRAIN_ATTN_PRODUCTS.index(which))
    a = make_operand(dev, "a", which, ka, sa, B, T, H, d, g)
    b = make_operand(dev, "b", which, kb, sb, B, T, H, d, g)
    c = Buf(dev, kc, sc, B, T, H, d, SENTINEL)
    ops.train_attn_product_bf16(which, a.ptr(), b.ptr(), c.ptr(), B, T, H, d)
    torch.cuda.synchronize()
    return a, b, c


def reference(which, a, b, T, hd, rounded=True):
    """(float64 product of the operands' blocks [B, H, T, N], the bound's sum |a| |b| [B, H, T, N], contraction length)"""
    bt = PRODUCTS[which][6]
    K = hd if bt else T
    x = a.blocks()[..., :K]
    y = b.blocks()
    if rounded:
        x, y = x.bfloat16(), y.bfloat16()
    x, y = x.double(), y.double()
    y = y.transpose(-1, -2) if bt else y
    scale = math.sqrt(hd) if which == "s" else 1.0
    return torch.matmul(x, y) / scale, torch.matmul(x.abs(), y.abs()) / scale, K


@pytest.mark.parametrize("which", list(PRODUCTS))
@pytest.mark.parametrize("shape", SHAPES, ids=["B{}H{}T{}hd{}".format(*s) for s in SHAPES])
def test_01_each_product_alone_and_what_it_writes(dev, shape, which):
    """|c - c64| <= (K + 2) 2^-24 sum_k |a^_k| |b^_k| element by element, c64 the float64 product of the bf16-rounded operands
    (bf16 x bf16 is exact in fp32: the roundings are the accumulation's K - 1 and, for S, the division's and its divisor's), on and
    below the diagonal only for the causal S.  The result is NOT the product of the unrounded operands: at least one element is
    further than that bound from it.  Operands carry NaN wherever they must not be read (``make_operand``).  Every element of C's
    buffer outside the (sequence, head) blocks' [T, N] ranges -- the other slices of a [B, T, 3d] target, the columns [T, ld) of a
    P-shaped one, the guards on both sides -- still holds the sentinel C was filled with."""
    B, H, T, hd = shape
    a, b, c = run_product(dev, which, B, H, T, hd)
    N = T if PRODUCTS[which][6] else hd
    got = c.blocks()[..., :N].double()
    c64, sab, K = reference(which, a, b, T, hd)
    assert torch.isfinite(c64).all()
    bound = (K + 2) * 2.0 ** -24 * sab
    mask = torch.ones(T, N, dtype=torch.bool, device=dev)
    if which == "s":
        mask = torch.tril(mask)
    err = ((got - c64).abs() / bound.clamp_min(1e-300))[..., mask]
    worst = float(err.max())
    print(f"[train_bf16_attn] {which} B{B} H{H} T{T} hd{hd}: largest |error| / bound {worst:.3f}")
    assert worst <= 1.0, (which, shape, worst)
    exact, _s, _k = reference(which, a, b, T, hd, rounded=False)
    far = (((got - exact).abs() > bound)[..., mask]).sum()
    assert int(far) >= 1, (which, shape, "the result is the exact-f32 product's")
    # what was written: the blocks' [T, N] ranges and nothing else
    written = torch.zeros_like(c.raw, dtype=torch.bool)
    c.blocks(written[GUARD:GUARD + c.n])[..., :N] = True
    assert bool((c.raw[~written] == SENTINEL).all()), (which, shape, "wrote outside C's blocks")
    touched = c.raw[written] != SENTINEL
    if which != "s":
        assert bool(touched.all()), (which, shape, "left part of C's blocks unwritten")


def test_02_a_q_slice_target_leaves_the_k_and_v_slices_alone(dev):
    """dQ into the Q slice of a [B, T, 3d] target: the K and V slices (other launches' results in the step) keep their bits, and so
    does every other head's block while ONE head's product is computed through a one-head call on its columns."""
    B, H, T, hd = 2, 3, 33, 48
    d = H * hd
    _a, _b, c = run_product(dev, "dq", B, H, T, hd)
    full = c.body.view(B, T, 3, d)
    assert bool((full[:, :, 1:] == SENTINEL).all()) and bool((full[:, :, 0] != SENTINEL).all())
    _a, _b, c = run_product(dev, "dv", B, H, T, hd)
    full = c.body.view(B, T, 3, d)
    assert bool((full[:, :, :2] == SENTINEL).all()) and bool((full[:, :, 2] != SENTINEL).all())


@pytest.mark.parametrize("which", list(PRODUCTS))
def test_03_a_block_does_not_depend_on_the_batch_it_rides_in(dev, which):
    """The [T, N] block of one (sequence, head) inside B = 3, H = 3 has the bits of the same operands computed as B = 1, H = 1."""
    from rag4dyg_amd import ops
    for T, hd in ((33, 48), (129, 64)):
        B, H = 3, 3
        a, b, c = run_product(dev, which, B, H, T, hd, seed=1)
        N = T if PRODUCTS[which][6] else hd
        ka, sa, kb, sb, kc, sc, _bt = PRODUCTS[which]
        for bi, hi in ((0, 0), (1, 2), (2, 1)):
            a1 = Buf(dev, ka, sa, 1, T, 1, hd, float("nan"), tail=4 * 3 * hd)
            b1 = Buf(dev, kb, sb, 1, T, 1, hd, float("nan"), tail=4 * 3 * hd)
            c1 = Buf(dev, kc, sc, 1, T, 1, hd, SENTINEL)
            a1.blocks()[0, 0] = a.blocks()[bi, hi]
            b1.blocks()[0, 0] = b.blocks()[bi, hi]
            ops.train_attn_product_bf16(which, a1.ptr(), b1.ptr(), c1.ptr(), 1, T, 1, hd)
            mask = torch.tril(torch.ones(T, N, dtype=torch.bool, device=dev)) if which == "s" else torch.ones(T, N, dtype=torch.bool, device=dev)
            assert torch.equal(c1.blocks()[0, 0, :, :N][mask], c.blocks()[bi, hi, :, :N][mask]), (which, T, hd, bi, hi)


# ------------------------------------------------------------------------------------------------------------------ the steps
def step_errors(out, exact):
    got = {"loss": float(out["loss"]), "grads": {n: t.detach().cpu().double().numpy() for n, t in out["grads"].items()}}
    for k in ("emb", "hidden"):
        if out.get(k) is not None:
            got[k] = out[k].detach().cpu().double().numpy()
    assert set(got["grads"]) == set(exact["grads"])
    return R.errors(got, exact)


def gate(c, mode, e):
    """Every gated quantity inside e_emu64 / K <= e_gpu <= K max(e_emu32, e_emu64); -> the gated e_gpu / e_emu64 ratios"""
    K, tab = A.margin(mode), A.error_table(c, mode)
    assert set(e) == set(tab)
    bad, ratios = {}, []
    for n, t in tab.items():
        gated = t["emu64"] >= R.GATE_FLOOR
        print(f"[train_bf16_attn] {mode} {R.case_id(c)} {n}: e_gpu {e[n]:.3e} emu64 {t['emu64']:.3e} emu32 {t['emu32']:.3e}" + ("" if gated else " (not gated)"))
        if not gated:
            continue
        ratios.append(e[n] / t["emu64"])
        if not t["emu64"] / K <= e[n] <= K * max(t["emu32"], t["emu64"]):
            bad[n] = (t["emu64"] / K, e[n], K * max(t["emu32"], t["emu64"]))
    assert len(ratios) >= A.MIN_GATED, (mode, R.case_id(c), len(ratios))
    print(f"[train_bf16_attn] {mode} {R.case_id(c)}: K {K:.2f}, {len(ratios)} gated, e_gpu / e_emu64 {min(ratios):.3f} .. {max(ratios):.3f}")
    assert not bad, f"{mode} {R.case_id(c)}: (e_emu64 / K, e_gpu, K max(e_emu32, e_emu64)) outside the gate: {bad}"
    return ratios


@pytest.mark.parametrize("c", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_04_step_against_the_exact_oracle_inside_the_combined_emulations_margin(dev, c):
    """"bf16+attn": all three errors against the EXACT float64 step; K and the tables come from the combined emulation alone."""
    _tr, step = TB.stepper(dev, c, "bf16+attn")
    b0, b1 = attn_hits(), TB.hits()
    out = step()
    da, dl = attn_delta(b0), TB.delta(b1)
    gate(c, "bf16+attn", step_errors(out, R.references(c)[0]))
    assert da["nt"] > 0 and da["nn"] > 0 and dl["fwd"] > 0 and dl["dgrad"] > 0


ATTN_ONLY = [R.case("L2_d256_T130", k) for k in R.KINDS] + [R.case("g10_trained", "lm")]


@pytest.mark.parametrize("c", ATTN_ONLY, ids=[R.case_id(c) for c in ATTN_ONLY])
def test_04b_attention_alone_under_gemm_mode_f32(dev, c):
    """"fp32+attn" under gemm mode f32 (every other GEMM exact): the attention-only emulation's tables and K."""
    from rag4dyg_amd import _lib, ops
    ops.set_gemm_mode("f32")
    _tr, step = TB.stepper(dev, c, "fp32+attn")
    b0, b1 = attn_hits(), TB.hits()
    out = step()
    lib = _lib.load()
    assert lib.r4d_get_train_bf16() == 0 and lib.r4d_get_train_attention_bf16() == 1
    assert attn_delta(b0)["nt"] > 0 and TB.delta(b1) == {"fwd": 0, "dgrad": 0, "wgrad": 0, "wgrad_fallback": 0}
    gate(c, "fp32+attn", step_errors(out, R.references(c)[0]))


def test_05_isolation(dev):
    """ "fp32" and "bf16" steps have the same bits before the new mode was ever on and after it went off, and count no launch of the
    new kernel; "bf16" leaves the attention switch off; the encoder forward and the retrieval encode loop keep their bits with the
    switch on; "bf16+attn" is not "bf16"."""
    from rag4dyg_amd import _lib, retrieval
    lib = _lib.load()
    m = TB.model_of(dev, LM)
    ids = R.inputs(LM)["ids"].to(dev)

    def encoder_bits():
        return m.transformer(input_ids=ids)[0].clone(), retrieval.encode_batches(m, [ids, ids[:2, :57].contiguous()]).clone()
    before = attn_hits()
    steps = {(p, k): TB.stepper(dev, c, p, model=m if k == "lm" else None)[1] for p in ("fp32", "bf16") for k, c in (("lm", LM), ("enc", ENC))}
    first = {key: TB.snapshot(s()) for key, s in steps.items()}
    assert lib.r4d_get_train_attention_bf16() == 0
    assert attn_delta(before) == {"nt": 0, "nn": 0}
    h0 = encoder_bits()
    _t, step_a = TB.stepper(dev, LM, "bf16+attn", model=m)
    ga = TB.snapshot(step_a())
    assert lib.r4d_get_train_bf16() == 1 and lib.r4d_get_train_attention_bf16() == 1
    assert attn_delta(before)["nt"] > 0
    g16 = first[("bf16", "lm")]
    assert any(not torch.equal(ga[n], g16[n]) for n in ga if n.startswith("grads:")), "bf16+attn gave the bits of bf16"
    h1 = encoder_bits()                                                     # with the attention switch ON
    assert torch.equal(h0[0], h1[0]) and torch.equal(h0[1], h1[1])
    _t, step_ea = TB.stepper(dev, ENC, "fp32+attn")
    step_ea()
    mid = attn_hits()
    for key, s in steps.items():
        TB.assert_same_bits(first[key], TB.snapshot(s()), (key, "after the attention mode"))
        assert lib.r4d_get_train_attention_bf16() == 0 and lib.r4d_get_train_bf16() == (key[0] == "bf16")
    assert attn_hits() == mid


@pytest.mark.parametrize("c", (ENC, LM, GEN), ids=("enc", "lm", "gen"))
def test_06_recompute_modes_give_the_same_bits(dev, c):
    base = None
    for attention in ("stored", "recompute"):
        for activations in ("stored", "recompute"):
            _t, step = TB.stepper(dev, c, "bf16+attn", dropout=(0.1, 0.1, 0.1), attention=attention, activations=activations, seed=5)
            s = TB.snapshot(step())
            if base is None:
                base = s
            else:
                TB.assert_same_bits(base, s, (attention, activations))


def test_06b_frozen_generator_step_equals_the_unfrozen_steps_bits(dev):
    m = TB.model_of(dev, GEN)
    _t, frozen = TB.stepper(dev, GEN, "bf16+attn", dropout=(0.1, 0.1, 0.1), freeze=True, seed=5, model=m)
    f = TB.snapshot(frozen())
    _t, free = TB.stepper(dev, GEN, "bf16+attn", dropout=(0.1, 0.1, 0.1), freeze=False, seed=5, model=m)
    u = TB.snapshot(free())
    assert {"loss", "hidden", "grads:lm_head.weight", "grads:gnn_fusion.convs.0.lin.weight", "grads:gnn_fusion.convs.0.bias"} <= set(f)
    for n in f:
        assert torch.equal(f[n], u[n]), n


@pytest.mark.parametrize("c", (ENC, LM), ids=("enc", "lm"))
def test_06c_poisoned_workspace_and_repeated_step(dev, c):
    """A repeated step gives the same bits, and so does a step on a workspace refilled with NaN bytes, 0x7F bytes or the word 1."""
    tr, step = TB.stepper(dev, c, "bf16+attn")
    base = TB.snapshot(step())
    TB.assert_same_bits(base, TB.snapshot(step()), "a repeated step")
    for pattern in (ZERO, NAN, HUGE, ONE):
        assert tr._ws is not None
        poison(tr._ws, pattern)
        TB.assert_same_bits(base, TB.snapshot(step()), ("workspace", pattern))


def test_07_launch_accounting(dev):
    """Per layer and group: 1 NT (S) + 1 NN (P.V) forward, 1 NT (dP) + 3 NN (dQ, dK, dV) backward.  Attention recompute forms S again
    in the backward (+1 NT per layer and group); activation recompute runs the forward's two again for every layer but the last
    (its activations are still there behind the forward).  The layer axis counts what "bf16" counts."""
    L = 2
    _t, step = TB.stepper(dev, LM, "bf16")
    b = TB.hits(); step()
    layer_axis = TB.delta(b)
    assert layer_axis == {"fwd": 4 * L, "dgrad": 4 * L, "wgrad": 4 * L, "wgrad_fallback": 0}
    _t, step = TB.stepper(dev, LM, "bf16+attn")
    b0, b1 = attn_hits(), TB.hits(); step()
    assert attn_delta(b0) == {"nt": 2 * L, "nn": 4 * L} and TB.delta(b1) == layer_axis
    _t, step = TB.stepper(dev, LM, "bf16+attn", attention="recompute")
    b0, b1 = attn_hits(), TB.hits(); step()
    assert attn_delta(b0) == {"nt": 3 * L, "nn": 4 * L} and TB.delta(b1) == layer_axis
    _t, step = TB.stepper(dev, LM, "bf16+attn", activations="recompute")
    b0 = attn_hits(); step()
    assert attn_delta(b0) == {"nt": 2 * L + (L - 1), "nn": 4 * L + (L - 1)}
    _t, step = TB.stepper(dev, LM, "bf16+attn", attention="recompute", activations="recompute")
    b0 = attn_hits(); step()
    assert attn_delta(b0) == {"nt": 3 * L + (L - 1), "nn": 4 * L + (L - 1)}
    G = len(ENC.Bs)
    assert G == 3
    _t, step = TB.stepper(dev, ENC, "bf16+attn")
    b0 = attn_hits(); step()
    assert attn_delta(b0) == {"nt": 2 * L * G, "nn": 4 * L * G}
    _t, step = TB.stepper(dev, ENC, "fp32+attn", attention="recompute")
    b0, b1 = attn_hits(), TB.hits(); step()
    assert attn_delta(b0) == {"nt": 3 * L * G, "nn": 4 * L * G} and TB.delta(b1) == {"fwd": 0, "dgrad": 0, "wgrad": 0, "wgrad_fallback": 0}
    _t, step = TB.stepper(dev, GEN, "bf16+attn")                           # frozen: the same attention launches, no weight gradient
    b0 = attn_hits(); step()
    assert attn_delta(b0) == {"nt": 2 * L, "nn": 4 * L}


def test_08_refusals(dev, monkeypatch):
    from rag4dyg_amd import _lib, training
    from rag4dyg_amd.lm_training import LMTrainer
    x = R.inputs(ENC)
    ids, G = [t.to(dev) for t in x["ids"]], x["G"].to(dev)
    for first, second in (("bf16+attn", "bf16"), ("bf16", "bf16+attn"), ("fp32+attn", "fp32"), ("fp32", "fp32+attn")):
        tr = training.EncoderTrainer(TB.model_of(dev, ENC), precision=first)
        tr.forward(ids)
        tr.precision = second
        with pytest.raises(_lib.R4DError, match="train-attention-bf16"):
            tr.backward(G)
        tr.precision = first
        tr.forward(ids)
        tr.backward(G)                                                     # the matching pair goes through
    m = TB.model_of(dev, LM)
    for bad in ("fp16", "BF16", "half", "fp16+attn"):
        with pytest.raises(ValueError):
            LMTrainer(m, precision=bad)
        with pytest.raises(ValueError):
            training.EncoderTrainer(m, precision=bad)
    monkeypatch.setenv("R4D_TRAIN_PRECISION", "bf16+attn")
    tr = LMTrainer(m)
    assert tr.enc.precision == "bf16+attn" and tr.enc.use_planes
    monkeypatch.setenv("R4D_TRAIN_PRECISION", "fp32+attn")
    from rag4dyg_amd import ops
    ops.set_gemm_mode("f32")
    tr = LMTrainer(m)
    assert tr.enc.precision == "fp32+attn" and not tr.enc.use_planes       # the planes follow the layer axis only


def test_09_a_short_training_run(dev):
    """30 AdamW steps of LMTrainer on L2 d256, B 8, T 40 (the seed of test_gpu_train_bf16.py::test_10) in "bf16" and "bf16+attn": the
    loss falls in both; the difference of the final losses is recorded (printed), not gated."""
    from rag4dyg_amd import training
    from rag4dyg_amd.lm_training import LMTrainer
    c = R.case("L2_d256_T130", "lm")
    V = R.weights(c.weights)[0]["transformer.wte.weight"].shape[0]
    ids = torch.randint(0, V - 2, (8, 40), generator=torch.Generator().manual_seed(77)).to(dev)
    losses = {}
    for precision in ("bf16", "bf16+attn"):
        tr = LMTrainer(TB.model_of(dev, c).train(), dropout=(0.1, 0.1, 0.1), seed=3, precision=precision)
        opt = training.AdamW(tr.params, tr.grads, lr=1e-3, weight_decay=0.01, flat_grads=tr.flat_grads)
        ls = []
        for _ in range(30):
            ls.append(tr.step(ids))
            opt.step(max_grad_norm=1.0)
        losses[precision] = [float(v) for v in torch.stack(ls).cpu()]
    a, b = losses["bf16"], losses["bf16+attn"]
    print(f"[train_bf16_attn] 30 steps: bf16 {a[0]:.4f} -> {a[-1]:.4f}, bf16+attn {b[0]:.4f} -> {b[-1]:.4f}, final difference {abs(a[-1] - b[-1]):.2e}")
    for ls in (a, b):
        assert all(v == v for v in ls) and ls[-1] < ls[0], ls
