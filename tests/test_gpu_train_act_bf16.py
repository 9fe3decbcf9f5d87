"""The bf16 activation store of the bf16 training steps on the GPU (``act_store="bf16"`` of the three trainers,
``r4d_set_train_act_bf16``): the LayerNorm outputs ln1 (layers >= 1) and ln2 and the GELU output f are written as
bf16 by their producers and read as bf16 by gemm_b1 / gemm_b1tn, which round the fp32 form to the same bits while they stage it.

So nothing here needs a tolerance: every comparison is for EQUAL BITS against code the store does not touch -- the single ops
against the fp32-operand ops on the same values, the steps against the same steps with the store off.  (One exception, stated
where it occurs: a NaN stays a NaN, but its payload is the hardware conversion's, not torch's.)

Every test restores the switches it found."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

import _train_modes
import _train_bf16_ref as R
from _poison import PATTERNS, poison
from conftest import load_state_dict_checked

pytestmark = pytest.mark.gpu

BRANCH_PREFIX = "tuning:train_act_bf16:"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


restore_switches = _train_modes.switches_restored(ops_too=True)


def hits(prefix=BRANCH_PREFIX):
    from rag4dyg_amd import _lib
    lib = _lib.load()
    out = {}
    for i in range(lib.r4d_dispatch_num_branches()):
        n = lib.r4d_dispatch_branch_name(i).decode()
        if n.startswith(prefix):
            out[n[len(prefix):]] = int(lib.r4d_dispatch_branch_hits(i))
    return out


def delta(before, prefix=BRANCH_PREFIX):
    return {n: v - before[n] for n, v in hits(prefix).items()}


def bits(t):
    """the tensor's bit patterns (so that NaNs compare like any other value)"""
    return t.contiguous().reshape(-1).view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# --------------------------------------------------------------------------------------------------------- the single ops
@pytest.mark.parametrize("d", (256, 768))
@pytest.mark.parametrize("rows", (1, 33, 130))
def test_01_layernorm_with_a_bf16_output(dev, rows, d):
    """y = RN_bf16(ops.layernorm(x)) bit for bit (round to nearest even), a row of zeros and a row holding a NaN included.  A NaN
    row is NaN in every element on both sides; only there the bits are the hardware conversion's (sign and quiet bit of the fp32
    NaN) where torch's conversion writes its canonical NaN -- compared as "NaN where NaN"."""
    from rag4dyg_amd import ops
    g = torch.Generator().manual_seed(rows * 1000 + d)
    x = torch.randn(rows, d, generator=g) * 3.0 + 0.5
    zero_row, nan_row = (rows // 2, rows - 1) if rows > 1 else (None, None)
    if rows > 1:
        x[zero_row] = 0.0
        x[nan_row, d // 3] = float("nan")
    w = torch.randn(d, generator=g) * 0.2 + 1.0
    b = torch.randn(d, generator=g) * 0.1
    x, w, b = x.to(dev), w.to(dev), b.to(dev)
    want32 = ops.layernorm(x, w, b)
    want = want32.to(torch.bfloat16)
    got = ops.layernorm_bf16(x, w, b)
    assert got.dtype == torch.bfloat16 and got.shape == want.shape
    ok = torch.ones(rows, dtype=torch.bool, device=dev)
    if rows > 1:
        ok[nan_row] = False
        assert bool(torch.isnan(want32[nan_row]).all()) and bool(torch.isnan(got[nan_row].float()).all())
        assert same_bits(got[zero_row], b.to(torch.bfloat16))                # LayerNorm of a constant row is the shift
    assert not bool(torch.isnan(got[ok].float()).any())
    assert same_bits(got[ok], want[ok]), (rows, d)
    assert same_bits(ops.layernorm_bf16(x, w, b)[ok], got[ok])               # a second launch


GEMM_M = (1, 32, 127, 129, 300)
GEMM_KN = ((256, 768), (256, 1024), (1024, 256), (256, 128))


def gemm_operands(K, N, dev):
    g = torch.Generator().manual_seed(10 * K + N)
    x = torch.randn(max(GEMM_M), K, generator=g)
    w = torch.randn(K, N, generator=g) * 0.05
    b = torch.randn(N, generator=g) * 0.1
    r = torch.randn(max(GEMM_M), N, generator=g)
    return x.to(dev), w.to(dev), b.to(dev), r.to(dev)


@pytest.mark.parametrize("K,N", GEMM_KN, ids=[f"K{K}-N{N}" for K, N in GEMM_KN])
def test_02_forward_gemm_with_a_bf16_a_operand(dev, K, N):
    """On A.to(bfloat16) the GEMM gives the bits of today's fp32-operand ops on A: none, residual, and GELU-keep (pre bit-identical,
    f = RN(old f)).  Rows do not depend on M: every smaller call equals the leading rows of the largest one."""
    from rag4dyg_amd import ops
    x, w, b, r = gemm_operands(K, N, dev)
    plane = ops.bf16_plane(w)
    big = None
    for M in sorted(GEMM_M, reverse=True):
        xm, rm = x[:M].contiguous(), r[:M].contiguous()
        xb = xm.to(torch.bfloat16)
        y0 = ops.conv1d_bf16_act(xb, plane, b, "none")
        assert y0.dtype == torch.float32 and same_bits(y0, ops.conv1d_bf16(xm, plane, b, "none")), ("none", M)
        assert same_bits(ops.conv1d_bf16_act(xb, plane, None, "none"), ops.conv1d_bf16(xm, plane, None, "none")), ("no bias", M)
        y1 = ops.conv1d_bf16_act(xb, plane, b, "residual", rm)
        assert same_bits(y1, ops.conv1d_bf16(xm, plane, b, "residual", rm)), ("residual", M)
        pre, f = ops.conv1d_bf16_act(xb, plane, b, "gelu_keep")
        pre_old, f_old = ops.conv1d_bf16_keep(xm, plane, b)
        assert f.dtype == torch.bfloat16 and same_bits(pre, pre_old) and same_bits(f, f_old.to(torch.bfloat16)), ("gelu_keep", M)
        if big is None:
            big = (y0, y1, pre, f)
        else:
            for got, ref in zip((y0, y1, pre, f), big):
                assert same_bits(got, ref[:M]), ("rows do not depend on M", M)


def test_02b_forward_gemm_reads_nothing_past_the_bf16_block(dev):
    """The A block sits at the END of an allocation whose tail is NaN-poisoned in a second layout: the result does not move."""
    from rag4dyg_amd import ops
    K, N, M = 256, 768, 129
    x, w, b, _r = gemm_operands(K, N, dev)
    plane = ops.bf16_plane(w)
    xb = x[:M].to(torch.bfloat16).contiguous()
    want = ops.conv1d_bf16_act(xb, plane, b, "none")
    buf = torch.full((M + 200, K), float("nan"), dtype=torch.bfloat16, device=dev)
    buf[:M] = xb
    assert same_bits(ops.conv1d_bf16_act(buf[:M], plane, b, "none"), want)


WG_M = (32, 33, 257, 545)
WG_IJ = ((256, 768), (256, 1024), (1024, 256))


@pytest.mark.parametrize("I,J", WG_IJ, ids=[f"I{I}-J{J}" for I, J in WG_IJ])
def test_03_weight_gradient_with_a_bf16_x_operand(dev, I, J):
    """dW and db equal r4d_weight_grad_bf16_f32 on the fp32 x bit for bit: one slice (M 32, 33) and several (257: 2, 545: 3), with
    and without db, given the same workspace; the workspace's content (every poison pattern) does not matter."""
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    for M in WG_M:
        g = torch.Generator().manual_seed(M * 7 + I + J)
        x = torch.randn(M, I, generator=g).to(dev)
        dy = (torch.randn(M, J, generator=g) * 1e-3).to(dev)
        xb = x.to(torch.bfloat16)
        dw_old, db_old = ops.weight_grad_bf16(x, dy)
        dw, db = ops.weight_grad_bf16_act(xb, dy)
        assert same_bits(dw, dw_old) and same_bits(db, db_old), (M, "with db")
        dw2, none = ops.weight_grad_bf16_act(xb, dy, want_db=False)
        assert none is None and same_bits(dw2, ops.weight_grad_bf16(x, dy, want_db=False)[0]) and same_bits(dw2, dw_old), (M, "without db")
        nbytes = int(lib.r4d_weight_grad_bf16_workspace_bytes(M, I, J))
        for pat in PATTERNS if (M, I) in ((545, 256), (33, 1024)) else ():
            ws = poison(torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev), pat)
            dwp, dbp = ops.weight_grad_bf16_act(xb, dy, workspace=ws)
            assert same_bits(dwp, dw_old) and same_bits(dbp, db_old), (M, pat)


def test_03b_weight_gradient_of_a_column_block(dev):
    """ldx > I: x is a column block of a wider bf16 buffer (and dy of a wider fp32 one)."""
    from rag4dyg_amd import _lib, ops
    M, I, J = 257, 256, 768
    g = torch.Generator().manual_seed(11)
    xw = torch.randn(M, I + 64, generator=g).to(dev)
    dyw = (torch.randn(M, 2 * J, generator=g) * 1e-3).to(dev)
    xbw = xw.to(torch.bfloat16)
    x, xb, dy = xw[:, 32:32 + I], xbw[:, 32:32 + I], dyw[:, J:2 * J]
    assert xb.stride(0) == I + 64 and dy.stride(0) == 2 * J
    dw_old, db_old = ops.weight_grad_bf16(x, dy)
    dw, db = ops.weight_grad_bf16_act(xb, dy)
    assert same_bits(dw, dw_old) and same_bits(db, db_old)
    with pytest.raises(_lib.R4DError, match=r"rc=-1"):                      # a row stride that is no multiple of 8 bf16
        ops.weight_grad_bf16_act(torch.zeros(M, I + 4, dtype=torch.bfloat16, device=dev)[:, :I], dy)


# ------------------------------------------------------------------------------------------------------------------ the steps
def model_of(dev, c):
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModelRAG
    sd, H = R.weights(c.weights)
    x = R.inputs(c)
    V, d = sd["transformer.wte.weight"].shape
    n_pos = sd["transformer.wpe.weight"].shape[0]
    m = GPT2LMHeadModelRAG(GPT2Config(vocab_size=V, n_positions=n_pos, n_ctx=n_pos, n_embd=d, n_layer=R.gpt2_ref.n_layers_of(sd), n_head=H))
    load_state_dict_checked(m, {k: v.clone() for k, v in sd.items()})
    m.tie_weights()
    if c.kind.startswith("gen"):
        gnn = m.get_gnn(d, d // 2, d, 1, 0.2)
        with torch.no_grad():
            gnn.convs[0].lin.weight.copy_(x["gcn_w"])
            gnn.convs[0].bias.copy_(x["gcn_b"])
        if c.kind == "gen":
            m.lm_head.weight = torch.nn.Parameter(x["head"].clone())
    return m.to(dev).eval()


def stepper(dev, c, precision, act_store, dropout=None, attention=None, activations=None, head_precision=None, seed=0, model=None):
    """(trainer, step() -> {"loss", "grads", "emb" / "hidden"} as device tensors) of one case"""
    from rag4dyg_amd import training
    from rag4dyg_amd.generator_training import GeneratorTrainer, PreparedBags
    from rag4dyg_amd.lm_training import LMTrainer
    m = model_of(dev, c) if model is None else model
    x = R.inputs(c)
    kw = dict(dropout=dropout, seed=seed, attention=attention, activations=activations, precision=precision, act_store=act_store)
    if c.kind == "enc":
        tr = training.EncoderTrainer(m, **kw)
        ids, G = [t.to(dev) for t in x["ids"]], x["G"].to(dev)

        def step():
            emb = tr.forward(ids)
            return {"loss": (emb.double() * G.double()).sum(), "grads": tr.backward(G), "emb": emb}
    elif c.kind == "lm":
        tr = LMTrainer(m, head_precision=head_precision, **kw)
        ids = x["ids"].to(dev)

        def step():
            return {"loss": tr.step(ids), "grads": tr.grads}
    else:
        kw["dropout"] = (0.0, 0.0, 0.0) if dropout is None else dropout
        tr = GeneratorTrainer(m, freeze=c.kind == "gen", head_precision=head_precision, **kw)
        tok = x["tok"].to(dev)
        bags = PreparedBags(x["idx"], x["src"], 7).batch(range(len(x["idx"])), dev)
        hidden = torch.empty(c.Bs[0], c.Ts[0], m.config.n_embd, device=dev)

        def step():
            return {"loss": tr.step(tok, bags, hidden_out=hidden), "grads": tr.grads, "hidden": hidden}
    return tr, step


def snapshot(out):
    """loss, mean pool / hidden_out and EVERY gradient tensor (the generator's: d_fused reaches the GCN gradients)"""
    s = {"grads:" + n: t.detach().clone() for n, t in out["grads"].items()}
    for k in ("loss", "emb", "hidden"):
        if out.get(k) is not None:
            s[k] = out[k].detach().clone()
    return s


def assert_same_bits(a, b, what):
    assert set(a) == set(b), what
    for n in a:
        assert same_bits(a[n], b[n]), (what, n)


def ws_of(tr):
    return tr._ws


STEP_CASES = [R.case(w, k) for w in ("L2_d256_T130", "L4_d512_T96") for k in R.KINDS]
DROP = (0.1, 0.1, 0.1)


@pytest.mark.parametrize("dropout", (None, DROP), ids=("nodrop", "drop"))
@pytest.mark.parametrize("c", STEP_CASES, ids=[R.case_id(c) for c in STEP_CASES])
def test_04_steps_keep_their_bits(dev, c, dropout):
    """Loss, mean pool / hidden_out and every gradient of three consecutive steps, store on against store off, under "bf16",
    "bf16+attn" and (where the step has a head) head_precision "bf16"; the store-on workspace is smaller by the formula."""
    L, d, M = (2, 256, R.rows_of(c)) if c.weights.startswith("L2") else (4, 512, R.rows_of(c))
    configs = [("bf16", None), ("bf16+attn", None)] + ([("bf16", "bf16")] if c.kind != "enc" else [])
    for precision, head in configs:
        runs = {}
        for store in ("fp32", "bf16"):
            tr, step = stepper(dev, c, precision, store, dropout=dropout, head_precision=head, seed=5)
            before = hits()
            runs[store] = ([snapshot(step()) for _ in range(3)], ws_of(tr).numel(), delta(before))
        for i in range(3):
            assert_same_bits(runs["fp32"][0][i], runs["bf16"][0][i], (precision, head, "step", i))
        if dropout is None:                                                  # no masks: the repeated steps are one step
            assert_same_bits(runs["bf16"][0][0], runs["bf16"][0][2], (precision, head, "repeat"))
        assert runs["fp32"][1] - runs["bf16"][1] == (12 * L - 2) * M * d, (runs["fp32"][1], runs["bf16"][1])
        assert runs["fp32"][2] == {"fwd": 0, "wgrad": 0, "ln": 0, "gelu": 0}
        frozen = c.kind == "gen"
        assert runs["bf16"][2] == {"fwd": 3 * (3 * L - 1), "wgrad": 0 if frozen else 3 * (3 * L - 1), "ln": 3 * (2 * L - 1), "gelu": 0}


def test_04c_gelu_fusion_off(dev):
    """R4D_TRAIN_FUSE_GELU=0 (read once per process: a child) sends f through the element-wise GELU launch, whose bf16-output form
    must leave the fused-off step's bits too."""
    env = dict(os.environ, R4D_TRAIN_FUSE_GELU="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "_act_bf16_fuse_child.py")], env=env, capture_output=True, text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    for kind in ("lm", "enc"):
        assert out[kind]["fp32"] == out[kind]["bf16"], (kind, out)
        assert out[kind]["gelu_launches"] == 2, out                          # one per layer of the L2 fixture


LM = R.case("L2_d256_T130", "lm")
ENC = R.case("L2_d256_T130", "enc")
GEN = R.case("L2_d256_T130", "gen")


@pytest.mark.parametrize("c", (ENC, LM, GEN), ids=("enc", "lm", "gen"))
def test_05_recompute_modes_give_the_same_bits(dev, c):
    """The four combinations of attention x activations with the store on give the bits of the stored step with the store off;
    the workspace shrinks by the mode's own formula."""
    L, d, M = 2, 256, R.rows_of(c)
    _t, step = stepper(dev, c, "bf16", "fp32", dropout=DROP, seed=5)
    base = snapshot(step())
    for attention in ("stored", "recompute"):
        for activations in ("stored", "recompute"):
            tr, step = stepper(dev, c, "bf16", "bf16", dropout=DROP, attention=attention, activations=activations, seed=5)
            assert_same_bits(base, snapshot(step()), (attention, activations))
            tr0, step0 = stepper(dev, c, "bf16", "fp32", dropout=DROP, attention=attention, activations=activations, seed=5)
            step0()
            want = (10 + 2) * M * d if activations == "recompute" else (12 * L - 2) * M * d
            assert ws_of(tr0).numel() - ws_of(tr).numel() == want, (attention, activations)


def test_06_fallback_and_branch_counts(dev):
    """d 64: the store changes neither bits nor workspace bytes and counts no branch.  d 256, L 2: per step 3 L - 1 forward GEMMs
    read a bf16 block (c_fc and the MLP projection of every layer, c_attn behind layer 0), as many weight gradients (none in the
    frozen step), 2 L - 1 LayerNorms write one; under activations recompute the backward forms layer 0's ln2 and f again."""
    c64 = R.case("L2_d64_T40", "lm")
    snaps, sizes = {}, {}
    before = hits()
    for store in ("fp32", "bf16"):
        tr, step = stepper(dev, c64, "bf16", store, dropout=DROP, seed=5)
        snaps[store] = snapshot(step())
        sizes[store] = ws_of(tr).numel()
    assert_same_bits(snaps["fp32"], snaps["bf16"], "d64")
    assert sizes["fp32"] == sizes["bf16"]
    assert delta(before) == {"fwd": 0, "wgrad": 0, "ln": 0, "gelu": 0}
    L = 2
    _t, step = stepper(dev, LM, "bf16", "bf16")
    b = hits(); step()
    assert delta(b) == {"fwd": 3 * L - 1, "wgrad": 3 * L - 1, "ln": 2 * L - 1, "gelu": 0}
    _t, step = stepper(dev, GEN, "bf16", "bf16")
    b = hits(); step()
    assert delta(b) == {"fwd": 3 * L - 1, "wgrad": 0, "ln": 2 * L - 1, "gelu": 0}
    _t, step = stepper(dev, LM, "bf16", "bf16", activations="recompute")
    b = hits(); step()
    assert delta(b) == {"fwd": 3 * L - 1 + 1, "wgrad": 3 * L - 1, "ln": 2 * L - 1 + 1, "gelu": 0}
    _t, step = stepper(dev, LM, "bf16", "fp32")
    b = hits(); step()
    assert delta(b) == {"fwd": 0, "wgrad": 0, "ln": 0, "gelu": 0}


def profile_counts(step):
    from rag4dyg_amd import _lib
    lib = _lib.load()
    _lib.check(lib.r4d_profile_enable(1), "profile_enable")
    try:
        step()
        torch.cuda.synchronize()
        out = {}
        for cls in range(lib.r4d_profile_num_classes()):
            ms, n, wk = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
            _lib.check(lib.r4d_profile_read(cls, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(wk)), "profile_read")
            if n.value:
                out[lib.r4d_profile_class_name(cls).decode()] = n.value
    finally:
        _lib.check(lib.r4d_profile_enable(0), "profile_enable")
    return out


@pytest.mark.parametrize("activations", ("stored", "recompute"))
def test_07_launch_accounting(dev, activations):
    """Per profile class an LM step with the store on launches exactly what it launches with the store off: no conversion launch."""
    counts = {}
    for store in ("fp32", "bf16"):
        _t, step = stepper(dev, LM, "bf16", store, dropout=DROP, activations=activations, seed=5)
        step()                                                               # (allocations and the derived weights: first call)
        counts[store] = profile_counts(step)
    print(f"[train_act_bf16] launches per class ({activations}): {counts['bf16']}")
    assert counts["fp32"] == counts["bf16"] and counts["bf16"].get("gemm_bf16_32", 0) > 0 and counts["bf16"].get("layernorm", 0) > 0, counts


@pytest.mark.parametrize("pattern", PATTERNS)
def test_08_poisoned_workspace(dev, pattern):
    """The workspace (bf16 halves and the alignment gaps behind them included) and every scratch buffer filled with the pattern
    before the step: the same bits.  Stored and activations-recompute layouts, all three trainers."""
    for c, activations in ((LM, "stored"), (LM, "recompute"), (ENC, "stored"), (GEN, "recompute")):
        tr, step = stepper(dev, c, "bf16", "bf16", dropout=DROP, activations=activations, seed=5)
        first = snapshot(step())
        getattr(tr, "enc", tr).step = 0                                      # the same dropout masks again
        poison(ws_of(tr), pattern)
        for buf in getattr(tr, "_scratch", {}).values():
            poison(buf, pattern)
        assert_same_bits(first, snapshot(step()), (R.case_id(c), activations, pattern))


def test_09a_backward_under_the_other_setting_is_refused(dev):
    from rag4dyg_amd import _lib, training
    x = R.inputs(ENC)
    ids, G = [t.to(dev) for t in x["ids"]], x["G"].to(dev)
    for first, second in (("bf16", "fp32"), ("fp32", "bf16")):
        tr = training.EncoderTrainer(model_of(dev, ENC), precision="bf16", act_store=first)
        tr.forward(ids)
        tr.act_store = second
        with pytest.raises(_lib.R4DError, match="train-act-bf16"):
            tr.backward(G)
        tr.act_store = first
        tr.forward(ids)
        tr.backward(G)                                                       # the matching pair goes through
    with pytest.raises(ValueError):
        training.EncoderTrainer(model_of(dev, ENC), precision="fp32", act_store="bf16")


def test_09b_a_layer_without_planes_is_refused_in_the_forward(dev):
    from rag4dyg_amd import _lib, training
    x = R.inputs(ENC)
    ids = [t.to(dev) for t in x["ids"]]
    tr = training.EncoderTrainer(model_of(dev, ENC), precision="bf16", act_store="bf16")
    tr._w3.pop((1, "c_fc_w"))                                               # layer 1's c_fc loses its planes
    with pytest.raises(_lib.R4DError, match="c_fc_w3"):
        tr.forward(ids)


def test_09c_isolation(dev):
    """Trainers of both settings alternate in one process and keep their bits; with the switch on and the layer switch off the fp32
    step's bits and bytes are untouched; the encoder's bf16 GEMM and an encoder forward under encode precision bf16 do not move."""
    from rag4dyg_amd import _lib, ops, retrieval
    lib = _lib.load()
    m = model_of(dev, LM)
    ids = R.inputs(LM)["ids"].to(dev)
    xg, wg, bg, _r = gemm_operands(256, 768, dev)
    plane = ops.bf16_plane(wg)

    def encoder_bits():
        was = ops.set_encode_precision("bf16")
        try:
            return (ops.conv1d_bf16(xg[:129].contiguous(), plane, bg, "gelu").clone(), m.transformer(input_ids=ids)[0].clone(),
                    retrieval.encode_batches(m, [ids, ids[:2, :57].contiguous()]).clone())
        finally:
            ops.set_encode_precision(was)
    h0 = encoder_bits()
    tr32, step32 = stepper(dev, LM, "fp32", "fp32", model=m)
    g32 = snapshot(step32())
    bytes32 = ws_of(tr32).numel()
    _t, step_off = stepper(dev, LM, "bf16", "fp32", model=m)
    _t, step_on = stepper(dev, LM, "bf16", "bf16", model=m)
    off = snapshot(step_off())
    for _ in range(2):                                                       # alternate
        assert_same_bits(off, snapshot(step_on()), "store on")
        assert lib.r4d_get_train_act_bf16() == 1
        assert_same_bits(off, snapshot(step_off()), "store off")
        assert lib.r4d_get_train_act_bf16() == 0
    for a, b in zip(h0, encoder_bits()):
        assert same_bits(a, b)
    # the store switch on with the layer switch off (past the constructor's pairing check): nothing may change
    before = hits()
    tr32.enc.act_store = "bf16"
    tr32._ws = None
    assert_same_bits(g32, snapshot(step32()), "fp32 step with the store switch on")
    assert lib.r4d_get_train_act_bf16() == 1 and lib.r4d_get_train_bf16() == 0
    assert ws_of(tr32).numel() == bytes32
    assert delta(before) == {"fwd": 0, "wgrad": 0, "ln": 0, "gelu": 0}
    for a, b in zip(h0, encoder_bits()):                                     # ... and with the switch still on
        assert same_bits(a, b)


def test_10_thirty_adamw_steps_end_on_the_same_parameters(dev):
    """30 AdamW steps of LMTrainer (L2 d256, B 8, T 40, dropout 0.1): the store-on run ends on the store-off run's parameters."""
    from rag4dyg_amd import training
    from rag4dyg_amd.lm_training import LMTrainer
    V = R.weights(LM.weights)[0]["transformer.wte.weight"].shape[0]
    ids = torch.randint(0, V - 2, (8, 40), generator=torch.Generator().manual_seed(77)).to(dev)
    end = {}
    for store in ("fp32", "bf16"):
        tr = LMTrainer(model_of(dev, LM).train(), dropout=DROP, seed=3, precision="bf16", act_store=store)
        opt = training.AdamW(tr.params, tr.grads, lr=1e-3, weight_decay=0.01, flat_grads=tr.flat_grads)
        losses = []
        for _ in range(30):
            losses.append(tr.step(ids))
            opt.step(max_grad_norm=1.0)
        end[store] = ({n: p.detach().clone() for n, p in tr.params.items()}, torch.stack(losses).clone())
    assert same_bits(end["fp32"][1], end["bf16"][1])
    assert float(end["bf16"][1][-1]) < float(end["bf16"][1][0])
    assert_same_bits(end["fp32"][0], end["bf16"][0], "parameters after 30 steps")
