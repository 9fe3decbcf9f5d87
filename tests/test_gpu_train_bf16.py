"""The training steps' opt-in bf16 precision on the GPU (``precision="bf16"`` of the three trainers, ``r4d_set_train_bf16``,
csrc/gemm_b1.hip, csrc/gemm_b1tn.hip): the three single ops against float64 of the bf16-rounded operands at derived bounds, the
steps against the EXACT float64 oracle inside the margin the two emulations of tests/_train_bf16_ref.py give, the isolation of
everything the switch must not touch, the recompute modes, the launch accounting, the refusals, and a short training run.

Every test restores the switches it found."""
import pytest
import torch

import _train_modes
import _train_bf16_ref as R
from _poison import PATTERNS, poison
from conftest import load_state_dict_checked

pytestmark = pytest.mark.gpu

BRANCH_PREFIX = "tuning:train_bf16:"
EPILOGUE_TOL = 1e-5      # tests/test_gpu_encode_bf16.py: the epilogue term of the GELU / residual kinds (max-norm, relative)
GELU_SLOPE = 1.13        # max |d gelu_new / dx| = 1.1290
GRID_M, GRID_K, GRID_N = (1, 129, 300), (32, 96, 512), (64, 200, 256)
WIDE = (4000, 96, 1500)  # the 128 x 256 tile (the grid above goes to 128 x 128 by the project's tile rule)
GRID = [(M, K, N) for M in GRID_M for K in GRID_K for N in GRID_N] + [WIDE]


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


def delta(before):
    return {n: v - before[n] for n, v in hits().items()}


def operands(M, K, N, dev, seed=0):
    g = torch.Generator().manual_seed(1000 * M + 10 * K + N + seed)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(K, N, generator=g) * 0.05
    b = torch.randn(N, generator=g) * 0.1
    r = torch.randn(M, N, generator=g)
    return x.to(dev), w.to(dev), b.to(dev), r.to(dev)


def gelu_new_grad64(u):
    u = u.detach().clone().requires_grad_(True)
    R.gpt2_ref.gelu_new(u).sum().backward()
    return u.grad


# --------------------------------------------------------------------------------------------------------- the single ops
def test_01_c_fc_forward_keeps_the_pre_activation(dev):
    """|pre - y64| <= (K + 2) 2^-24 (|x^| |w^|^T + |b|) (bf16 x bf16 is exact in fp32: the roundings are the accumulation's and the
    bias add's); the GELU output at 1.13 x that plus the epilogue term.  Both outputs carry the bits of the encoder's single op."""
    from rag4dyg_amd import ops
    worst = 0.0
    for (M, K, N) in GRID:
        x, w, b, _r = operands(M, K, N, dev)
        plane = ops.bf16_plane(w)
        xh, wh = x.bfloat16().double(), w.bfloat16().double()
        y64 = xh @ wh + b.double()
        bound = (K + 2) * 2.0 ** -24 * (xh.abs() @ wh.abs() + b.abs().double())
        pre, y = ops.conv1d_bf16_keep(x, plane, b)
        g64 = R.gpt2_ref.gelu_new(y64)
        e_pre = float(((pre.double() - y64).abs() / bound).max())
        e_y = float(((y.double() - g64).abs() / (GELU_SLOPE * bound + EPILOGUE_TOL * g64.abs().max())).max())
        worst = max(worst, e_pre, e_y)
        assert e_pre <= 1.0 and e_y <= 1.0, f"M={M} K={K} N={N}: |error| / bound (pre, gelu) = {e_pre}, {e_y}"
        assert torch.equal(pre, ops.conv1d_bf16(x, plane, b, "none")) and torch.equal(y, ops.conv1d_bf16(x, plane, b, "gelu")), (M, K, N)
    print(f"conv1d_bf16_keep: {len(GRID)} shapes, largest |error| / bound {worst:.3f}")


def test_02_data_gradient_none_residual_and_gelu_derivative(dev):
    """dx [M, in] = bf16(dy [M, out]) . bf16(W [in, out])^T: the grid's K is the contracted ``out``, its N the ``in``."""
    from rag4dyg_amd import ops
    worst = 0.0
    for (M, K, N) in GRID:
        dy, wt, _b, second = operands(M, K, N, dev)                       # wt [out, in] = W^T; second [M, in]
        W = wt.t().contiguous()                                           # the Conv1D weight [in, out]
        plane_t = ops.bf16_plane(W, transposed=True)                      # [in][out]: plane 0 of a trainer's _w3t
        assert plane_t.shape == (N, K)
        dh, wh = dy.bfloat16().double(), wt.bfloat16().double()
        v64 = dh @ wh
        bound = (K + 2) * 2.0 ** -24 * (dh.abs() @ wh.abs())
        dx = ops.conv1d_bf16_dgrad(dy, plane_t)
        e0 = float(((dx.double() - v64).abs() / bound).max())
        assert torch.equal(dx, ops.conv1d_bf16(dy, plane_t, None)), (M, K, N)
        r64 = v64 + second.double()
        dxr = ops.conv1d_bf16_dgrad(dy, plane_t, "residual", second)
        e1 = float(((dxr.double() - r64).abs() / (bound + EPILOGUE_TOL * r64.abs().max())).max())
        gp = gelu_new_grad64(second.double())
        g64 = v64 * gp
        dxg = ops.conv1d_bf16_dgrad(dy, plane_t, "gelu_grad", second)
        e2 = float(((dxg.double() - g64).abs() / (GELU_SLOPE * bound + EPILOGUE_TOL * g64.abs().max())).max())
        worst = max(worst, e0, e1, e2)
        assert max(e0, e1, e2) <= 1.0, f"M={M} out={K} in={N}: |error| / bound (none, residual, gelu') = {e0}, {e1}, {e2}"
    print(f"conv1d_bf16_dgrad: {len(GRID)} shapes, largest |error| / bound {worst:.3f}")


@pytest.mark.parametrize("kind", ("none", "residual", "gelu_grad"))
def test_02b_data_gradient_rows_do_not_depend_on_the_call(dev, kind):
    from rag4dyg_amd import ops
    dy, wt, _b, second = operands(300, 512, 256, dev)
    plane_t = ops.bf16_plane(wt.t().contiguous(), transposed=True)

    def run(lo, hi):
        return ops.conv1d_bf16_dgrad(dy[lo:hi].contiguous(), plane_t, kind, second[lo:hi].contiguous() if kind != "none" else None)
    y300 = run(0, 300)
    assert torch.equal(run(0, 1), y300[0:1]) and torch.equal(run(299, 300), y300[299:300])
    assert torch.equal(run(0, 129), y300[:129]) and torch.equal(run(171, 300), y300[171:])


def _wgrad_check(x, dy, dev, workspace=None):
    from rag4dyg_amd import ops
    M, I = x.shape
    J = dy.shape[1]
    dw, db = ops.weight_grad_bf16(x, dy, workspace=workspace)
    xh, dh = x.bfloat16().double(), dy.bfloat16().double()
    S = (M + 255) // 256                                                  # no more slices than that (8 k-tiles each at least)
    w64 = xh.t() @ dh
    e_w = float(((dw.double() - w64).abs() / ((M + S + 2) * 2.0 ** -24 * (xh.abs().t() @ dh.abs()))).max())
    e_b = float(((db.double() - dy.double().sum(0)).abs() / ((M + 2) * 2.0 ** -24 * dy.double().abs().sum(0))).max())
    return dw, db, e_w, e_b


@pytest.mark.parametrize("M", (32, 33, 95, 390, 4100))
def test_03_weight_gradient(dev, M):
    """dW against float64 of the rounded operands within (M + S + 2) 2^-24 |x^|^T |dy^| (M products in fp32, S slice sums), db
    against the float64 column sums of the UNROUNDED dy within (M + 2) 2^-24 sum |dy|.  The operands are allocated at their
    exact size.  A second run and every poisoned workspace give the same bits."""
    from rag4dyg_amd import _lib
    lib = _lib.load()
    for I in (128, 256, 1024):
        for J in (256, 768):
            g = torch.Generator().manual_seed(M * 7 + I + J)
            x = torch.randn(M, I, generator=g).to(dev)
            dy = (torch.randn(M, J, generator=g) * 1e-3).to(dev)
            dw, db, e_w, e_b = _wgrad_check(x, dy, dev)
            assert e_w <= 1.0 and e_b <= 1.0, f"M={M} I={I} J={J}: |error| / bound (dW, db) = {e_w}, {e_b}"
            dw2, db2, _, _ = _wgrad_check(x, dy, dev)
            assert torch.equal(dw, dw2) and torch.equal(db, db2), (M, I, J, "second run")
            if (I, J) in ((128, 256), (1024, 768)):
                nbytes = lib.r4d_weight_grad_bf16_workspace_bytes(M, I, J)
                for pat in PATTERNS:
                    ws = poison(torch.empty(int(nbytes), dtype=torch.uint8, device=dev), pat)
                    dwp, dbp, _, _ = _wgrad_check(x, dy, dev, workspace=ws)
                    assert torch.equal(dw, dwp) and torch.equal(db, dbp), (M, I, J, pat)


def test_03b_weight_gradient_of_column_blocks_and_refusals(dev):
    from rag4dyg_amd import _lib, ops
    M, I, J = 390, 256, 256
    g = torch.Generator().manual_seed(9)
    xw = torch.randn(M, I + 64, generator=g).to(dev)
    dyw = (torch.randn(M, 3 * J, generator=g) * 1e-3).to(dev)
    x, dy = xw[:, 32:32 + I], dyw[:, J:2 * J]                              # lda > I, ldb > J
    assert x.stride(0) == I + 64 and dy.stride(0) == 3 * J
    dw, db, e_w, e_b = _wgrad_check(x, dy, dev)
    assert e_w <= 1.0 and e_b <= 1.0, (e_w, e_b)
    dwc, dbc = ops.weight_grad_bf16(x.contiguous(), dy.contiguous())
    assert torch.equal(dw, dwc) and torch.equal(db, dbc)
    before = hits()
    for bad_i, bad_j, bad_m in ((64, 256, 390), (128, 192, 390), (128, 256, 31)):
        with pytest.raises(_lib.R4DError, match=r"rc=-1"):                 # R4D_ERR_INVALID
            ops.weight_grad_bf16(torch.zeros(bad_m, bad_i, device=dev), torch.zeros(bad_m, bad_j, device=dev))
    assert hits() == before


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


def stepper(dev, c, precision, dropout=None, attention=None, activations=None, freeze=None, seed=0, model=None):
    """(trainer, step() -> {"loss", "grads", "emb" / "hidden"} as device tensors) of one case"""
    from rag4dyg_amd import training
    from rag4dyg_amd.generator_training import GeneratorTrainer, PreparedBags
    from rag4dyg_amd.lm_training import LMTrainer
    m = model_of(dev, c) if model is None else model
    x = R.inputs(c)
    kw = dict(dropout=dropout, seed=seed, attention=attention, activations=activations, precision=precision)
    if c.kind == "enc":
        tr = training.EncoderTrainer(m, **kw)
        ids, G = [t.to(dev) for t in x["ids"]], x["G"].to(dev)

        def step():
            emb = tr.forward(ids)
            return {"loss": (emb.double() * G.double()).sum(), "grads": tr.backward(G), "emb": emb}
    elif c.kind == "lm":
        tr = LMTrainer(m, **kw)
        ids = x["ids"].to(dev)

        def step():
            return {"loss": tr.step(ids), "grads": tr.grads}
    else:
        kw["dropout"] = (0.0, 0.0, 0.0) if dropout is None else dropout
        tr = GeneratorTrainer(m, freeze=(c.kind == "gen") if freeze is None else freeze, **kw)
        tok = x["tok"].to(dev)
        bags = PreparedBags(x["idx"], x["src"], 7).batch(range(len(x["idx"])), dev)
        hidden = torch.empty(c.Bs[0], c.Ts[0], m.config.n_embd, device=dev)

        def step():
            return {"loss": tr.step(tok, bags, hidden_out=hidden), "grads": tr.grads, "hidden": hidden}
    return tr, step


def snapshot(out):
    s = {"grads:" + n: t.detach().clone() for n, t in out["grads"].items()}
    for k in ("loss", "emb", "hidden"):
        if out.get(k) is not None:
            s[k] = out[k].detach().clone()
    return s


def assert_same_bits(a, b, what):
    assert set(a) == set(b), what
    for n in a:
        assert torch.equal(a[n], b[n]), (what, n)


@pytest.mark.parametrize("c", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_04_step_against_the_exact_oracle_inside_the_emulations_margin(dev, c):
    """For every quantity whose float64 emulation is >= 1e-4 from exact:  e_emu64 / K <= e_gpu <= K max(e_emu32, e_emu64), all
    three errors taken against the EXACT float64 step.  The lower side shows the arithmetic is bf16's (the default's error is
    1e-6 there); K comes from the two emulations alone (test_host_train_bf16.py::test_margin_table).  The d 64 fixture's weight
    gradients fall back to the default kernel on the device and stay exact in the emulation."""
    K = R.margin()
    exact = R.references(c)[0]
    tab = R.error_table(c)
    _tr, step = stepper(dev, c, "bf16")
    before = hits()
    out = step()
    d_ = delta(before)
    got = {"loss": float(out["loss"]), "grads": {n: t.detach().cpu().double().numpy() for n, t in out["grads"].items()}}
    for k in ("emb", "hidden"):
        if out.get(k) is not None:
            got[k] = out[k].detach().cpu().double().numpy()
    assert set(got["grads"]) == set(exact["grads"])
    e = R.errors(got, exact)
    assert set(e) == set(tab)
    bad, n_gated = {}, 0
    for n, t in tab.items():
        gated = t["emu64"] >= R.GATE_FLOOR
        n_gated += gated
        lo, hi = t["emu64"] / K, K * max(t["emu32"], t["emu64"])
        print(f"[train_bf16] {R.case_id(c)} {n}: e_gpu {e[n]:.3e} emu64 {t['emu64']:.3e} emu32 {t['emu32']:.3e}" + ("" if gated else " (not gated)"))
        if gated and not lo <= e[n] <= hi:
            bad[n] = (lo, e[n], hi)
    print(f"[train_bf16] {R.case_id(c)}: K {K:.2f}, {n_gated} gated quantities, launches {d_}")
    assert c.weights in R.GATED
    assert not bad, f"{R.case_id(c)}: (e_emu64 / K, e_gpu, K max(e_emu32, e_emu64)) outside the gate: {bad}"
    assert d_["fwd"] > 0 and d_["dgrad"] > 0
    if c.weights == "L2_d64_T40" and c.kind != "gen":
        assert d_["wgrad"] == 0 and d_["wgrad_fallback"] > 0


LM = R.case("L2_d256_T130", "lm")
ENC = R.case("L2_d256_T130", "enc")
GEN = R.case("L2_d256_T130", "gen")


def test_05_isolation(dev):
    """Default precision never runs a bf16 training launch; its bits before the mode was ever on and after it went off are the
    same; the train switch leaves the encoder's bits alone and the encode switch a training step's."""
    from rag4dyg_amd import _lib, ops, retrieval
    lib = _lib.load()
    m = model_of(dev, LM)
    ids = R.inputs(LM)["ids"].to(dev)

    def encoder_bits():                                                     # forward() and the retrieval encode loop
        return m.transformer(input_ids=ids)[0].clone(), retrieval.encode_batches(m, [ids, ids[:2, :57].contiguous()]).clone()
    before = hits()
    _t, step32 = stepper(dev, LM, "fp32", model=m)
    g0 = snapshot(step32())
    _t, step_e = stepper(dev, ENC, "fp32")
    e0 = snapshot(step_e())
    assert delta(before) == {"fwd": 0, "dgrad": 0, "wgrad": 0, "wgrad_fallback": 0}
    h0 = encoder_bits()
    _t, step16 = stepper(dev, LM, "bf16", model=m)
    g1 = snapshot(step16())
    assert lib.r4d_get_train_bf16() == 1
    assert not torch.equal(g0["loss"], g1["loss"]) or not torch.equal(g0["grads:transformer.wpe.weight"], g1["grads:transformer.wpe.weight"])
    h1 = encoder_bits()                                                     # with the TRAIN switch on
    assert torch.equal(h0[0], h1[0]) and torch.equal(h0[1], h1[1])
    assert_same_bits(g0, snapshot(step32()), "default precision after bf16")
    assert lib.r4d_get_train_bf16() == 0
    assert_same_bits(e0, snapshot(step_e()), "default precision (enc) after bf16")
    was = ops.set_encode_precision("bf16")                                                  # the ENCODE switch and a training step
    try:
        assert_same_bits(g0, snapshot(step32()), "fp32 training under encode bf16")
        assert_same_bits(g1, snapshot(step16()), "bf16 training under encode bf16")
    finally:
        ops.set_encode_precision(was)


@pytest.mark.parametrize("c", (ENC, LM, GEN), ids=("enc", "lm", "gen"))
def test_06_recompute_modes_give_the_same_bits(dev, c):
    base = None
    for attention in ("stored", "recompute"):
        for activations in ("stored", "recompute"):
            _t, step = stepper(dev, c, "bf16", dropout=(0.1, 0.1, 0.1), attention=attention, activations=activations, seed=5)
            s = snapshot(step())
            if base is None:
                base = s
            else:
                assert_same_bits(base, s, (attention, activations))


def test_06b_frozen_generator_step_equals_the_unfrozen_steps_bits(dev):
    m = model_of(dev, GEN)                                                   # untied head
    _t, frozen = stepper(dev, GEN, "bf16", dropout=(0.1, 0.1, 0.1), freeze=True, seed=5, model=m)
    f = snapshot(frozen())
    _t, free = stepper(dev, GEN, "bf16", dropout=(0.1, 0.1, 0.1), freeze=False, seed=5, model=m)
    u = snapshot(free())
    assert {"loss", "hidden", "grads:lm_head.weight", "grads:gnn_fusion.convs.0.lin.weight", "grads:gnn_fusion.convs.0.bias"} <= set(f)
    for n in f:
        assert torch.equal(f[n], u[n]), n


def test_07_launch_accounting(dev):
    """12 L bf16 launches per unfrozen step (4 forward, 4 data-gradient, 4 weight-gradient GEMMs per block), 8 L per frozen one,
    3 (L - 1) more forward launches under activation recompute directly behind the forward; d 64: every weight gradient falls back."""
    L = 2
    _t, step = stepper(dev, LM, "bf16")
    b = hits(); step()
    assert delta(b) == {"fwd": 4 * L, "dgrad": 4 * L, "wgrad": 4 * L, "wgrad_fallback": 0}
    _t, step = stepper(dev, GEN, "bf16")
    b = hits(); step()
    assert delta(b) == {"fwd": 4 * L, "dgrad": 4 * L, "wgrad": 0, "wgrad_fallback": 0}
    _t, step = stepper(dev, LM, "bf16", activations="recompute")
    b = hits(); step()
    assert delta(b) == {"fwd": 4 * L + 3 * (L - 1), "dgrad": 4 * L, "wgrad": 4 * L, "wgrad_fallback": 0}
    c4 = R.case("L4_d512_T96", "enc")
    _t, step = stepper(dev, c4, "bf16", activations="recompute")
    b = hits(); step()
    assert delta(b) == {"fwd": 4 * 4 + 3 * 3, "dgrad": 16, "wgrad": 16, "wgrad_fallback": 0}
    _t, step = stepper(dev, R.case("L2_d64_T40", "lm"), "bf16")
    b = hits(); step()
    assert delta(b) == {"fwd": 4 * L, "dgrad": 4 * L, "wgrad": 0, "wgrad_fallback": 4 * L}


def test_08_refusals(dev, monkeypatch):
    from rag4dyg_amd import _lib, training
    from rag4dyg_amd.lm_training import LMTrainer
    x = R.inputs(ENC)
    ids, G = [t.to(dev) for t in x["ids"]], x["G"].to(dev)
    for first, second in (("bf16", "fp32"), ("fp32", "bf16")):
        tr = training.EncoderTrainer(model_of(dev, ENC), precision=first)
        tr.forward(ids)
        tr.precision = second
        with pytest.raises(_lib.R4DError, match="train-bf16"):
            tr.backward(G)
        tr.precision = first
        tr.forward(ids)
        tr.backward(G)                                                     # the matching pair goes through
    m = model_of(dev, LM)
    for bad in ("fp16", "BF16", "half"):
        with pytest.raises(ValueError):
            LMTrainer(m, precision=bad)
        with pytest.raises(ValueError):
            training.EncoderTrainer(m, precision=bad)
    monkeypatch.setenv("R4D_TRAIN_PRECISION", "fp16")
    with pytest.raises(ValueError):
        LMTrainer(m)
    monkeypatch.setenv("R4D_TRAIN_PRECISION", "bf16")
    assert LMTrainer(m).enc.precision == "bf16"


def test_09_gemm_mode_f32_with_bf16_precision(dev):
    from rag4dyg_amd import ops
    ops.set_gemm_mode("f32")
    tr32, _s = stepper(dev, LM, "fp32")
    assert not tr32.enc.use_s3 and not tr32.enc._w3 and not tr32.enc._w3t          # the default keeps no planes in this mode
    tr, step = stepper(dev, LM, "bf16")
    assert not tr.enc.use_s3 and len(tr.enc._w3) == 8 and len(tr.enc._w3t) == 8
    b = hits()
    out = step()
    assert delta(b) == {"fwd": 8, "dgrad": 8, "wgrad": 8, "wgrad_fallback": 0}
    e = R.errors({"loss": float(out["loss"]), "grads": {n: t.cpu().double().numpy() for n, t in out["grads"].items()}}, R.references(LM)[0])
    tab, K = R.error_table(LM), R.margin()
    bad = {n: e[n] for n, t in tab.items() if t["emu64"] >= R.GATE_FLOOR and not t["emu64"] / K <= e[n] <= K * max(t["emu32"], t["emu64"])}
    assert not bad, bad


def test_10_a_short_training_run(dev):
    """30 AdamW steps of LMTrainer on L2 d256, B 8, T 40, the same seed in fp32 and bf16: the bf16 loss falls; the difference of
    the final losses is recorded (printed), not gated."""
    from rag4dyg_amd import training
    from rag4dyg_amd.lm_training import LMTrainer
    c = R.case("L2_d256_T130", "lm")
    V = R.weights(c.weights)[0]["transformer.wte.weight"].shape[0]
    ids = torch.randint(0, V - 2, (8, 40), generator=torch.Generator().manual_seed(77)).to(dev)
    losses = {}
    for precision in ("fp32", "bf16"):
        tr = LMTrainer(model_of(dev, c).train(), dropout=(0.1, 0.1, 0.1), seed=3, precision=precision)
        opt = training.AdamW(tr.params, tr.grads, lr=1e-3, weight_decay=0.01, flat_grads=tr.flat_grads)
        ls = []
        for _ in range(30):
            ls.append(tr.step(ids))
            opt.step(max_grad_norm=1.0)
        losses[precision] = [float(v) for v in torch.stack(ls).cpu()]
    a, b = losses["fp32"], losses["bf16"]
    print(f"[train_bf16] 30 steps: fp32 {a[0]:.4f} -> {a[-1]:.4f}, bf16 {b[0]:.4f} -> {b[-1]:.4f}, final difference {abs(a[-1] - b[-1]):.2e}")
    assert all(v == v for v in b) and b[-1] < b[0], b
