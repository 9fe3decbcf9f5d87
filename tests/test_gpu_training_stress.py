"""GPU tests of the three training steps (retriever ``EncoderTrainer``, SimpleDyG ``LMTrainer``, RAG ``GeneratorTrainer``) under
TRAINED-MODEL STATISTICS and LONG sequences -- the stressed / sharpened weight sets of the inference fixtures G10 / G11 / G13,
saturated GELU pre-activations, T up to 1024 -- and of the backward kernels at their edges.

Every gradient is held against float64 autograd of the oracle twice: by the absolute caps of the existing step tests (where
the float32 reference alone leaves room for them) and by the YARDSTICK bound  e_dev <= K * max(e_ref, 2e-6)  per parameter
tensor, e = max |g - g64| / max |g64| and e_ref the same calculus in float32 on the CPU under the CPU's summation orders.  The
case table, K and the oracles live in ``_training_stress_cases.py``; ``test_host_training_stress.py`` checks them on the CPU.
Run with ``-s`` for the e_dev / e_ref table (profiles/train_stress_parity.md)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _training_stress_cases as C
from conftest import GEMM_MODES, REPO, elementwise_err, load_state_dict_checked, rel_err

pytestmark = pytest.mark.gpu

# every float of the pre-set workspace is a NaN (0xFFFFFFFF): a step that reads a word it has not written -- a pad column of a
# transposed operand, a row of the next head -- cannot multiply it away, and the tail behind the library's layout shows a write
PATTERN, TAIL = 0xFF, 4096

# (entry id, arithmetic) -> tensor names exempt from the yardstick bound: a documented property of that arithmetic, with the
# evidence in profiles/train_stress_parity.md.  At most two cells, none under "f32".
EXEMPT = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------------ the steps
def _model(dev, e):
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModelRAG
    from oracle import gpt2_ref
    sd, H = C.weights(e.weights)
    x = C.inputs(e)
    V, d = sd["transformer.wte.weight"].shape
    n_pos = sd["transformer.wpe.weight"].shape[0]
    m = GPT2LMHeadModelRAG(GPT2Config(vocab_size=V, n_positions=n_pos, n_ctx=n_pos, n_embd=d, n_layer=gpt2_ref.n_layers_of(sd), n_head=H))
    load_state_dict_checked(m, {k: v.clone() for k, v in sd.items()})
    m.tie_weights()
    if e.kind.startswith("gen"):
        gnn = m.get_gnn(d, d // 2, d, 1, 0.2)
        with torch.no_grad():
            gnn.convs[0].lin.weight.copy_(x["gcn_w"])
            gnn.convs[0].bias.copy_(x["gcn_b"])
        if e.kind == "gen":
            m.lm_head.weight = torch.nn.Parameter(x["head"].clone())
    return m.to(dev).eval()


def _guarded_workspace(nbytes, dev):
    """The trainer's workspace, TAIL bytes larger than the library asks for and filled with the byte pattern: the trainers keep a
    buffer that is large enough, so whatever the step writes beyond its own layout shows in the tail."""
    assert nbytes > 0
    return torch.full((int(nbytes) + TAIL,), PATTERN, dtype=torch.uint8, device=dev)


def _stepper(dev, e):
    """(step() -> {"loss", "grads", "emb" / "hidden"}, tail_intact() -> bool) of one entry on the device."""
    from rag4dyg_amd import _lib, training
    from rag4dyg_amd.generator_training import GeneratorTrainer, PreparedBags
    from rag4dyg_amd.lm_training import LMTrainer
    lib = _lib.load()
    m = _model(dev, e)
    x = C.inputs(e)
    if e.kind == "enc":
        tr = training.EncoderTrainer(m)
        ids = [t.to(dev) for t in x["ids"]]
        G = x["G"].to(dev)
        n = len(ids)
        cfg = tr._structs()[0]
        nbytes = lib.r4d_gpt2_train_workspace_bytes(ctypes.byref(cfg), n, (ctypes.c_int32 * n)(*e.Bs), (ctypes.c_int32 * n)(*e.Ts))
        tr._ws = _guarded_workspace(nbytes, dev)

        def step():
            emb = tr.forward(ids)
            grads = tr.backward(G)
            return {"loss": None, "grads": grads, "emb": emb}
    elif e.kind == "lm":
        tr = LMTrainer(m)
        ids = x["ids"].to(dev)
        cfg = tr.enc._structs()[0]
        nbytes = lib.r4d_gpt2_lm_train_workspace_bytes(ctypes.byref(cfg), e.Bs[0], e.Ts[0], tr.ldV)
        tr._ws = _guarded_workspace(nbytes, dev)

        def step():
            return {"loss": tr.step(ids), "grads": tr.grads}
    else:
        freeze = e.kind == "gen"
        tr = GeneratorTrainer(m, freeze=freeze, dropout=(0.0, 0.0, 0.0))
        if freeze:
            assert set(tr.params) == {"lm_head.weight", "gnn_fusion.convs.0.lin.weight", "gnn_fusion.convs.0.bias"}
        tok = x["tok"].to(dev)
        bags = PreparedBags(x["idx"], x["src"], 7).batch(range(len(x["idx"])), dev)
        cfg = tr.enc._structs()[0]
        nbytes = lib.r4d_rag_train_workspace_bytes(ctypes.byref(cfg), e.Bs[0], e.Ts[0], tr.ldV)
        tr._ws = _guarded_workspace(nbytes, dev)
        hidden = torch.empty(e.Bs[0], e.Ts[0], m.config.n_embd, device=dev)

        def step():
            return {"loss": tr.step(tok, bags, hidden_out=hidden), "grads": tr.grads, "hidden": hidden}

    def tail_intact():
        return tr._ws.numel() == int(nbytes) + TAIL and bool((tr._ws[int(nbytes):] == PATTERN).all())
    return step, tail_intact


def measure(dev, e):
    """One step of an entry on the device against its reference profile.  Returns the measures (nothing asserted) and the
    step / tail closures."""
    p = C.reference_profile(e)
    step, tail_intact = _stepper(dev, e)
    out = step()
    got = {n: t.detach().cpu().double().numpy() for n, t in out["grads"].items()}
    r = {"p": p, "out": out, "step": step, "tail_intact": tail_intact, "names_equal": set(got) == set(p.ref64["grads"])}
    r["loss_dev"] = None if out["loss"] is None else float(out["loss"])
    r["finite"] = all(np.isfinite(g).all() for g in got.values()) and (r["loss_dev"] is None or np.isfinite(r["loss_dev"]))
    if not r["names_equal"] or not r["finite"]:
        return r
    ref = p.ref64["grads"]
    r["e_dev"] = C.max_norm_errs(got, ref)
    r["ew"] = {n: elementwise_err(got[n], ref[n], rtol=C.EW_RTOL, atol=C.EW_ATOL) for n in ref}
    r["ratio"] = {n: r["e_dev"][n] / max(p.e_ref[n], C.E_FLOOR) for n in ref}
    r["loss_err"] = None if r["loss_dev"] is None else abs(r["loss_dev"] / p.ref64["loss"] - 1)
    key = "emb" if "emb" in out else "hidden" if "hidden" in out else None
    r["hidden_err"] = None if key is None else rel_err(out[key].cpu().numpy(), p.ref64[key])
    return r


def assert_bounds(e, mode, r, only=None, caps=None):
    """The caps the entry carries and the yardstick bound, on every tensor (or those whose name contains one of ``only``)."""
    caps = e.caps if caps is None else caps
    assert r["names_equal"] and r["finite"], (C.entry_id(e), mode, r["names_equal"], r["finite"])
    pick = [n for n in r["e_dev"] if only is None or any(o in n for o in only)]
    assert pick
    worst = max(pick, key=lambda n: r["ratio"][n])
    print(f"[stress] {C.entry_id(e)} | {mode} | e_dev/e_ref worst {r['ratio'][worst]:.2f} ({worst}: {r['e_dev'][worst]:.2e} vs "
          f"{r['p'].e_ref[worst]:.2e}) | max-norm {max(r['e_dev'][n] for n in pick):.2e} (ref {max(r['p'].e_ref[n] for n in pick):.2e}) | "
          f"element-wise {max(r['ew'][n] for n in pick):.3f} (ref {r['p'].ew_ref:.3f}) | loss {r['loss_err']} | emb/hidden {r['hidden_err']}")
    if r["loss_err"] is not None:
        assert r["loss_err"] < C.LOSS_CAP, (r["loss_dev"], r["p"].ref64["loss"])
    assert max(r["e_dev"][n] for n in pick) < C.NORM_CAP, {n: r["e_dev"][n] for n in pick if r["e_dev"][n] >= C.NORM_CAP}
    if "e" in caps:
        assert max(r["ew"][n] for n in pick) < C.EW_CAP, {n: r["ew"][n] for n in pick if r["ew"][n] >= C.EW_CAP}
    if "h" in caps and r["hidden_err"] is not None:
        assert r["hidden_err"] < C.HIDDEN_CAP, r["hidden_err"]
    exempt = EXEMPT.get((C.entry_id(e), mode), ())
    bad = {n: (r["e_dev"][n], r["p"].e_ref[n]) for n in pick if n not in exempt and r["e_dev"][n] > C.K * max(r["p"].e_ref[n], C.E_FLOOR)}
    assert not bad, f"{C.entry_id(e)} {mode}: e_dev > {C.K} * max(e_ref, {C.E_FLOOR}) for (e_dev, e_ref) {bad}"


def run_entry(dev, e, mode, only=None):
    r = measure(dev, e)
    assert_bounds(e, mode, r, only=only)
    return r


def test_exemptions_stay_within_their_limits():
    assert len(EXEMPT) <= 2 and all(mode != "f32" and mode in GEMM_MODES for _id, mode in EXEMPT)
    assert all(i in C.ENTRY_IDS for i, _m in EXEMPT)


@pytest.mark.parametrize("e", C.ENTRIES, ids=C.ENTRY_IDS)
def test_training_step_under_trained_statistics_equals_oracle(dev, e, gemm_mode):
    """(All three arithmetics.)  Caps, yardstick, three bit-identical steps, and the workspace tail behind the library's own
    layout untouched."""
    r = run_entry(dev, e, gemm_mode)
    first = {n: t.clone() for n, t in r["out"]["grads"].items()}
    keep = {k: r["out"][k].clone() for k in ("loss", "emb", "hidden") if r["out"].get(k) is not None}
    for _ in range(2):
        again = r["step"]()
        assert all(torch.equal(again[k], keep[k]) for k in keep), [k for k in keep if not torch.equal(again[k], keep[k])]
        assert all(torch.equal(again["grads"][n], first[n]) for n in first), [n for n in first if not torch.equal(again["grads"][n], first[n])]
    assert r["tail_intact"](), "the step wrote behind the workspace size the library reports"


# ------------------------------------------------------------------------------------------------ the fused GELU derivative
_FUSE_ENTRY = "gelusat_l1-enc-T40"
_FUSE_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import torch
import _training_stress_cases as C
import test_gpu_training_stress as S
from rag4dyg_amd import ops
e = C.ENTRIES[C.ENTRY_IDS.index(sys.argv[2])]
for mode in ("f16x2", "bf16x3", "f32"):
    ops.set_gemm_mode(mode)
    S.run_entry(torch.device("cuda:0"), e, mode, only=("mlp.c_fc.",))
print("FUSE_GELU_OK", os.environ["R4D_TRAIN_FUSE_GELU"])
"""


def test_c_fc_gradients_with_and_without_the_fused_gelu_derivative(dev, tmp_path):
    """One-layer model, saturated pre-activations (max |x| >= 10, a sixth of them in the 1 - tanh^2 cancellation region): the
    ``mlp.c_fc`` weight / bias gradients meet the bounds with the GELU derivative fused into the data-gradient GEMM's epilogue
    (``EPI_GELU_GRAD``, the default) and, in a fresh process (the variable is read once), with the two element-wise launches."""
    from rag4dyg_amd import ops
    assert os.environ.get("R4D_TRAIN_FUSE_GELU", "1") == "1", "this process must run the default (fused) epilogue"
    e = C.ENTRIES[C.ENTRY_IDS.index(_FUSE_ENTRY)]
    was = ops.gemm_mode()
    try:
        for mode in GEMM_MODES:
            ops.set_gemm_mode(mode)
            run_entry(dev, e, mode, only=("mlp.c_fc.",))
    finally:
        ops.set_gemm_mode(was)
    script = tmp_path / "fuse_worker.py"
    script.write_text(_FUSE_WORKER)
    pr = subprocess.run([sys.executable, str(script), REPO, _FUSE_ENTRY], env=dict(os.environ, R4D_TRAIN_FUSE_GELU="0"),
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(pr.stdout[-3000:])
    assert pr.returncode == 0 and "FUSE_GELU_OK 0" in pr.stdout, pr.stdout[-3000:]


def test_gelu_backward_kernel_through_saturation(dev):
    """``r4d_gelu_new_bwd_f32`` on pre-activations covering [-30, 30] densely plus exact 0, +-4, +-8, +-10.5, +-12."""
    from rag4dyg_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(17)
    special = torch.tensor([0.0, 4.0, -4.0, 8.0, -8.0, 10.5, -10.5, 12.0, -12.0, 30.0, -30.0])
    pre = torch.cat([torch.linspace(-30.0, 30.0, 60001), special, torch.randn(4000, generator=g) * 6.0]).float()
    dy = torch.randn(pre.numel(), generator=g)
    dy[60001:60001 + special.numel()] = 1.0
    pr = pre.double().requires_grad_(True)
    u = 0.7978845608028654 * (pr + 0.044715 * pr ** 3)
    (0.5 * pr * (1.0 + torch.tanh(u))).backward(dy.double())
    P, DY = pre.to(dev), dy.to(dev)
    dx = torch.full_like(P, float("nan"))
    _lib.check(lib.r4d_gelu_new_bwd_f32(P.data_ptr(), DY.data_ptr(), P.numel(), dx.data_ptr(), _stream()), "gelu_bwd")
    got = dx.cpu().numpy()
    assert np.isfinite(got).all()
    assert elementwise_err(got, pr.grad.numpy(), rtol=1e-4, atol=1e-5) < 1
    sat = np.abs(pre.numpy()) >= 12.0                                             # saturated: derivative 1 or 0 to 1e-5
    assert np.abs(got[sat] - np.where(pre.numpy()[sat] > 0, dy.numpy()[sat], 0.0)).max() < 1e-5 * np.abs(dy.numpy()).max()


# ------------------------------------------------------------------------------------------------ causal softmax backward
@pytest.mark.parametrize("scale", [1.0, 8.0, 40.0])
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 127, 128, 129, 640, 1000, 1023, 1024])
def test_causal_softmax_backward_edges(dev, T, scale):
    """``r4d_causal_softmax_bwd_f32`` at the lengths around its 64-column register tiles and 128-column leading dimension, up
    to the 16 x 64 limit, on flat and on peaked rows (logit spread ``scale`` after the division: row maximum near 1, most P
    below 1e-20 or exactly 0 at 40), with the dP buffer holding NaN right of the diagonal and in the pad columns -- the memory
    the kernel's comment calls unwritten.  Element-wise against float64 autograd, exact zeros there, no NaN, same bits again."""
    from rag4dyg_amd import _lib
    lib = _lib.load()
    nbh, ld, sd = 1 + T % 6, (T + 127) // 128 * 128, 8.0
    g = torch.Generator().manual_seed(1000 * T + int(scale))
    logits = (torch.randn(nbh, T, T, generator=g) * (scale * sd)).double().requires_grad_(True)
    mask = torch.tril(torch.ones(T, T, dtype=torch.bool))
    probs = torch.softmax(torch.where(mask, logits / sd, torch.tensor(-1e4, dtype=torch.float64)), dim=-1)
    dP = torch.randn(nbh, T, T, generator=g)
    probs.backward(dP.double())
    Pd = torch.zeros(nbh, T, ld)
    Pd[:, :, :T] = torch.where(mask, probs.detach().float(), torch.zeros(()))
    dPd = torch.full((nbh, T, ld), float("nan"))
    dPd[:, :, :T] = torch.where(mask, dP, torch.full((), float("nan")))
    Pd = Pd.to(dev)
    runs = []
    for _ in range(2):
        buf = dPd.to(dev)
        _lib.check(lib.r4d_causal_softmax_bwd_f32(Pd.data_ptr(), buf.data_ptr(), nbh, T, ld, sd, _stream()), "softmax_bwd")
        runs.append(buf.cpu())
    got = runs[0]
    assert not torch.isnan(got).any(), "NaN from the unwritten part of dP reached the output"
    assert torch.equal(runs[0], runs[1])
    full_mask = torch.zeros(T, ld, dtype=torch.bool)
    full_mask[:, :T] = mask
    assert float(got[:, ~full_mask].abs().max()) == 0.0                          # right of the diagonal and the pad: exact zeros
    want = torch.where(mask, logits.grad, torch.zeros((), dtype=torch.float64))
    if T == 1:                                                                   # a one-key softmax has no gradient
        assert float(got.abs().max()) < 1e-6
        return
    assert float(want.abs().max()) > 0
    assert elementwise_err(got[:, :, :T].numpy(), want.numpy()) < 1


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def _ln_reference(x, w, b, dy, dtype, reverse):
    xs, dys = (x.flip(0), dy.flip(0)) if reverse else (x, dy)
    xr, wr, br = (t.detach().clone().to(dtype).requires_grad_(True) for t in (xs, w, b))
    torch.nn.functional.layer_norm(xr, (x.shape[1],), wr, br, 1e-5).backward(dys.to(dtype))
    dx = xr.grad.flip(0) if reverse else xr.grad
    return dx.double().numpy(), wr.grad.double().numpy(), br.grad.double().numpy()


@pytest.mark.parametrize("rows,d", [(37, 256), (5003, 512), (3000, 768), (260, 1024)])
def test_layernorm_backward_on_offset_rows_with_outlier_gains(dev, rows, d):
    """``r4d_layernorm_bwd_f32`` on rows whose mean is 5-50 x their spread (the variance is a small difference of large numbers),
    three gains at 8 x and a 20 x outlier column in dy: dx element-wise against float64, dw / db under the yardstick bound with
    ``torch.nn.functional.layer_norm`` autograd in float32 (1 and 16 threads, rows in both orders) as the reference."""
    from rag4dyg_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(rows + d)
    mean = 1.0 + 9.0 * torch.rand(rows, 1, generator=g)
    mean[0] = 5.0
    x = torch.randn(rows, d, generator=g) * 0.2 + mean
    w = torch.randn(d, generator=g) * 0.1 + 1.0
    w[[d // 40, d // 3, (7 * d) // 9]] *= 8.0
    b = torch.randn(d, generator=g) * 0.1
    dy = torch.randn(rows, d, generator=g)
    dy[:, d // 5] *= 20.0
    dx64, dw64, db64 = _ln_reference(x, w, b, dy, torch.float64, False)
    was = torch.get_num_threads()
    e_w, e_b = 0.0, 0.0
    try:
        for threads, rev in C.ORDERS:
            torch.set_num_threads(threads)
            _dx, dw32, db32 = _ln_reference(x, w, b, dy, torch.float32, rev)
            e_w, e_b = max(e_w, rel_err(dw32, dw64)), max(e_b, rel_err(db32, db64))
    finally:
        torch.set_num_threads(was)
    X, W, DY = x.to(dev), w.to(dev), dy.to(dev)
    dx, dw, db = torch.empty_like(X), torch.empty(d, device=dev), torch.empty(d, device=dev)
    ws = torch.empty(lib.r4d_layernorm_bwd_workspace_bytes(rows, d), dtype=torch.uint8, device=dev)
    _lib.check(lib.r4d_layernorm_bwd_f32(X.data_ptr(), W.data_ptr(), DY.data_ptr(), None, rows, d, 1e-5, dx.data_ptr(), dw.data_ptr(),
                                         db.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "ln_bwd")
    d_w, d_b = rel_err(dw.cpu().numpy(), dw64), rel_err(db.cpu().numpy(), db64)
    ew = elementwise_err(dx.cpu().numpy(), dx64)
    print(f"[stress] layernorm_bwd {rows}x{d}: dx element-wise {ew:.3f}; dw {d_w:.2e} (ref {e_w:.2e}), db {d_b:.2e} (ref {e_b:.2e})")
    assert ew < 1
    assert d_w <= C.K * max(e_w, C.E_FLOOR) and d_b <= C.K * max(e_b, C.E_FLOOR), (d_w, e_w, d_b, e_b)


# ------------------------------------------------------------------------------------------------ beyond the fp16 range
def test_training_step_beyond_the_fp16_range_is_right_or_loud(dev, gemm_mode):
    """One ``c_fc`` column scaled until its GELU output exceeds 2^18 in the float64 oracle (csrc/gemm_h2.hip: the f16x2 A operand's
    hi term overflows there).  Under bf16x3 and f32 the step meets the bounds; under f16x2 it meets them OR is loud -- an
    ``R4DError``, a non-finite loss or a non-finite gradient -- never finite and wrong (inference has this guarantee in
    test_range_guard_f16x2_never_hands_out_nan_rankings)."""
    from rag4dyg_amd import _lib
    e = C.f16_range_entry()
    assert C.f16_range_weights()[2] > C.F16_RANGE_LIMIT
    try:
        r = measure(dev, e)
    except _lib.R4DError as err:
        assert gemm_mode == "f16x2", err
        print(f"[stress] f16 range | {gemm_mode} | loud: {err}")
        return
    if gemm_mode == "f16x2" and not r["finite"]:
        print(f"[stress] f16 range | {gemm_mode} | loud: non-finite loss or gradient (loss {r['loss_dev']})")
        return
    assert_bounds(e, gemm_mode, r)
