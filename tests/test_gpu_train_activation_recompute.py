"""GPU tests of the recompute mode of the training activations (``r4d_set_train_activations(1)``, csrc/train.hip): the forward
keeps each layer's input, the backward forms one layer's ln1 .. f (and P) at a time again in ONE shared set by the forward's own
launches.  The same launches on the same bits, so the acceptance test is EQUALITY OF BITS with stored-activations mode in the
same process and the same GEMM arithmetic -- of the retriever, LM and RAG steps, under both attention modes, with every dropout
site on and off -- plus one independent anchor against float64 autograd.

Shapes: L = 3 (a first, a middle and a last layer), H2 d64, ragged right-padded batches (2,7), (3,33), (2,129) (T crosses the
128-position tile), and one d = 256 L2 H2 (2,40) case for the pre-split GEMM path."""
import ctypes
import math

import pytest
import torch

import _train_modes
from conftest import elementwise_err, rel_err
from test_gpu_train_attention_recompute import _assert_same_step, _batches, _bits_equal, _demb, _enc_model

pytestmark = pytest.mark.gpu

TINY = ("L3 H2 d64", 3, 2, 64, ((2, 7), (3, 33), (2, 129)))
WIDE = ("L2 H2 d256", 2, 2, 256, ((2, 40),))
DROPS = [(0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (0.1, 0.0, 0.0), (0.0, 0.0, 0.1)]       # (embd, attn, resid)
DROP_IDS = ["dropout off", "dropout 0.1", "embd dropout", "resid dropout"]
ATTENTION = ["stored", "recompute"]
ATT_IDS = ["P stored", "P recompute"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_both_switches_stored_afterwards = _train_modes.switches_restored(force_stored=("attention", "activations"))


def _enc_trainer(m, drop, attention, activations):
    from rag4dyg_amd import training
    return training.EncoderTrainer(m, dropout=drop, seed=77, attention=attention, activations=activations)


def _step(dev, tr, batches, demb):
    emb = tr.forward([b.to(dev) for b in batches]).clone()
    return emb, {n: g.clone() for n, g in tr.backward(demb).items()}


# ------------------------------------------------------------------------------------------------ the retriever step
@pytest.mark.parametrize("attention", ATTENTION, ids=ATT_IDS)
@pytest.mark.parametrize("drop", DROPS, ids=DROP_IDS)
@pytest.mark.parametrize("name,L,H,d,shapes", [TINY, WIDE], ids=[TINY[0], WIDE[0]])
def test_retriever_step_has_the_bits_of_stored_activations(dev, name, L, H, d, shapes, drop, attention, gemm_mode):
    """Mean-pool output and every gradient of three consecutive steps (new masks each step) equal stored-activations mode; the
    workspace is smaller; without dropout the three steps are identical."""
    from rag4dyg_amd import _lib
    m, _sd = _enc_model(dev, L, H, d)
    batches = _batches(97, shapes, seed=len(shapes))
    demb = _demb(shapes, d, dev)
    stored, rec = _enc_trainer(m, drop, attention, "stored"), _enc_trainer(m, drop, attention, "recompute")
    steps = []
    for _ in range(3):
        a = _step(dev, stored, batches, demb)
        b = _step(dev, rec, batches, demb)
        assert _lib.load().r4d_get_train_activations() == 1                   # the second trainer did select recompute mode
        _assert_same_step(a, b)
        steps.append(b)
    M = sum(B * T for B, T in shapes)
    assert stored._ws.numel() - rec._ws.numel() >= 4 * (15 * (L - 1) - 1) * M * d - 256 * (9 * L + 12)
    if not any(drop):
        _assert_same_step(steps[0], steps[1])
        _assert_same_step(steps[0], steps[2])
    else:
        assert not _bits_equal(steps[0][0], steps[1][0])                       # new masks every step


@pytest.mark.parametrize("drop", [DROPS[0], DROPS[1]], ids=DROP_IDS[:2])
def test_smaller_shape_after_a_larger_one_equals_a_fresh_trainer(dev, drop):
    """No stale reads from the shared set: the offsets of every block move with the shape."""
    name, L, H, d, shapes = TINY
    m, _sd = _enc_model(dev, L, H, d)
    big = _batches(97, ((3, 140), (4, 65), (2, 129)), seed=8)
    small = _batches(97, shapes, seed=3)
    used = _enc_trainer(m, drop, "stored", "recompute")
    _step(dev, used, big, _demb(((3, 140), (4, 65), (2, 129)), d, dev))
    ws_before = used._ws.data_ptr()
    got = _step(dev, used, small, _demb(shapes, d, dev))
    assert used._ws.data_ptr() == ws_before                                    # the larger step's buffer, reused
    for activations in ("recompute", "stored"):
        fresh = _enc_trainer(m, drop, "stored", activations)
        fresh.step = used.step - 1                                             # the same dropout counter as the used trainer's step
        _assert_same_step(_step(dev, fresh, small, _demb(shapes, d, dev)), got)


def test_recompute_step_equals_float64_autograd(dev):
    """The independent anchor: one L3 retriever step in recompute mode (both switches), dropout off, under the loss
    0.5 * sum(pooled ** 2), against float64 autograd of the oracle's grad-enabled forward.  Bounds of the generator-training
    tests: loss within 1e-5 relative, every gradient rel_err < 1e-3 and element-wise rtol 1e-3 / atol 1e-4."""
    from oracle import gpt2_ref
    name, L, H, d, shapes = TINY
    m, sd = _enc_model(dev, L, H, d)
    batches = _batches(97, shapes, seed=len(shapes))
    tr = _enc_trainer(m, (0.0, 0.0, 0.0), "recompute", "recompute")
    emb = tr.forward([b.to(dev) for b in batches]).clone()
    grads = {n: g.clone() for n, g in tr.backward(emb).items()}               # dLoss/d(pooled) = pooled
    loss = 0.5 * float((emb.double() ** 2).sum())
    sdg = {k: v.clone().double().requires_grad_(True) for k, v in sd.items() if k != "lm_head.weight"}
    sdg["lm_head.weight"] = sdg["transformer.wte.weight"]
    pooled = torch.cat([gpt2_ref.gpt2_forward.__wrapped__(sdg, ids, H, want_logits=False)["hidden"].mean(dim=1) for ids in batches])
    want = 0.5 * (pooled ** 2).sum()
    want.backward()
    errs = {n: rel_err(grads[n].cpu().numpy(), sdg[n].grad.numpy()) for n in grads}
    ew = {n: elementwise_err(grads[n].cpu().numpy(), sdg[n].grad.numpy(), rtol=1e-3, atol=1e-4) for n in grads}
    print(f"recompute vs float64 autograd: loss {abs(loss / float(want.detach()) - 1):.2e} (bound 1e-5), worst gradient "
          f"{max(errs.values()):.2e} (bound 1e-3), element-wise {max(ew.values()):.2e} (bound 1)")
    assert abs(loss / float(want.detach()) - 1) < 1e-5, (loss, float(want.detach()))
    assert max(errs.values()) < 1e-3, {n: e for n, e in errs.items() if e > 1e-3}
    assert max(ew.values()) < 1, {n: e for n, e in ew.items() if e >= 1}


# ------------------------------------------------------------------------------------------------ the LM step
def _lm_forward_only(dev, tr, ids):
    """ln_f rows of the library's forward-only entry on the trainer's weights, and the shifted cross entropy of their logits."""
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    c, w, _g, keep = tr.enc._structs()
    B, T = ids.shape
    Bs, Ts = (ctypes.c_int32 * 1)(B), (ctypes.c_int32 * 1)(T)
    ptrs = (ctypes.c_void_p * 1)(ids.data_ptr())
    tr.enc.select_modes()
    ws = torch.empty(int(lib.r4d_gpt2_train_workspace_bytes(ctypes.byref(c), 1, Bs, Ts)), dtype=torch.uint8, device=dev)
    h = torch.empty(B, T, tr.d, device=dev)
    _lib.check(lib.r4d_gpt2_train_forward_hidden_f32(ctypes.byref(c), ctypes.byref(w), 1, ptrs, Bs, Ts, h.data_ptr(), None, ws.data_ptr(),
                                                     ws.numel(), torch.cuda.current_stream().cuda_stream), "gpt2_train_forward_hidden")
    logits = ops.lm_logits(h, tr.enc.params["transformer.wte.weight"])
    loss = torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]).double(), ids[:, 1:].reshape(-1))
    return h, loss


@pytest.mark.parametrize("attention", ATTENTION, ids=ATT_IDS)
@pytest.mark.parametrize("drop", DROPS[:2], ids=DROP_IDS[:2])
def test_lm_step_has_the_bits_of_stored_activations(dev, drop, attention, gemm_mode):
    import test_gpu_lm_training as lm_tests
    from rag4dyg_amd.lm_training import LMTrainer
    m, _sd = lm_tests._model(dev, 3, 2, 64, 60, seed=11)
    ids = lm_tests._ids(60, 3, 130, seed=3, pad=59).to(dev)
    out, fwd = [], []
    for mode in ("stored", "recompute"):
        tr = LMTrainer(m, dropout=drop, seed=1234, attention=attention, activations=mode)
        for _ in range(2):                                                     # the second step of each trainer is compared
            loss = tr.step(ids).clone()
        out.append((loss.view(1), {n: g.clone() for n, g in tr.grads.items()}, tr))
        fwd.append(_lm_forward_only(dev, tr, ids))
    assert out[0][2]._ws.numel() > out[1][2]._ws.numel()
    assert math.isfinite(float(out[0][0]))
    _assert_same_step(out[0], out[1])
    assert _bits_equal(fwd[0][0], fwd[1][0]) and torch.equal(fwd[0][1], fwd[1][1])      # forward only: rows and loss
    if not any(drop):
        assert abs(float(fwd[1][1]) / float(out[1][0]) - 1) < 1e-5             # and it is the step's loss


# ------------------------------------------------------------------------------------------------ the RAG step
@pytest.mark.parametrize("attention", ATTENTION, ids=ATT_IDS)
@pytest.mark.parametrize("drop", DROPS[:2], ids=DROP_IDS[:2])
@pytest.mark.parametrize("freeze", [True, False], ids=["frozen", "unfrozen"])
def test_rag_step_has_the_bits_of_stored_activations(dev, freeze, drop, attention, gemm_mode):
    """Layer 0 runs through the splice kernel here.  Loss, hidden rows, every gradient, d_fused; backward=False writes no
    gradient and gives the same loss in both modes."""
    import test_gpu_generator_training as gen_tests
    from rag4dyg_amd.generator_training import GeneratorTrainer
    L, d, B, T = 3, 64, 3, 130
    m, tok, idx, src = gen_tests._setup(dev, L, 2, d, 60, B, T, seed=11, freeze=freeze)
    bags = gen_tests._bags(idx, src, dev)
    out = []
    for mode in ("stored", "recompute"):
        tr = GeneratorTrainer(m, freeze=freeze, dropout=drop, seed=1234, attention=attention, activations=mode)
        h = torch.empty(B, T + 1, d, device=dev)
        loss = tr.step(tok.to(dev), bags, hidden_out=h).clone()
        grads = {n: g.clone() for n, g in tr.grads.items()}
        grads["d_fused"] = tr._scratch["d_fused"].clone()
        grads["hidden_out"] = h
        tr.flat_grads.fill_(7.0)
        h0 = torch.empty_like(h)
        loss0 = tr.step(tok.to(dev), bags, backward=False, hidden_out=h0).clone()
        assert torch.all(tr.flat_grads == 7.0)                                 # forward only: the gradients are untouched
        out.append((loss.view(1), grads, tr, loss0, h0))
    assert out[0][2]._ws.numel() > out[1][2]._ws.numel()
    assert math.isfinite(float(out[0][0])) and float(out[0][1]["d_fused"].abs().sum()) > 0
    _assert_same_step(out[0], out[1])
    assert torch.equal(out[0][3], out[1][3]) and _bits_equal(out[0][4], out[1][4])


# ------------------------------------------------------------------------------------------------ the switch at run time
@pytest.mark.parametrize("fwd_mode,bwd_mode", [("recompute", "stored"), ("stored", "recompute")])
def test_backward_under_another_activations_mode_than_its_forward_is_refused(dev, fwd_mode, bwd_mode):
    from rag4dyg_amd import _lib
    lib = _lib.load()
    name, L, H, d, shapes = TINY
    m, _sd = _enc_model(dev, L, H, d)
    batches = _batches(97, shapes, seed=9)
    demb = _demb(shapes, d, dev)
    drop = (0.1, 0.1, 0.1)
    ref = _enc_trainer(m, drop, "stored", "stored")
    want = _step(dev, ref, batches, demb)
    tr = _enc_trainer(m, drop, "stored", fwd_mode)
    tr._ws = torch.empty(ref._ws.numel(), dtype=torch.uint8, device=dev)       # large enough for either layout
    tr.forward([b.to(dev) for b in batches])
    tr.activations = bwd_mode                                                  # the trainer now selects the other mode before the backward
    with pytest.raises(_lib.R4DError):
        tr.backward(demb)
    assert lib.r4d_get_train_activations() == {"stored": 0, "recompute": 1}[bwd_mode]
    tr.activations = fwd_mode                                                  # under its own mode the same backward goes through
    got = {n: g.clone() for n, g in tr.backward(demb).items()}
    assert all(_bits_equal(got[n], want[1][n]) for n in got)
    _assert_same_step(want, _step(dev, _enc_trainer(m, drop, "stored", "stored"), batches, demb))


def test_trainers_of_different_activation_modes_alternate_in_one_process(dev):
    """a's forward, b's whole step, a's backward: a's backward then runs on a workspace that is not the latest forward's."""
    name, L, H, d, shapes = TINY
    m, _sd = _enc_model(dev, L, H, d)
    batches = _batches(97, shapes, seed=4)
    demb = _demb(shapes, d, dev)
    drop = (0.1, 0.1, 0.1)
    ref_tr = _enc_trainer(m, drop, "stored", "stored")
    ref = [_step(dev, ref_tr, batches, demb) for _ in range(2)]
    a, b = _enc_trainer(m, drop, "recompute", "recompute"), _enc_trainer(m, drop, "stored", "stored")
    c = _enc_trainer(m, drop, "stored", "recompute")
    for k in range(2):
        ea = a.forward([x.to(dev) for x in batches]).clone()
        got_b = _step(dev, b, batches, demb)
        got_c = _step(dev, c, batches, demb)
        ga = {n: g.clone() for n, g in a.backward(demb).items()}
        _assert_same_step(ref[k], (ea, ga))
        _assert_same_step(ref[k], got_b)
        _assert_same_step(ref[k], got_c)
