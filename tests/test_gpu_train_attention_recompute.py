"""GPU tests of the recompute mode of the training attention (``r4d_set_train_attention(1)``, csrc/train.hip): no kept
probabilities, P formed again in the backward by the forward's two launches, two fused row kernels (csrc/train_ops.hip) in
place of the element-wise passes.  Every GEMM reads the bits it reads in stored mode, so the acceptance test is EQUALITY OF
BITS with stored mode -- of each kernel against the composition of the existing entries, and of the retriever, LM and RAG
steps -- plus one independent anchor against float64 autograd."""
import math

import numpy as np
import pytest
import torch

import _train_modes
from conftest import rel_err

pytestmark = pytest.mark.gpu

SEED, STEP = 0x1234_5678_9ABC_DEF0, 2 ** 33 + 17
KERNEL_TS = [1, 5, 33, 64, 65, 127, 128, 129, 300, 1024]
NBH = 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_stored_mode_afterwards = _train_modes.switches_restored(force_stored=("attention",))


def _tpad128(T):
    return (T + 127) // 128 * 128


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _probabilities(dev, T, seed):
    """P [NBH, T, ld]: a causal softmax (zero right of the diagonal and in the padding), and a dP with NaN wherever no kernel
    may read it (right of the diagonal)."""
    ld = _tpad128(T)
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(NBH, T, T, generator=g) * 2
    mask = torch.tril(torch.ones(T, T, dtype=torch.bool))
    P = torch.zeros(NBH, T, ld)
    P[:, :, :T] = torch.softmax(logits.masked_fill(~mask, float("-inf")), dim=-1)
    dP = torch.full((NBH, T, ld), float("nan"))
    dP[:, :, :T] = torch.randn(NBH, T, T, generator=g).masked_fill(~mask, float("nan"))
    return P.to(dev), dP.to(dev), ld


def _transposed(x, T, ld):
    out = torch.zeros(NBH, T, ld, dtype=torch.float32, device=x.device)
    out[:, :, :T] = x[:, :, :T].transpose(1, 2)
    return out


def _drop_args(p, T):
    return (p, SEED, STEP, 9, 4 * (1000 + T)) if p > 0 else (0.0, 0, 0, 0, 0)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("T", KERNEL_TS)
def test_fused_softmax_backward_kernel_has_the_bits_of_the_three_launches(dev, T, p):
    """Kernel (a) against r4d_dropout_f32 in place on dP, r4d_causal_softmax_bwd_f32, then a transpose: dS over all ld columns
    and dS^T over all ld columns of its T rows, both buffers NaN before the launch."""
    from rag4dyg_amd import _lib
    lib = _lib.load()
    P, dP, ld = _probabilities(dev, T, seed=T)
    n = NBH * T * ld
    scale_div = float(math.sqrt(32.0))
    p_, seed, step, site, base = _drop_args(p, T)
    ref = dP.clone()
    if p > 0:
        _lib.check(lib.r4d_dropout_f32(ref.data_ptr(), None, n, ref.data_ptr(), p_, seed, step, site, base, _stream()), "dropout")
    _lib.check(lib.r4d_causal_softmax_bwd_f32(P.data_ptr(), ref.data_ptr(), NBH, T, ld, scale_div, _stream()), "softmax_bwd")
    ref_t = _transposed(ref, T, ld)
    got = dP.clone()
    got_t = torch.full((NBH, T, ld), float("nan"), device=dev)
    _lib.check(lib.r4d_softmax_dropout_bwd_transpose_f32(P.data_ptr(), got.data_ptr(), got_t.data_ptr(), NBH, T, ld, scale_div, p_, seed,
                                                         step, site, base, _stream()), "softmax_dropout_bwd_transpose")
    assert not torch.isnan(ref).any() and not torch.isnan(got).any() and not torch.isnan(got_t).any()
    assert _bits_equal(got, ref), f"dS differs in {(got != ref).sum().item()} elements"
    assert _bits_equal(got_t, ref_t), f"dS^T differs in {(got_t != ref_t).sum().item()} elements"
    assert T == 1 or ref[:, :, :T].abs().max() > 0                                # (a one-element softmax has a zero gradient)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("T", KERNEL_TS)
def test_fused_dropout_transpose_kernel_has_the_bits_of_the_two_launches(dev, T, p):
    """Kernel (b) against r4d_dropout_f32 followed by a transpose; at one shape the kept set against the oracle's generator."""
    from rag4dyg_amd import _lib
    lib = _lib.load()
    P, _dP, ld = _probabilities(dev, T, seed=T + 7)
    n = NBH * T * ld
    p_, seed, step, site, base = _drop_args(p, T)
    ref = torch.empty_like(P)
    _lib.check(lib.r4d_dropout_f32(P.data_ptr(), None, n, ref.data_ptr(), p_, seed, step, site, base, _stream()), "dropout")
    ref_t = _transposed(ref, T, ld)
    got_t = torch.full((NBH, T, ld), float("nan"), device=dev)
    _lib.check(lib.r4d_dropout_transpose_f32(P.data_ptr(), got_t.data_ptr(), NBH, T, ld, p_, seed, step, site, base, _stream()),
               "dropout_transpose")
    assert not torch.isnan(got_t).any()
    assert _bits_equal(got_t, ref_t), f"differs in {(got_t != ref_t).sum().item()} elements"
    if p > 0 and T == 33:
        from oracle import train_ref
        keep = train_ref.philox_keep(n, p, seed, step, site, base).reshape(NBH, T, ld)[:, :, :T]
        causal = np.tril(np.ones((T, T), dtype=bool))[None]
        kept = got_t[:, :, :T].transpose(1, 2).cpu().numpy() != 0                 # [bh, i, j]
        assert (P[:, :, :T].cpu().numpy()[np.broadcast_to(causal, kept.shape)] > 0).all()
        assert np.array_equal(kept, keep & causal)
        assert 0.8 < kept.sum() / (NBH * causal.sum()) < 0.97


# ------------------------------------------------------------------------------------------------ the retriever step
def _enc_model(dev, L, H, d, V=97, seed=3):
    from oracle import gpt2_ref
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModelRAG
    sd = gpt2_ref.make_state_dict(L, d, V, n_positions=1024, seed=seed, random_affine=True)
    m = GPT2LMHeadModelRAG(GPT2Config(vocab_size=V, n_positions=1024, n_ctx=1024, n_embd=d, n_layer=L, n_head=H))
    m.load_state_dict(sd, strict=False)
    return m.to(dev).eval(), sd


def _batches(V, shapes, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for B, T in shapes:
        ids = torch.randint(0, V - 2, (B, T), generator=g)
        for i in range(1, B):                                             # right-padded ragged rows, the first one full
            ids[i, int(torch.randint(max(1, T // 2), T + 1, (1,), generator=g)):] = V - 2
        out.append(ids)
    return out


def _enc_step(dev, m, batches, demb, attention, dropout, trainer=None):
    from rag4dyg_amd import training
    tr = trainer or training.EncoderTrainer(m, dropout=dropout, seed=77, attention=attention)
    emb = tr.forward([b.to(dev) for b in batches]).clone()
    grads = {n: g.clone() for n, g in tr.backward(demb).items()}
    return emb, grads, tr


def _assert_same_step(a, b):
    assert _bits_equal(a[0], b[0]), "mean-pool output differs"
    bad = [n for n in a[1] if not _bits_equal(a[1][n], b[1][n])]
    assert not bad, bad
    assert all(torch.isfinite(g).all() for g in a[1].values())
    assert sum(float(g.abs().sum()) for g in a[1].values()) > 0


FIVE = ((2, 7), (3, 33), (2, 129), (2, 130), (3, 64))
STEP_CASES = [("five batches, dropout off", 2, 2, 64, FIVE, (0.0, 0.0, 0.0)),
              ("five batches, dropout 0.1", 2, 2, 64, FIVE, (0.1, 0.1, 0.1)),
              ("head_dim 96, T 40 and 200", 1, 2, 192, ((2, 40), (2, 200)), (0.1, 0.1, 0.1)),
              ("T 1024", 1, 1, 64, ((1, 1024),), (0.1, 0.1, 0.1))]


def _demb(shapes, d, dev, seed=5):
    return torch.randn(sum(B for B, _ in shapes), d, generator=torch.Generator().manual_seed(seed)).to(dev)


@pytest.mark.parametrize("name,L,H,d,shapes,drop", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_retriever_step_has_the_bits_of_stored_mode(dev, name, L, H, d, shapes, drop):
    m, _sd = _enc_model(dev, L, H, d)
    batches = _batches(97, shapes, seed=len(shapes))
    demb = _demb(shapes, d, dev)
    stored = _enc_step(dev, m, batches, demb, "stored", drop)
    rec = _enc_step(dev, m, batches, demb, "recompute", drop)
    assert stored[2]._ws.numel() >= rec[2]._ws.numel()
    if L > 1 or len(shapes) > 1:
        assert stored[2]._ws.numel() > rec[2]._ws.numel()
    _assert_same_step(stored, rec)


def test_recompute_step_equals_float64_autograd(dev, monkeypatch):
    """The independent anchor: the five-batch step in recompute mode, dropout off, against float64 autograd of the oracle's
    grad-enabled forward (the one oracle.train_ref.training_step differentiates) under a loss linear in the mean-pooled
    embeddings.  tests/test_gpu_training.py states its stored-mode bound inline (max-norm 1e-4 on the embeddings, 1e-3 on every
    gradient, conftest.rel_err: test_training_gradients_other_shapes_equal_oracle) and exports no name for it, so the same two
    figures stand here -- and that test itself, imported, runs once more below with the mode switched to recompute."""
    from oracle import gpt2_ref
    from rag4dyg_amd import _lib, ops
    L, H, d = 2, 2, 64
    m, sd = _enc_model(dev, L, H, d)
    batches = _batches(97, FIVE, seed=len(FIVE))
    demb = _demb(FIVE, d, dev)
    emb, grads, _tr = _enc_step(dev, m, batches, demb, "recompute", (0.0, 0.0, 0.0))
    sdg = {k: v.clone().double().requires_grad_(True) for k, v in sd.items() if k != "lm_head.weight"}
    sdg["lm_head.weight"] = sdg["transformer.wte.weight"]
    pooled = torch.cat([gpt2_ref.gpt2_forward.__wrapped__(sdg, ids, H, want_logits=False)["hidden"].mean(dim=1) for ids in batches])
    (pooled * demb.cpu().double()).sum().backward()
    e_emb = rel_err(emb.cpu().numpy(), pooled.detach().numpy())
    errs = {n: rel_err(grads[n].cpu().numpy(), sdg[n].grad.numpy()) for n in grads}
    print(f"recompute vs float64 autograd: embeddings {e_emb:.2e} (bound 1e-4), worst gradient {max(errs.values()):.2e} (bound 1e-3)")
    assert e_emb < 1e-4
    assert max(errs.values()) < 1e-3, {n: e for n, e in errs.items() if e > 1e-3}
    import test_gpu_training as stored_tests
    monkeypatch.setenv("R4D_TRAIN_ATTENTION", "recompute")
    stored_tests.test_training_gradients_other_shapes_equal_oracle(dev, 2, 4, 64, 60, 2, (25, 30, 22), ops.gemm_mode())
    assert _lib.load().r4d_get_train_attention() == 1                      # its trainer did run in recompute mode


# ------------------------------------------------------------------------------------------------ the LM and the RAG step
@pytest.mark.parametrize("drop", [(0.0, 0.0, 0.0), (0.1, 0.1, 0.1)], ids=["dropout off", "dropout 0.1"])
@pytest.mark.parametrize("B,T", [(3, 20), (2, 160)])
def test_lm_step_has_the_bits_of_stored_mode(dev, B, T, drop):
    import test_gpu_lm_training as lm_tests
    from rag4dyg_amd.lm_training import LMTrainer
    m, _sd = lm_tests._model(dev, 2, 2, 64, 60, seed=11)
    ids = lm_tests._ids(60, B, T, seed=3, pad=59).to(dev)
    out = []
    for mode in ("stored", "recompute"):
        tr = LMTrainer(m, dropout=drop, seed=1234, attention=mode)
        loss = tr.step(ids).clone()
        out.append((loss.view(1), {n: g.clone() for n, g in tr.grads.items()}, tr))
    assert out[0][2]._ws.numel() > out[1][2]._ws.numel()
    assert math.isfinite(float(out[0][0]))
    _assert_same_step(out[0], out[1])


@pytest.mark.parametrize("drop", [(0.0, 0.0, 0.0), (0.1, 0.1, 0.1)], ids=["dropout off", "dropout 0.1"])
@pytest.mark.parametrize("freeze", [True, False], ids=["frozen", "unfrozen"])
def test_rag_step_has_the_bits_of_stored_mode(dev, freeze, drop):
    import test_gpu_generator_training as gen_tests
    from rag4dyg_amd.generator_training import GeneratorTrainer
    m, tok, idx, src = gen_tests._setup(dev, 2, 2, 64, 60, 3, 20, seed=11, freeze=freeze)
    bags = gen_tests._bags(idx, src, dev)
    out = []
    for mode in ("stored", "recompute"):
        tr = GeneratorTrainer(m, freeze=freeze, dropout=drop, seed=1234, attention=mode)
        loss = tr.step(tok.to(dev), bags).clone()
        out.append((loss.view(1), {n: g.clone() for n, g in tr.grads.items()}, tr))
    assert out[0][2]._ws.numel() > out[1][2]._ws.numel()
    assert math.isfinite(float(out[0][0]))
    _assert_same_step(out[0], out[1])


# ------------------------------------------------------------------------------------------------ the switch at run time
def test_backward_under_another_mode_than_its_forward_is_refused(dev):
    from rag4dyg_amd import _lib, training
    lib = _lib.load()
    m, _sd = _enc_model(dev, 2, 2, 64)
    shapes = FIVE[:3]
    batches = _batches(97, shapes, seed=9)
    demb = _demb(shapes, 64, dev)
    drop = (0.1, 0.1, 0.1)
    want = _enc_step(dev, m, batches, demb, "stored", drop)
    tr = training.EncoderTrainer(m, dropout=drop, seed=77, attention="recompute")
    tr._ws = torch.empty(want[2]._ws.numel(), dtype=torch.uint8, device=dev)      # large enough for either layout
    tr.forward([b.to(dev) for b in batches])
    tr.attention = "stored"                                                       # the trainer now selects mode 0 before the backward
    with pytest.raises(_lib.R4DError):
        tr.backward(demb)
    assert lib.r4d_get_train_attention() == 0
    _assert_same_step(want, _enc_step(dev, m, batches, demb, "stored", drop))     # and stored mode is what it was


def test_two_trainers_of_different_modes_alternate_in_one_process(dev):
    from rag4dyg_amd import training
    m, _sd = _enc_model(dev, 2, 2, 64)
    shapes = FIVE[:3]
    batches = _batches(97, shapes, seed=4)
    demb = _demb(shapes, 64, dev)
    drop = (0.1, 0.1, 0.1)
    ref = []                                                                      # steps 1..3 of one stored trainer: the reference bits
    tr = None
    for _ in range(3):
        emb, grads, tr = _enc_step(dev, m, batches, demb, "stored", drop, trainer=tr)
        ref.append((emb, grads))
    assert not _bits_equal(ref[0][0], ref[1][0])                                  # new masks every step
    a = training.EncoderTrainer(m, dropout=drop, seed=77, attention="stored")
    b = training.EncoderTrainer(m, dropout=drop, seed=77, attention="recompute")
    for k in range(3):
        ea = a.forward([x.to(dev) for x in batches]).clone()                      # interleaved: a's forward, b's whole step, a's backward
        got_b = _enc_step(dev, m, batches, demb, None, None, trainer=b)
        ga = {n: g.clone() for n, g in a.backward(demb).items()}
        _assert_same_step(ref[k], (ea, ga))
        _assert_same_step(ref[k], got_b)
