"""GPU tests of the vocabulary-chunked LM head (``csrc/lm_head.hip``, ldV > 15,872 -- every call here was refused before it
existed): ``r4d_lm_ce_f32`` at the smallest such size and at three chunks against float64 torch, the SimpleDyG step
(``LMTrainer``, all three arithmetics, the recompute modes) and the RAG step (``GeneratorTrainer``, frozen / unfrozen, the
forward-only loss) against the oracles of the small-vocabulary tests, the buffer contract on poisoned memory and ``main_SimpleDyG.py`` end to end on a 15,900-node toy graph.  (The workspace query is host arithmetic:
``tests/test_host_large_vocab_head.py``.)

Tolerances: those of ``tests/test_gpu_lm_training.py`` -- CE kernel: loss relative 1e-6, ``elementwise_err < 1``; step: loss 1e-5,
gradients ``rel_err < 1e-3`` and ``elementwise_err(rtol 1e-3, atol 1e-4) < 1`` against float64 autograd.  The shapes are tiny
(d = 64, L <= 2, B * T <= 32 rows); what is large is V alone.  This file is also the coverage of the chunked branch: the
dispatcher-branch table has no row for it."""
import io
import re
from contextlib import redirect_stdout

import pytest
import torch

import _train_modes
import test_gpu_generator_training as gen_tests
import test_gpu_lm_training as lm_tests
from _poison import PATTERNS, ZERO, poison, poisoned_allocations
from conftest import elementwise_err, rel_err

pytestmark = pytest.mark.gpu

SMALLEST = 15873                      # padded to 16,000 columns: the smallest vocabulary the one-row kernel cannot take


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_switches_restored = _train_modes.switches_restored(force_stored=("attention", "activations"))


def _chunk():
    from rag4dyg_amd import _lib
    C = int(_lib.load().r4d_lm_head_chunk_rows(1 << 20))
    assert C % 128 == 0 and 128 <= C <= 15872
    return C


def _vocab(which):
    return SMALLEST if which == "smallest" else 2 * _chunk() + 5       # three chunks, the last one: 5 classes + 123 pad columns


# ================================================================================================ 1. r4d_lm_ce_f32
def _ce_case(V, B, T, scale, with_labels):
    """Logits, the label array and the float64 reference.  Hand-placed labels (rows 0 .. 5 of the first sequence): column 0,
    C - 1, C, V - 1, a label in the FIRST chunk under a maximum in the LAST one (the running sum is rescaled after the label's
    chunk), and the reverse."""
    C = _chunk()
    g = torch.Generator().manual_seed(V + T)
    x = torch.randn(B * T, V, generator=g) * scale
    src = torch.randint(0, V, (B, T), generator=g)
    if with_labels:
        src[torch.rand(B, T, generator=g) < 0.3] = -100
    src[0, 1:7] = torch.tensor([0, C - 1, C, V - 1, 5, V - 3])
    x[4, V - 1] = 12.0 * scale                                        # (V - 1 lies in the last chunk whatever C is)
    x[5, 1] = 12.0 * scale
    return x, src


@pytest.mark.parametrize("B,T", [(2, 9), (3, 8)])
@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("which", ["smallest", "three chunks"])
def test_lm_ce_beyond_one_lds_row_equals_float64(dev, which, scale, B, T):
    """Loss (relative 1e-6), dlogits element-wise, exact zeros in the pad columns (garbage on entry) and in uncounted rows, a
    bit-identical relaunch.  (3, 8) runs with a label array holding 30 % -100 and grad_scale 0.5, (2, 9) with labels == ids."""
    from rag4dyg_amd.lm_training import padded_vocab
    V = _vocab(which)
    with_labels, gs = (T == 8), (0.5 if T == 8 else 1.0)
    ldV, N = padded_vocab(V), B * T
    assert ldV > 15872 and ldV > V
    x, src = _ce_case(V, B, T, scale, with_labels)
    ref = x.double().requires_grad_(True)
    want = torch.nn.functional.cross_entropy(ref.view(B, T, V)[:, :-1].reshape(-1, V), src[:, 1:].reshape(-1))
    (want * gs).backward()
    want = float(want.detach())
    logits = torch.empty(N, ldV, device=dev)
    logits[:, :V] = x.to(dev)
    logits[:, V:] = 7.0                                               # garbage in the pad: never read as a class
    logits[:, V + 1::2] = 3.0e38
    first = logits.clone()
    src_d = src.to(dev)
    ids_d, labels_d = (torch.zeros_like(src_d), src_d) if with_labels else (src_d, None)
    loss = lm_tests._ce(logits, ids_d, V, T, labels_d, gs)
    print(f"V={V} scale={scale} B={B} T={T}: loss rel err {abs(float(loss) / want - 1):.3e}")
    assert abs(float(loss) / want - 1) < 1e-6, (float(loss), want)
    got = logits.cpu()
    assert torch.all(got[:, V:] == 0)
    counted = torch.zeros(B, T, dtype=torch.bool)
    counted[:, :-1] = src[:, 1:] != -100
    assert counted.view(-1)[:6].all()
    assert torch.all(got[~counted.view(-1)] == 0)
    ew = elementwise_err(got[:, :V].numpy(), ref.grad.numpy())
    print(f"    dlogits element-wise {ew:.3e}")
    assert ew < 1
    again = first.clone()
    loss2 = lm_tests._ce(again, ids_d, V, T, labels_d, gs)
    assert torch.equal(again, logits) and torch.equal(loss2, loss)


def test_lm_ce_beyond_one_lds_row_flags_a_bad_label(dev):
    from rag4dyg_amd import ops
    from rag4dyg_amd.lm_training import padded_vocab
    V, B, T = SMALLEST, 2, 9
    ops.range_flag(dev)
    ops.take_range_flag()
    ids = torch.randint(0, V, (B, T)).to(dev)
    lm_tests._ce(torch.randn(B * T, padded_vocab(V), device=dev), ids, V, T)
    assert ops.take_range_flag() == 0
    lab = ids.clone()
    lab[1, 2] = V
    lm_tests._ce(torch.randn(B * T, padded_vocab(V), device=dev), ids, V, T, labels=lab)
    assert ops.take_range_flag() & ops.RANGE_BAD_LABEL


# ================================================================================================ 2. the SimpleDyG step
LM_SHAPES = {"smallest": (1, 2, 64, 2, 8), "three chunks": (2, 2, 64, 2, 12)}          # L, H, d, B, T
_LM_CACHE = {}


def _lm_ids(V, B, T):
    """Right-padded ids with tokens of EVERY chunk: the last one (V - 2 .. V - 5), V - 1 itself (the pad id), and the two rows on
    either side of the first chunk boundary."""
    C = _chunk()
    ids = lm_tests._ids(V, B, T, seed=V + T, pad=V - 1)
    ids[0, 1:7] = torch.tensor([V - 2, C, C - 1, V - 5, V - 1, 0])
    ids[1, 1:3] = torch.tensor([V - 3, min(C + 1, V - 1)])
    return ids


def _lm_case(dev, which):
    """Model, ids and the float64 oracle (computed once per shape; shared by the arithmetics and the poison test, never written)."""
    if which not in _LM_CACHE:
        L, H, d, B, T = LM_SHAPES[which]
        V = _vocab(which)
        m, sd = lm_tests._model(dev, L, H, d, V, seed=L * 100 + d)
        ids = _lm_ids(V, B, T)
        want, ref = lm_tests._oracle(sd, ids, H)
        _LM_CACHE[which] = (m, ids, H, want, ref)
    return _LM_CACHE[which]


@pytest.mark.parametrize("which", list(LM_SHAPES))
def test_lm_step_on_a_large_vocabulary_equals_oracle(dev, which, gemm_mode):
    """Loss and every gradient (wte = scatter + both sweeps' head part) against float64 autograd; three steps bit-identical; the
    two recompute modes give the stored modes' bits."""
    from rag4dyg_amd.lm_training import LMTrainer
    m, ids, _H, want, ref = _lm_case(dev, which)
    tr = LMTrainer(m)
    assert tr.ldV > 15872
    loss = tr.step(ids.to(dev))
    assert abs(float(loss) / want - 1) < 1e-5, (float(loss), want)
    worst = {n: rel_err(tr.grads[n].cpu().numpy(), ref[n].numpy()) for n in ref}
    assert max(worst.values()) < 1e-3, {n: e for n, e in worst.items() if e > 1e-3}
    ew = {n: elementwise_err(tr.grads[n].cpu().numpy(), ref[n].numpy(), rtol=1e-3, atol=1e-4) for n in ref}
    assert max(ew.values()) < 1, {n: e for n, e in ew.items() if e >= 1}
    first = {n: t.clone() for n, t in tr.grads.items()}
    for _ in range(2):
        assert torch.equal(tr.step(ids.to(dev)), loss)
        assert all(torch.equal(tr.grads[n], first[n]) for n in first)
    for kw in (dict(attention="recompute"), dict(activations="recompute")):
        other = LMTrainer(m, **kw)
        assert torch.equal(other.step(ids.to(dev)), loss), kw
        assert all(torch.equal(other.grads[n], first[n]) for n in first), kw


# ================================================================================================ 3. the RAG step
RAG = dict(L=1, H=2, d=64, V=SMALLEST, B=2, T=12)


def test_rag_step_on_a_large_vocabulary_equals_oracle(dev):
    """The frozen, untied configuration and the unfrozen, tied one against float64 autograd."""
    from rag4dyg_amd.generator_training import GeneratorTrainer
    c = RAG
    for freeze in (True, False):
        m, tok, idx, src = gen_tests._setup(dev, c["L"], c["H"], c["d"], c["V"], c["B"], c["T"], seed=23, freeze=freeze)
        tok[0, 1:5] = torch.tensor([c["V"] - 2, _chunk(), _chunk() - 1, c["V"] - 1])
        tr = GeneratorTrainer(m, freeze=freeze, dropout=(0.0, 0.0, 0.0))
        assert tr.ldV > 15872
        loss = tr.step(tok.to(dev), gen_tests._bags(idx, src, dev))
        want, ref, _h = gen_tests._oracle(m, tok, idx, src, c["H"], freeze=freeze)
        gen_tests._check(tr, ref, loss, want)


def test_rag_frozen_step_equals_unfrozen_step_and_the_forward_only_loss(dev):
    """Frozen loss, head gradient and fusion gradients equal the unfrozen (untied) step's bit for bit; ``backward=False`` -- the
    head stops after its first sweep -- returns the same loss bits and writes no gradient."""
    from rag4dyg_amd.generator_training import GeneratorTrainer
    c = RAG
    m, tok, idx, src = gen_tests._setup(dev, c["L"], c["H"], c["d"], c["V"], c["B"], c["T"], seed=31, freeze=True)
    bags = gen_tests._bags(idx, src, dev)
    frozen = GeneratorTrainer(m, freeze=True, dropout=(0.1, 0.1, 0.1), seed=5)
    loss_f = frozen.step(tok.to(dev), bags)
    g_f = {n: t.clone() for n, t in frozen.grads.items()}
    free = GeneratorTrainer(m, freeze=False, dropout=(0.1, 0.1, 0.1), seed=5)       # untied head, transformer trainable
    loss_u = free.step(tok.to(dev), bags)
    assert torch.equal(loss_f, loss_u)
    for n in g_f:
        assert torch.equal(g_f[n], free.grads[n]), n
    plain = GeneratorTrainer(m, freeze=True, dropout=(0.0, 0.0, 0.0))
    loss = plain.step(tok.to(dev), bags)
    plain.flat_grads.fill_(7.0)
    only = plain.step(tok.to(dev), bags, backward=False)
    assert torch.equal(only, loss) and torch.all(plain.flat_grads == 7.0)


# ================================================================================================ 4. the buffer contract
def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _assert_poison_is_invisible(run):
    """``run(pattern)`` -> {name: tensor}: under NaN bytes, 0x7F bytes and the word 1 the bits of the run on zeroed memory."""
    base = run(ZERO)
    assert all(torch.isfinite(v).all() for v in base.values()) and sum(float(v.double().abs().sum()) for v in base.values()) > 0
    for pattern in PATTERNS[1:]:
        got = run(pattern)
        bad = [n for n in base if not torch.equal(_bits(base[n]), _bits(got[n]))]
        assert set(got) == set(base) and not bad, (pattern, bad)


def test_large_vocabulary_lm_ce_does_not_read_unwritten_memory(dev):
    from rag4dyg_amd import _lib, ops
    from rag4dyg_amd.lm_training import padded_vocab
    lib = _lib.load()
    V, B, T = _vocab("three chunks"), 2, 9
    ldV, N = padded_vocab(V), B * T
    x, src = _ce_case(V, B, T, 1.0, False)
    x, src = x.to(dev), src.to(dev)

    def run(pattern):
        ops._WS.clear()
        with poisoned_allocations(pattern):
            logits = torch.empty(N, ldV, device=dev)                  # pad columns: the pattern
            logits[:, :V] = x
            ws = ops.workspace(lib.r4d_lm_ce_workspace_bytes(N), dev, "lm_ce_large_poison")
            loss = torch.empty((), dtype=torch.float32, device=dev)
        _lib.check(lib.r4d_lm_ce_f32(logits.data_ptr(), N, V, ldV, src.data_ptr(), None, T, 1.0, loss.data_ptr(), ws.data_ptr(),
                                     ws.numel(), torch.cuda.current_stream().cuda_stream), "lm_ce")
        assert torch.all(logits[:, V:] == 0)
        return dict(dlogits=logits, loss=loss.view(1))
    _assert_poison_is_invisible(run)


def test_large_vocabulary_lm_step_does_not_read_unwritten_memory(dev):
    """First allocation under poison, then the same step in the re-poisoned workspace: loss and every gradient."""
    from rag4dyg_amd.lm_training import LMTrainer
    m, ids, _H, _want, _ref = _lm_case(dev, "three chunks")

    def run(pattern):
        with poisoned_allocations(pattern):                           # the head planes too
            tr = LMTrainer(m)
            tr.step(ids.to(dev))
        poison(tr._ws, pattern)
        poison(tr.flat_grads, pattern)
        with poisoned_allocations(pattern):
            loss = tr.step(ids.to(dev)).clone()
        return dict({n: t.clone() for n, t in tr.grads.items()}, loss=loss.view(1))
    _assert_poison_is_invisible(run)


@pytest.mark.parametrize("freeze", [True, False], ids=["frozen", "unfrozen"])
def test_large_vocabulary_rag_step_does_not_read_unwritten_memory(dev, freeze):
    from rag4dyg_amd.generator_training import GeneratorTrainer
    c = RAG
    m, tok, idx, src = gen_tests._setup(dev, c["L"], c["H"], c["d"], c["V"], c["B"], c["T"], seed=11, freeze=freeze)
    bags = gen_tests._bags(idx, src, dev)

    def run(pattern):
        with poisoned_allocations(pattern):
            tr = GeneratorTrainer(m, freeze=freeze, dropout=(0.0, 0.0, 0.0))
            tr.step(tok.to(dev), bags)
        for b in [tr._ws, tr.flat_grads] + list(tr._scratch.values()):
            poison(b, pattern)
        with poisoned_allocations(pattern):
            loss = tr.step(tok.to(dev), bags).clone()
            only = tr.step(tok.to(dev), bags, backward=False).clone()
        return dict({n: t.clone() for n, t in tr.grads.items()}, loss=loss.view(1), loss_only=only.view(1),
                    d_fused=tr._scratch["d_fused"].clone())
    _assert_poison_is_invisible(run)


# ================================================================================================ 5. the CLI
def test_main_simpledyg_trains_and_evaluates_a_15900_node_graph(dev, tmp_path, monkeypatch):
    """``main_SimpleDyG.py --do_train --evaluate_during_training`` on a toy graph of 15,900 node tokens (+ the time and special
    tokens: ldV > 15,872): two epochs run, the loss falls, checkpoint-0 loads, and ``--do_eval`` over it prints finite metrics
    (the greedy evaluation works at this V as well).  Then ``main_generator.py --do_train --freeze`` trains two epochs from that
    checkpoint: training loss falling, the forward-only validation loss finite."""
    import main_SimpleDyG
    base = lm_tests._write_lm_dataset(str(tmp_path), v0=15900, n_train=96, n_val=16, n_test=16)
    monkeypatch.chdir(tmp_path)
    out = tmp_path / "out"
    common = (f"--dataset toy --timestamp 4 --output_dir {out} --model_type gpt2 --model_name_or_path gpt2 "
              f"--train_data_file {base}/train.link_prediction --eval_data_file {base}/val.link_prediction "
              f"--eval_data_gt_file {base}/val_gt.link_prediction --test_data_file {base}/test.link_prediction "
              f"--test_data_gt_file {base}/test_gt.link_prediction --block_size 512 --n_layer 1 --n_head 2 --n_embed 64 --seed 3 ")
    buf = io.StringIO()
    with redirect_stdout(buf):
        main_SimpleDyG.main((common + "--do_train --evaluate_during_training --per_gpu_train_batch_size 16 --learning_rate 5e-3 "
                             "--warmup_steps 2 --num_train_epochs 2 --patience 10").split())
    log = buf.getvalue()
    losses = [float(x) for x in re.findall(r"\| train loss: ([0-9.eE+-]+)", log)]
    assert len(losses) == 2 and losses[1] < losses[0], losses
    ck = out / "checkpoint-0"
    sd = torch.load(ck / "pytorch_model.bin", map_location="cpu", weights_only=True)
    assert sd["transformer.wte.weight"].shape[0] > 15872 and all(torch.isfinite(v).all() for v in sd.values())
    buf = io.StringIO()
    with redirect_stdout(buf):
        res = main_SimpleDyG.main((common.replace(str(out), str(ck)) + "--do_eval --per_gpu_eval_batch_size 8").split())
    got = res[str(ck)]
    assert re.search(r"eval_loss = [0-9.]+  NDCG@5 = [0-9.eE+-]+  jaccard = [0-9.eE+-]+", buf.getvalue()), buf.getvalue()[-2000:]
    vals = [got["eval_loss"], got["NDCG"][0], got["jaccard"][0]]
    assert all(v == v and abs(v) != float("inf") for v in (float(x) for x in vals)), got
    assert 0 < float(got["eval_loss"]) < 12, got                                  # ln(V) = 9.7 for an untrained model
    # the next stage on the same vocabulary: main_generator.py --do_train --freeze from that checkpoint (the RAG step's head)
    import main_generator
    import numpy as np
    from test_gpu_generator_training_cli import _gen_argv
    rng = np.random.default_rng(5)
    for split, n in (("train", 96), ("val", 16), ("test", 16)):
        np.savetxt(f"{base}/{split}_index.gen", np.stack([rng.choice(96, 10, replace=False) for _ in range(n)]), fmt="%d")
        np.savetxt(f"{base}/{split}_score.gen", rng.random((n, 10)), fmt="%.6f")
    argv = _gen_argv(base, tmp_path / "gout", ck, "--do_train --num_train_epochs 2 --patience 10")
    argv[argv.index("--n_layer") + 1] = "1"
    buf = io.StringIO()
    with redirect_stdout(buf):
        main_generator.main(argv)
    log = buf.getvalue()
    losses = [float(x) for x in re.findall(r"\| train loss: ([0-9.eE+-]+)", log)]
    val = [float(x) for x in re.findall(r"val loss: ([0-9.eE+-]+)", log)]
    assert len(losses) == 2 and losses[1] < losses[0] and len(val) == 2 and all(v == v and v < 12 for v in val), (losses, val)
    assert "test_metrics last epoch" in log
