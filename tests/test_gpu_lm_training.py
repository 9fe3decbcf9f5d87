"""GPU tests of SimpleDyG LM training (``main_SimpleDyG.py --do_train``): the fused shifted cross-entropy kernel against float64
torch, the whole training step (forward, LM head, cross entropy, backward into every parameter and both parts of the tied wte)
against the oracle's forward + CPU autograd under all three arithmetics, dropout given the same masks, determinism, the optimizer
loop with the linear warm-up schedule, gradient accumulation, and the CLI end to end (one rank and two)."""
import ctypes
import io
import json
import os
import re
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from conftest import REPO, elementwise_err, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _ce(logits, ids, V, T, labels=None, grad_scale=1.0):
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    N, ldV = logits.shape
    ws = ops.workspace(lib.r4d_lm_ce_workspace_bytes(N), logits.device, "lm_ce_test")
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    _lib.check(lib.r4d_lm_ce_f32(logits.data_ptr(), N, V, ldV, ids.data_ptr(), labels.data_ptr() if labels is not None else None, T,
                                 float(grad_scale), loss.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream),
               "lm_ce")
    return loss


@pytest.mark.parametrize("V,B,T,scale,with_labels,gs", [(60, 3, 17, 1.0, False, 1.0), (1800, 4, 64, 30.0, True, 0.5),
                                                         (8814, 32, 512, 1.0, False, 1.0), (8814, 2, 40, 30.0, False, 0.25),
                                                         (11906, 8, 100, 3.0, True, 2.0)])
def test_lm_ce_kernel_equals_float64(dev, V, B, T, scale, with_labels, gs):
    """Loss (relative 1e-6), dlogits element-wise, exact zeros in pad columns and unlabelled rows, bit-identical relaunch."""
    from rag4dyg_amd.lm_training import padded_vocab
    g = torch.Generator().manual_seed(V + T)
    ldV = padded_vocab(V)
    N = B * T
    x = torch.randn(N, V, generator=g) * scale
    ids = torch.randint(0, V, (B, T), generator=g)
    labels = None
    lab = ids.clone()
    if with_labels:
        lab[torch.rand(B, T, generator=g) < 0.3] = -100
        labels = lab.to(dev)
    ref = x.double().requires_grad_(True)
    lv = ref.view(B, T, V)[:, :-1].reshape(-1, V)
    want = torch.nn.functional.cross_entropy(lv, lab[:, 1:].reshape(-1))
    (want * gs).backward()
    logits = torch.zeros(N, ldV, device=dev)
    logits[:, :V] = x.to(dev)
    logits[:, V:] = 7.0                                             # garbage in the pad: never read as a class
    first = logits.clone()
    loss = _ce(logits, ids.to(dev), V, T, labels, gs)
    want = float(want.detach())
    assert abs(float(loss) / want - 1) < 1e-6, (float(loss), want)
    got = logits.cpu()
    assert torch.all(got[:, V:] == 0)
    counted = torch.zeros(B, T, dtype=torch.bool)
    counted[:, :-1] = lab[:, 1:] != -100
    assert torch.all(got[~counted.view(-1)] == 0)
    assert elementwise_err(got[:, :V].numpy(), ref.grad.numpy()) < 1
    again = first.clone()
    loss2 = _ce(again, ids.to(dev), V, T, labels, gs)
    assert torch.equal(again, logits) and torch.equal(loss2, loss)


def _model(dev, L, H, d, V, seed, n_positions=1024):
    from oracle import gpt2_ref
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModel
    sd = gpt2_ref.make_state_dict(L, d, V, n_positions=n_positions, seed=seed, random_affine=True)
    sd.pop("lm_head.weight", None)
    cfg = GPT2Config(vocab_size=V, n_positions=n_positions, n_ctx=n_positions, n_embd=d, n_layer=L, n_head=H)
    m = GPT2LMHeadModel(cfg)
    m.load_state_dict(sd, strict=False)
    m.tie_weights()
    return m.to(dev).eval(), sd


def _ids(V, B, T, seed, pad):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V - 2, (B, T), generator=g)
    for i in range(1, B):                                            # right-padded with the pad id (counted, as upstream)
        n = int(torch.randint(max(3, T // 2), T + 1, (1,), generator=g))
        ids[i, n:] = pad
    return ids


def _oracle(sd, ids, H, drop=None):
    from oracle import gpt2_ref
    sdg = {k: v.clone().double().requires_grad_(True) for k, v in sd.items() if k != "lm_head.weight"}
    sdg["lm_head.weight"] = sdg["transformer.wte.weight"]
    if drop is not None:
        drop.next_group(*ids.shape)
    r = gpt2_ref.gpt2_forward.__wrapped__(sdg, ids, H, want_logits=True, drop=drop)      # grad-enabled
    loss = gpt2_ref.lm_loss(r["logits"], ids)
    loss.backward()
    return float(loss.detach()), {k: v.grad.float() for k, v in sdg.items() if k != "lm_head.weight"}


@pytest.mark.parametrize("L,H,d,V,B,T", [(2, 2, 64, 60, 3, 20),           # tiny
                                         (6, 8, 768, 1800, 4, 64),        # UCI_13 script shape
                                         (2, 6, 768, 8814, 2, 160),       # wikiv2 script shape, > one 128-position tile
                                         (2, 2, 256, 500, 3, 40),         # hepth-like (head_dim 128)
                                         (2, 4, 64, 60, 2, 30)])          # head_dim 16
def test_lm_training_step_gradients_equal_oracle(dev, L, H, d, V, B, T, gemm_mode):
    """(All three arithmetics.)  Loss within 1e-5 and every parameter gradient (wte: embedding scatter + LM head) at max-norm
    < 1e-3 and element-wise (rtol 1e-3, atol 1e-4) against the oracle's float64 autograd; three repeated steps bit-identical."""
    from rag4dyg_amd.lm_training import LMTrainer
    m, sd = _model(dev, L, H, d, V, seed=L * 100 + d + V)
    ids = _ids(V, B, T, seed=V + T, pad=V - 1)
    tr = LMTrainer(m)
    loss = tr.step(ids.to(dev))
    want, ref = _oracle(sd, ids, H)
    assert abs(float(loss) / want - 1) < 1e-5, (float(loss), want)
    worst = {n: rel_err(tr.grads[n].cpu().numpy(), ref[n].numpy()) for n in ref}
    assert max(worst.values()) < 1e-3, {n: e for n, e in worst.items() if e > 1e-3}
    ew = {n: elementwise_err(tr.grads[n].cpu().numpy(), ref[n].numpy(), rtol=1e-3, atol=1e-4) for n in ref}
    assert max(ew.values()) < 1, {n: e for n, e in ew.items() if e >= 1}
    first = {n: t.clone() for n, t in tr.grads.items()}
    for _ in range(2):
        l2 = tr.step(ids.to(dev))
        assert torch.equal(l2, loss)
        assert all(torch.equal(tr.grads[n], first[n]) for n in first)


def test_mean_pool_entries_unchanged_beside_the_lm_step(dev):
    """The retriever's r4d_gpt2_train_*_f32 pair gives the same bits before and after LM steps on the same model."""
    from rag4dyg_amd import training
    from rag4dyg_amd.lm_training import LMTrainer
    m, _sd = _model(dev, 2, 2, 64, 60, seed=5)
    ids = _ids(60, 3, 20, seed=1, pad=59).to(dev)
    enc = training.EncoderTrainer(m)
    emb = enc.forward([ids])
    g1 = {n: t.clone() for n, t in enc.backward(torch.ones_like(emb)).items()}
    lm = LMTrainer(m)
    lm.step(ids)
    emb2 = enc.forward([ids])
    g2 = enc.backward(torch.ones_like(emb2))
    assert torch.equal(emb, emb2) and all(torch.equal(g1[n], g2[n]) for n in g1)


def test_lm_training_step_with_dropout_equals_oracle_given_the_same_masks(dev):
    from oracle import train_ref
    from rag4dyg_amd.lm_training import LMTrainer
    L, H, d, V, B, T = 2, 2, 64, 60, 3, 20
    m, sd = _model(dev, L, H, d, V, seed=11)
    ids = _ids(V, B, T, seed=3, pad=V - 1)
    p = (0.1, 0.1, 0.1)
    tr = LMTrainer(m, dropout=p, seed=1234)
    loss = tr.step(ids.to(dev))
    drop = train_ref.PhiloxDropout(*p, seed=1234, step=tr.enc.step)
    want, ref = _oracle(sd, ids, H, drop=drop)
    assert abs(float(loss) / want - 1) < 1e-5
    worst = {n: rel_err(tr.grads[n].cpu().numpy(), ref[n].numpy()) for n in ref}
    assert max(worst.values()) < 1e-3, worst


def test_three_adamw_steps_with_schedule_track_the_oracle(dev):
    """Warm-up + linear decay + clipping over three updates; the LM-head operand is fresh after every update: the loss of each
    step matches the oracle on the updated weights, and the logits of the trained model equal ``m(ids)[0]``."""
    from oracle import gpt2_ref, train_ref
    from rag4dyg_amd import training
    from rag4dyg_amd.lm_training import LMTrainer, LinearWarmupSchedule, linear_warmup_lambda
    L, H, d, V, B, T = 2, 2, 64, 60, 3, 20
    m, sd = _model(dev, L, H, d, V, seed=21)
    ids = [_ids(V, B, T, seed=s, pad=V - 1) for s in (1, 2, 3)]
    lr, wd, max_norm, warm, total = 3e-3, 0.01, 0.5, 1, 4
    tr = LMTrainer(m)
    opt = training.AdamW(tr.params, tr.grads, lr=lr, eps=1e-8, weight_decay=wd, flat_grads=tr.flat_grads)
    sch = LinearWarmupSchedule(lr, warm, total)
    opt.lr = sch.lr
    lam = linear_warmup_lambda(warm, total)
    P = {k: v.clone().double() for k, v in sd.items()}
    M_ = {k: torch.zeros_like(v) for k, v in P.items()}
    V_ = {k: torch.zeros_like(v) for k, v in P.items()}
    for step, b in enumerate(ids, start=1):
        loss = tr.step(b.to(dev))
        want, ref = _oracle({k: v.float() for k, v in P.items()}, b, H)
        assert abs(float(loss) / want - 1) < 2e-5, (step, float(loss), want)
        opt.step(max_norm)
        sch.step()
        opt.lr = sch.lr
        coef, _ = train_ref.clip_coefficient(list(ref.values()), max_norm)
        step_lr = lr * lam(step - 1)
        for k in ref:
            decay = 0.0 if "bias" in k else wd
            P[k], M_[k], V_[k] = train_ref.adamw_step(P[k], ref[k].double() * coef, M_[k], V_[k], step, step_lr, (0.9, 0.999), 1e-8, decay)
        assert abs(opt.lr - lr * lam(step)) < 1e-12
    worst = max(rel_err(tr.params[k].detach().cpu().numpy(), P[k].numpy()) for k in tr.params)
    assert worst < 1e-3, worst
    with torch.no_grad():
        logits = m(ids[0].to(dev))[0]
    want_logits = gpt2_ref.gpt2_forward({k: v.detach().cpu() for k, v in m.state_dict().items()}, ids[0], H)["logits"]
    assert rel_err(logits.cpu().numpy(), want_logits.numpy()) < 1e-4
    # a fourth step sees the updated weights through its own (refreshed) head operand: its loss is the shifted CE of m(ids)[0]
    loss4 = tr.step(ids[0].to(dev))
    want4 = float(gpt2_ref.lm_loss(logits.double().cpu(), ids[0]))
    assert abs(float(loss4) / want4 - 1) < 2e-5, (float(loss4), want4)


def test_gradient_accumulation_equals_mean_of_micro_batch_gradients(dev):
    from rag4dyg_amd.lm_training import LMTrainer
    m, _sd = _model(dev, 2, 2, 64, 60, seed=31)
    a, b = _ids(60, 3, 20, seed=1, pad=59).to(dev), _ids(60, 3, 20, seed=2, pad=59).to(dev)
    tr = LMTrainer(m)
    tr.step(a)
    ga = tr.flat_grads.clone()
    tr.step(b)
    gb = tr.flat_grads.clone()
    tr.step(a, grad_scale=0.5)
    tr.accumulate()
    tr.step(b, grad_scale=0.5)
    tr.accumulate()
    tr.take_accumulated()
    assert rel_err(tr.flat_grads.cpu().numpy(), ((ga + gb) / 2).cpu().numpy()) < 1e-6


def test_untied_lm_head_is_refused(dev):
    from rag4dyg_amd import _lib
    from rag4dyg_amd.lm_training import LMTrainer
    m, _sd = _model(dev, 1, 2, 64, 60, seed=1)
    m.lm_head.weight = torch.nn.Parameter(m.lm_head.weight.detach().clone())
    with pytest.raises(_lib.R4DError):
        LMTrainer(m)


def _write_lm_dataset(root, ds="toy", t=4, v0=40, n_train=480, n_val=40, n_test=40, seed=0):
    """Reference file grammar; the prediction is a deterministic function of the ego node (a learnable target)."""
    rng = np.random.default_rng(seed)
    base = os.path.join(root, "resources", ds, str(t))
    os.makedirs(base)
    os.makedirs(os.path.join(root, "vocabs", ds, str(t)))
    json.dump({str(i): i for i in range(v0)}, open(os.path.join(root, "vocabs", ds, str(t), "vocab.json"), "w"))

    def hist(ego):
        parts = [f"<|endoftext|> <|history|> {ego}"]
        parts.append("<|time0|> " + " ".join(str(int(x)) for x in rng.integers(0, v0, rng.integers(1, 3))))
        return " ".join(parts) + " <|endofhistory|>"

    def pre(ego):
        return f"<|pre|> <|time{t}|> {(ego * 7 + 3) % v0} {(ego * 3 + 1) % v0} <|endofpre|> <|endoftext|>"
    egos = rng.integers(0, v0, n_train)
    open(os.path.join(base, "train.link_prediction"), "w").write("\n".join(hist(int(e)) + " " + pre(int(e)) for e in egos) + "\n")
    for split, n in (("val", n_val), ("test", n_test)):
        es = rng.integers(0, v0, n)
        open(os.path.join(base, f"{split}.link_prediction"), "w").write("\n".join(hist(int(e)) for e in es) + "\n")
        open(os.path.join(base, f"{split}_gt.link_prediction"), "w").write("\n".join(pre(int(e)) for e in es) + "\n")
    return base


def _lm_argv(base, out, extra):
    return (f"--dataset toy --timestamp 4 --output_dir {out} --model_type gpt2 --model_name_or_path gpt2 "
            f"--train_data_file {base}/train.link_prediction --eval_data_file {base}/val.link_prediction "
            f"--eval_data_gt_file {base}/val_gt.link_prediction --test_data_file {base}/test.link_prediction "
            f"--test_data_gt_file {base}/test_gt.link_prediction --block_size 512 --n_layer 2 --n_head 2 --n_embed 64 --seed 3 "
            f"--do_train --per_gpu_train_batch_size 16 --learning_rate 5e-3 --warmup_steps 5 " + extra).split()


def test_main_simpledyg_do_train_end_to_end(dev, tmp_path, monkeypatch):
    """``main_SimpleDyG.py --do_train``: the average train loss falls, the best weights' test NDCG@5 beats the untrained model's,
    checkpoint-0 holds the six artefacts (optimizer / scheduler loadable by torch), and ``main_retriever.py --do_train
    --should_continue --simpledyg_checkpoint`` starts from it: its transformer weights before the first step are the saved ones."""
    import main_SimpleDyG
    base = _write_lm_dataset(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    out = tmp_path / "out"
    buf = io.StringIO()
    with redirect_stdout(buf):
        main_SimpleDyG.main(_lm_argv(base, out, "--num_train_epochs 8 --patience 10"))
    log = buf.getvalue()
    losses = [float(x) for x in re.findall(r"\| train loss: ([0-9.eE+-]+)", log)]
    assert len(losses) == 8 and all(b < a for a, b in zip(losses, losses[1:])), losses
    ndcg = [float(x) for x in re.findall(r"val_NDCG@5: ([0-9.eE+-]+)", log)]
    assert max(ndcg) > 0, ndcg
    ck = out / "checkpoint-0"
    for f in ("config.json", "pytorch_model.bin", "tokenizer.json", "training_args.bin", "optimizer.pt", "scheduler.pt"):
        assert (ck / f).exists(), f
    sched = torch.optim.lr_scheduler.LambdaLR(torch.optim.SGD([{"params": [torch.zeros(1)]}, {"params": [torch.zeros(1)]}], lr=1.0),
                                              lambda s: 1.0)
    sched.load_state_dict(torch.load(ck / "scheduler.pt", weights_only=False))
    opt_sd = torch.load(ck / "optimizer.pt", weights_only=False)
    assert len(opt_sd["param_groups"]) == 2 and len(opt_sd["state"]) > 0
    sd = torch.load(ck / "pytorch_model.bin", map_location="cpu", weights_only=True)
    assert "lm_head.weight" in sd and all(torch.isfinite(v).all() for v in sd.values())
    assert "top_k_scores_test" in log
    # untrained model, same evaluation: the trained one predicts the deterministic targets better
    from rag4dyg_amd.evaluation import get_eval_metrics
    ns = main_SimpleDyG.parse(main_SimpleDyG.SIMPLEDYG, "main_SimpleDyG.py", _lm_argv(base, tmp_path / "o2", ""))
    ns.with_mask_token = False
    ns.device, ns.n_gpu = dev, 1
    ns.para_names, ns.para_values = ["x"], ["y"]
    from rag4dyg_amd.tokenizer import get_model_tokenizer
    m0, tok, _cls, ns = get_model_tokenizer(ns, main_SimpleDyG.MODEL_CLASSES)
    best = main_SimpleDyG.GPT2LMHeadModel.from_pretrained(str(ck)).to(dev)       # checkpoint-0 holds the best weights
    with redirect_stdout(io.StringIO()):
        base_ndcg = get_eval_metrics(ns, m0.to(dev), tok, 0, mode="test")["NDCG"][0]
        best_test = get_eval_metrics(ns, best, tok, 0, mode="test")["NDCG"][0]
    assert best_test > base_ndcg, (best_test, base_ndcg)
    # the next stage: main_retriever.py --do_train --should_continue --simpledyg_checkpoint checkpoint-0 starts from the saved
    # transformer (its own tokenizer adds [MASK]: one more wte row, the saved rows unchanged)
    import main_retriever
    from rag4dyg_amd import annotation, training
    np.random.seed(1)
    annotation.main(["retrieval_data_annotation.py", "toy", "4", "0.3"])
    ret = tmp_path / "resources" / "toy" / "4" / "train_retrieval"
    torch.save(torch.rand(480) * 20, tmp_path / "resources" / "toy_train_query_time.pt")
    seen = {}

    class Spy(training.EncoderTrainer):                              # built by training.train before its first step
        def __init__(self, model, *a, **k):
            seen.update({n: p.detach().cpu().clone() for n, p in model.transformer.state_dict().items()})
            super().__init__(model, *a, **k)
    monkeypatch.setattr(training, "EncoderTrainer", Spy)
    rargv = (f"--dataset toy --timestamp 4 --output_dir {tmp_path / 'rout'} --model_type gpt2 --model_name_or_path gpt2 "
             f"--train_data_file {base}/train.link_prediction --train_pair_data_file {ret}/train_index.retrieval "
             f"--eval_data_file {base}/val.link_prediction --eval_data_gt_file {ret}/val_score.retrieval "
             f"--test_data_file {base}/test.link_prediction --test_data_gt_file {ret}/test_score.retrieval "
             f"--block_size 512 --n_layer 2 --n_head 2 --n_embed 64 --topK 5 --seed 3 --do_train --should_continue "
             f"--simpledyg_checkpoint {ck} --max_steps 2 --per_gpu_train_batch_size 16 --learning_rate 1e-3 --warmup_steps 0 "
             f"--lambda_decay 0.05 --alpha 0.1 --temperature 0.2 --patience 10").split()
    with redirect_stdout(io.StringIO()):
        main_retriever.main(rargv)
    compared = 0
    for k, v in seen.items():
        want = sd.get("transformer." + k)
        if want is None:
            continue
        if k == "wte.weight":
            assert v.shape[0] == want.shape[0] + 1
            v = v[:want.shape[0]]
        assert torch.equal(v, want), k
        compared += 1
    assert compared >= 2 + 2 * 12 + 2, compared


def test_main_simpledyg_early_stopping_at_patience(dev, tmp_path, monkeypatch):
    """A validation score that falls after the first epoch stops training after --patience epochs; checkpoint-0 is epoch 0's."""
    import main_SimpleDyG
    from rag4dyg_amd import evaluation
    base = _write_lm_dataset(str(tmp_path), seed=1)
    monkeypatch.chdir(tmp_path)
    scores = iter([0.5, 0.4, 0.3, 0.2, 0.1, 0.05, 0.01, 0.0])
    calls = []

    def fake(args, model, tokenizer, step, mode="val"):
        calls.append(mode)
        return {"NDCG": [next(scores) if len(calls) <= 8 and mode == "val" else 0.0], "jaccard": [0.0]}
    monkeypatch.setattr(evaluation, "get_eval_metrics", fake)
    out = tmp_path / "out"
    buf = io.StringIO()
    with redirect_stdout(buf):
        main_SimpleDyG.main(_lm_argv(base, out, "--num_train_epochs 8 --patience 2"))
    log = buf.getvalue()
    assert "Early Stopping" in log
    assert len(re.findall(r"val_NDCG@5:", log)) == 3                 # epoch 0 best, epochs 1 and 2 count, stop
    assert (out / "checkpoint-0" / "optimizer.pt").exists()


_CLI_WORKER = r"""
import hashlib, os, sys
sys.path.insert(0, sys.argv[1])
from rag4dyg_amd import lm_training
import main_SimpleDyG
orig_train, orig_save = lm_training.train, lm_training.save_checkpoint


def save(*a, **k):
    print("SAVED_BY_RANK", os.environ["RANK"], flush=True)
    return orig_save(*a, **k)


def train(args, ds, model, tok):
    r = orig_train(args, ds, model, tok)
    h = hashlib.sha256()
    for k, v in sorted(model.state_dict().items()):
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    print("DIGEST", h.hexdigest(), flush=True)
    return r


lm_training.save_checkpoint, lm_training.train = save, train
main_SimpleDyG.main(sys.argv[2:])
"""


def test_main_simpledyg_do_train_two_ranks(dev, tmp_path):
    """Two ranks as torch.distributed.run starts them (gloo, one GPU), each on its own DistributedSampler share: a digest of
    every parameter byte is identical on both ranks after training (broadcast at the start, averaged gradients every update),
    and only rank 0 writes checkpoints."""
    base = _write_lm_dataset(str(tmp_path), seed=2)
    out = tmp_path / "out"
    argv = _lm_argv(base, out, "--num_train_epochs 2 --patience 10 --gradient_accumulation_steps 2")
    script = tmp_path / "cli_worker.py"
    script.write_text(_CLI_WORKER)
    procs = []
    for rk in range(2):
        env = dict(os.environ, R4D_DIST_BACKEND="gloo", PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""),
                   RANK=str(rk), LOCAL_RANK=str(rk), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29563")
        procs.append(subprocess.Popen([sys.executable, str(script), REPO] + argv, cwd=tmp_path, env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    done = [pr.communicate(timeout=900) for pr in procs]
    assert all(pr.returncode == 0 for pr in procs), [e[-2500:] for _, e in done]
    digests = [re.findall(r"DIGEST ([0-9a-f]+)", o) for o, _ in done]
    assert len(digests[0]) == 1 and digests[0] == digests[1], digests
    assert "SAVED_BY_RANK 0" in done[0][0] and "SAVED_BY_RANK" not in done[1][0]
    assert (out / "checkpoint-0" / "pytorch_model.bin").exists()


_DP_WORKER = r"""
import os, sys
import torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from test_gpu_lm_training import _ids, _model
from rag4dyg_amd import training
from rag4dyg_amd.lm_training import LMTrainer
rank = int(os.environ["RANK"])
dist.init_process_group(backend="gloo")
dev = torch.device("cuda:0")
m, _sd = _model(dev, 2, 2, 64, 60, seed=41)
tr = LMTrainer(m)
opt = training.AdamW(tr.params, tr.grads, lr=1e-3, weight_decay=0.01, flat_grads=tr.flat_grads)
tr.step(_ids(60, 3, 20, seed=100 + rank, pad=59).to(dev))          # every rank its own batch
local = tr.flat_grads.clone()
tr.all_reduce_mean()
both = [torch.empty_like(local) for _ in range(2)]
dist.all_gather(both, local)
want = (both[0].double() + both[1].double()) / 2
err = float((tr.flat_grads.double() - want).abs().max() / want.abs().max())
assert float((both[0] - both[1]).abs().max()) > 0, "the two ranks saw the same batch"
assert err < 1e-6, err
opt.step(1.0)
flat_p = torch.cat([p.detach().reshape(-1) for p in tr.params.values()])
ps = [torch.empty_like(flat_p) for _ in range(2)]
dist.all_gather(ps, flat_p)
assert torch.equal(ps[0], ps[1]), "parameters diverged across ranks"
print("DP_OK", err)
dist.destroy_process_group()
"""


def test_data_parallel_lm_step_averages_gradients_over_ranks(dev, tmp_path):
    """Two ranks (gloo, one GPU) step on DIFFERENT batches: the gradient the optimizer sees is the mean of the two local
    gradients, and the updated parameters are bit-identical on both ranks."""
    script = tmp_path / "dp_worker.py"
    script.write_text(_DP_WORKER)
    procs = [subprocess.Popen([sys.executable, str(script), REPO],
                              env=dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                                       MASTER_PORT="29564"),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs) and all("DP_OK" in o for o in outs), [o[-2000:] for o in outs]


@pytest.mark.parametrize("name", ["cfg1_simpledyg"])
def test_lm_step_loss_equals_reference_g3(dev, name, gemm_mode):
    """(All three arithmetics.)  The training step's loss in eval mode on the G3 fixture (L6 H8 d768 V1800, the fixture's own
    weights recipe) equals the loss recorded from the reference within the 1e-4 of test_encoder_g3_config_shapes."""
    from conftest import load_golden
    from rag4dyg_amd.lm_training import LMTrainer
    g = load_golden("g3_" + name)
    L, H, d, V, B, T, seed = (int(x) for x in g["cfg"])
    m, _sd = _model(dev, L, H, d, V, seed=seed)
    tr = LMTrainer(m)
    loss = tr.step(torch.as_tensor(g["ids"]).to(dev))
    assert abs(float(loss) - float(g["loss"])) < 1e-4, (float(loss), float(g["loss"]))


def test_out_of_range_label_raises_the_range_flag(dev):
    """A label outside [0, V) that is not -100 is not counted (like ignore_index) AND raises R4D_RANGE_BAD_LABEL."""
    from rag4dyg_amd import ops
    ops.range_flag(dev)
    ops.take_range_flag()
    V, B, T = 60, 2, 8
    ids = torch.randint(0, V, (B, T)).to(dev)
    logits = torch.randn(B * T, 128, device=dev)
    _ce(logits, ids, V, T)
    assert ops.take_range_flag() == 0
    lab = ids.clone()
    lab[0, 3] = -100
    _ce(torch.randn(B * T, 128, device=dev), ids, V, T, labels=lab)
    assert ops.take_range_flag() == 0
    lab[1, 2] = V
    _ce(torch.randn(B * T, 128, device=dev), ids, V, T, labels=lab)
    assert ops.take_range_flag() & ops.RANGE_BAD_LABEL
