"""GPU tests of the generator-training command line end to end: ``main_SimpleDyG.py --do_train`` writes checkpoint-0, then
``main_generator.py --do_train --freeze --simpledyg_checkpoint ... --fusion graphpooling --m 1`` trains on a synthetic dataset
(with index and score files) and writes the reference's checkpoint, which ``--do_eval`` loads and scores; and the same training
under two ranks (gloo, one GPU) ends with identical parameters on both."""
import io
import os
import re
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from conftest import REPO
from test_gpu_lm_training import _lm_argv, _write_lm_dataset

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def simpledyg(tmp_path_factory):
    """Dataset + retrieval files + a SimpleDyG checkpoint-0 trained by ``main_SimpleDyG.py --do_train``."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import main_SimpleDyG
    root = tmp_path_factory.mktemp("gen")
    base = _write_lm_dataset(str(root), seed=4)
    rng = np.random.default_rng(5)
    for split, n in (("train", 480), ("val", 40), ("test", 40)):
        idx = np.stack([rng.choice(480, 10, replace=False) for _ in range(n)])
        np.savetxt(os.path.join(base, f"{split}_index.gen"), idx, fmt="%d")
        np.savetxt(os.path.join(base, f"{split}_score.gen"), rng.random((n, 10)), fmt="%.6f")
    cwd = os.getcwd()
    os.chdir(root)
    try:
        with redirect_stdout(io.StringIO()):
            main_SimpleDyG.main(_lm_argv(base, root / "sdg", "--num_train_epochs 2 --patience 10"))
    finally:
        os.chdir(cwd)
    return root, base, root / "sdg" / "checkpoint-0"


def _gen_argv(base, out, ck, extra):
    files = " ".join(f"--{s}_{k}_file {base}/{s}_{k}.gen" for s in ("train", "val", "test") for k in ("index", "score"))
    return (f"--dataset toy --timestamp 4 --output_dir {out} --model_type gpt2 --model_name_or_path gpt2 "
            f"--train_data_file {base}/train.link_prediction --eval_data_file {base}/val.link_prediction "
            f"--eval_data_gt_file {base}/val_gt.link_prediction --test_data_file {base}/test.link_prediction "
            f"--test_data_gt_file {base}/test_gt.link_prediction {files} --block_size 512 --n_layer 2 --n_head 2 --n_embed 64 "
            f"--seed 3 --per_gpu_train_batch_size 16 --per_gpu_eval_batch_size 16 --learning_rate 5e-3 --warmup_steps 0 "
            f"--fusion graphpooling --gnn_layers 1 --m 1 --topK 7 --freeze --simpledyg_checkpoint {ck} " + extra).split()


def test_main_generator_do_train_freeze_end_to_end(simpledyg, monkeypatch):
    """Reference checkpoint keys; transformer.* equal to the SimpleDyG checkpoint bit for bit; lm_head.weight untied from wte and
    trained; the epoch loss falls; ``--do_eval`` loads the checkpoint and scores it."""
    import main_generator
    root, base, ck = simpledyg
    monkeypatch.chdir(root)
    out = root / "gout"
    buf = io.StringIO()
    with redirect_stdout(buf):
        main_generator.main(_gen_argv(base, out, ck, "--do_train --num_train_epochs 4 --patience 10"))
    log = buf.getvalue()
    losses = [float(x) for x in re.findall(r"\| train loss: ([0-9.eE+-]+)", log)]
    assert len(losses) == 4 and all(b < a for a, b in zip(losses, losses[1:])), losses
    assert len(re.findall(r"val loss: ([0-9.eE+-]+)", log)) == 4
    assert "test_metrics best epoch" in log and "test_metrics last epoch" in log
    gck = out / "checkpoint-0"
    for f in ("config.json", "pytorch_model.bin", "training_args.bin", "optimizer.pt", "scheduler.pt"):
        assert (gck / f).exists(), f
    got = torch.load(gck / "pytorch_model.bin", map_location="cpu", weights_only=True)
    sdg = torch.load(ck / "pytorch_model.bin", map_location="cpu", weights_only=True)
    assert {"lm_head.weight", "gnn_fusion.convs.0.lin.weight", "gnn_fusion.convs.0.bias"} <= set(got)
    tr_keys = [k for k in sdg if k.startswith("transformer.")]
    assert len(tr_keys) >= 2 + 2 * 12 + 2 and {k for k in got if k.startswith("transformer.")} == set(tr_keys)
    for k in tr_keys:
        assert torch.equal(got[k], sdg[k]), k
    assert got["lm_head.weight"].shape == got["transformer.wte.weight"].shape
    assert not torch.equal(got["lm_head.weight"], got["transformer.wte.weight"])
    assert got["gnn_fusion.convs.0.lin.weight"].shape == (64, 64)
    opt = torch.load(gck / "optimizer.pt", weights_only=False)
    assert len(opt["state"]) == 3 and [len(g["params"]) for g in opt["param_groups"]] == [2, 1]
    with redirect_stdout(io.StringIO()):
        res = main_generator.main(_gen_argv(base, gck, ck, "--do_eval"))
    assert list(res) == [str(gck)] and 0.0 <= res[str(gck)]["NDCG"][0] <= 1.0


_CLI_WORKER = r"""
import hashlib, os, sys
sys.path.insert(0, sys.argv[1])
from rag4dyg_amd import generator_training
import main_generator
orig_train, orig_save = generator_training.train, generator_training.save_checkpoint


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


generator_training.save_checkpoint, generator_training.train = save, train
main_generator.main(sys.argv[2:])
"""


def test_main_generator_do_train_two_ranks(simpledyg, tmp_path):
    """Two ranks as torch.distributed.run starts them (gloo, one GPU), each on its DistributedSampler share: a digest of every
    parameter byte is identical on both ranks after training, and only rank 0 writes the checkpoint."""
    root, base, ck = simpledyg
    out = tmp_path / "out"
    argv = _gen_argv(base, out, ck, "--do_train --num_train_epochs 2 --patience 10 --gradient_accumulation_steps 2")
    script = tmp_path / "gen_worker.py"
    script.write_text(_CLI_WORKER)
    procs = []
    for rk in range(2):
        env = dict(os.environ, R4D_DIST_BACKEND="gloo", PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""),
                   RANK=str(rk), LOCAL_RANK=str(rk), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29573")
        procs.append(subprocess.Popen([sys.executable, str(script), REPO] + argv, cwd=root, env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    done = [pr.communicate(timeout=900) for pr in procs]
    assert all(pr.returncode == 0 for pr in procs), [e[-2500:] for _, e in done]
    digests = [re.findall(r"DIGEST ([0-9a-f]+)", o) for o, _ in done]
    assert len(digests[0]) == 1 and digests[0] == digests[1], digests
    assert "SAVED_BY_RANK 0" in done[0][0] and "SAVED_BY_RANK" not in done[1][0]
    assert (out / "checkpoint-0" / "pytorch_model.bin").exists()
