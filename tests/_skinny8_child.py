"""Child process of tests/test_gpu_skinny_gemm.py: the 32-column forms of the weight-stream GEMM (gemm_skinny8_kernel), which the
dispatcher picks only under R4D_SKINNY16=0 -- a word the library reads once per process, so the parent starts this file in a
fresh process with that word set.  K = 512 and 768 at M in {1, 17, 32}, N in {31, 33, 90}: the three epilogues (the residual in
place, as the decode step calls it) and the per-launch LayerNorm; K = 1024, N = 33: split-K plus the epilogue launch; and a folded
LayerNorm, which needs the 16-column kernel and must be refused.  Same set-up and gates as the parent's own cases.  Prints one
JSON line: {"cases": [{label, rho, rho_seq32, hard, measured, ok, problems}], "counters": {name: hits}, "fold_refused": message}."""
import contextlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import _skinny_ref as R  # noqa: E402
from _skinny_run import Runner  # noqa: E402
from rag4dyg_amd import _lib, ops  # noqa: E402

assert os.environ.get("R4D_SKINNY16") == "0", "start this file with R4D_SKINNY16=0"
dev = torch.device("cuda:0")
run = Runner(dev, skinny16=False)
cases = []


def one(label, d, M, N, epilogue, ln=None, inplace=False):
    try:                                        # run.case asserts the set-up, the after-checks and both gates
        with contextlib.redirect_stdout(sys.stderr):            # its [rho] line: stdout carries the JSON line alone
            c, _y = run.case(d, M, N, epilogue, bias=True, ln=ln, inplace=inplace, label=label)
        cases.append({"label": label, "form": run.records[-1][1], "rho": c.last_rho, "rho_seq32": c.rho_seq32, "hard": c.hard,
                      "measured": c.measured, "ok": True, "problems": []})
    except AssertionError as e:
        cases.append({"label": label, "ok": False, "problems": [str(e)[:500]]})


for K in R.S8_KS:
    for N in R.S8_NS:
        d, dl = R.make(32, K, N, seed=8), R.make(32, K, N, seed=8, ln=True)
        for M in R.S8_MS:
            for e in R.EPILOGUES:
                one(f"skinny8 K{K} M{M} N{N} {e}", d, M, N, e, inplace=(e == "residual"))
            one(f"skinny8 K{K} M{M} N{N} layernorm", dl, M, N, "gelu", ln="launch")
K, M, N = R.S8_SPLITK
one(f"skinny8 split-K K{K} N{N}", R.make(M, K, N, seed=8), M, N, "residual", inplace=True)

d = R.make(32, 512, 33, seed=8, ln=True)
t = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
wTg, lnc = ops.fold_layernorm(t["wT"], t["g"], t["beta"])
torch.cuda.synchronize()
_lib.load().r4d_dispatch_reset()
try:
    ops.conv1d_skinny(t["x"], wTg, t["bias"], ln_fold=lnc)
    refused = ""
except _lib.R4DError as e:
    refused = str(e)
torch.cuda.synchronize()
assert run.counters() == {}, "the refused call counted a branch"
print(json.dumps({"cases": cases, "counters": run.total, "fold_refused": refused}))
