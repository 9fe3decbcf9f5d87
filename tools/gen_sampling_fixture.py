"""Write tests/golden/g15_sampling_filter.npz: the kept sets that the REFERENCE's own functions give on the CPU.

    python tools/gen_sampling_fixture.py [--find-seeds]        (R4D_GOLDEN_OUT=<dir>: write there instead)

For every vocabulary size of tests/_sampling_ref.FIXTURE_SIZES: seeded tie-free logits and a seen mask (``make_logits``), and for
every point of the grid (top_k, top_p, temperature, repetition_penalty) the mask of the logits that are still finite after the
reference's ``enforce_repetition_penalty_``, ``/ temperature`` and ``top_k_top_p_filtering`` (models/modeling_utils.py), imported
from the reference tree and called, not copied.  The float64 restatement must give the same sets, and its margins are asserted
here: no cumulative mass within 1e-4 of its top_p, no logit within 1e-5 (relative) of its top-k threshold -- so a correct kernel
has to match the sets EXACTLY.  ``--find-seeds`` prints, per size, the first seed whose row has those margins (the table
``SEEDS`` of tests/_sampling_ref.py).
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True

import _sampling_ref as sr  # noqa: E402


def find_seeds():
    for V in sr.ALL_SIZES:
        for seed in range(100000):
            x, seen = sr.make_logits(V, seed)
            if np.unique(x).size == V and sr.grid_margins_ok(x, seen):
                print(f"    {V}: {seed},")
                break


def reference_keep(x, seen, top_k, top_p, tau, r):
    from models.modeling_utils import PreTrainedModel, top_k_top_p_filtering
    logits = torch.from_numpy(x.copy()).unsqueeze(0)
    if r != 1.0:
        prev = torch.from_numpy(np.nonzero(seen)[0]).unsqueeze(0)
        PreTrainedModel.enforce_repetition_penalty_(None, logits, 1, 1, prev, r)
    if tau != 1.0:
        logits = logits / tau
    out = top_k_top_p_filtering(logits, top_k=top_k, top_p=top_p)
    return torch.isfinite(out[0]).numpy()


def main():
    if "--find-seeds" in sys.argv:
        return find_seeds()
    from oracle.gen_golden import GOLD, _install_stubs
    _install_stubs()
    out = {"grid": np.asarray(sr.GRID, dtype=np.float64), "sizes": np.asarray(sr.FIXTURE_SIZES, dtype=np.int64)}
    for V in sr.FIXTURE_SIZES:
        x, seen = sr.make_logits(V, sr.SEEDS[V])
        assert np.unique(x).size == V
        keeps = []
        for k, p, t, r in sr.GRID:
            res = sr.sample_row(x, seen, True, t, k, p, r)
            assert res["p_margin"] > sr.P_MARGIN and res["k_margin"] > sr.K_MARGIN, (V, k, p, t, r, res["p_margin"], res["k_margin"])
            ref = reference_keep(x, seen, k, p, t, r)
            assert np.array_equal(ref, res["keep"]), (V, k, p, t, r)
            keeps.append(ref)
        out[f"x_{V}"], out[f"seen_{V}"], out[f"keep_{V}"] = x, sr.pack_bits(seen), sr.pack_bits(np.stack(keeps))
    path = os.path.join(os.environ.get("R4D_GOLDEN_OUT") or GOLD, "g15_sampling_filter.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
