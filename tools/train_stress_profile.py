"""CPU measurement behind ``tests/_training_stress_cases.py:K`` (profiles/train_stress_parity.md, first table): for every entry
of the training stress table the float32 reference's error against the float64 oracle under the four CPU summation orders, the
per-tensor spread of that error (K = 2 x the largest spread, within [1.5, 10]), the value of every capped measure, and the
attention / GELU statistics of the inputs.  Reference only: nothing here runs on, or knows of, the device.

    python tools/train_stress_profile.py [entry id substring ...]
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402

import _training_stress_cases as C  # noqa: E402


def main(argv):
    rows, worst = [], (1.0, None, None)
    print("| entry | spread (tensor) | max-norm e_ref | element-wise | loss | emb / hidden | row-max median per layer | max abs c_fc pre-act "
          "(share in 4..8) | s |")
    print("|---|---|---|---|---|---|---|---|---|")
    for e in C.ENTRIES:
        if argv and not any(a in C.entry_id(e) for a in argv):
            continue
        t0 = time.time()
        p = C.reference_profile(e)
        spread, name = C.order_spread(p)
        if spread > worst[0]:
            worst = (spread, C.entry_id(e), name)
        med, pre = C.attention_and_gelu_statistics(e)
        share = float(((np.abs(pre) > 4) & (np.abs(pre) < 8)).mean())
        meds = " / ".join("-" if m is None else f"{m:.2f}" for m in med)
        print(f"| {C.entry_id(e)} | {spread:.2f} ({name}) | {max(p.e_ref.values()):.1e} | {p.ew_ref:.3f} | {p.loss_ref:.1e} | "
              f"{p.hidden_ref:.1e} | {meds} | {np.abs(pre).max():.1f} ({100 * share:.1f} %) | {time.time() - t0:.1f} |", flush=True)
        rows.append(spread)
    k = min(max(2 * worst[0], 1.5), 10.0)
    print(f"\nlargest spread {worst[0]:.2f} ({worst[1]}, {worst[2]}): K = 2 x that = {2 * worst[0]:.2f} (clamped to [1.5, 10]: {k:.2f}); "
          f"the module's K is {C.K}")


if __name__ == "__main__":
    main(sys.argv[1:])
