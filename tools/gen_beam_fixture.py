"""Write tests/golden/g16_beam_search.npz: the output ids of the REFERENCE's own ``generate(num_beams > 1, do_sample=False)``.

    python tools/gen_beam_fixture.py        (R4D_GOLDEN_OUT=<dir>: write there instead)

A tiny GPT-2 (vocab 40, 32 positions, n_embd 64, 2 layers, 2 heads; tests/_beam_ref.make_weights: scaled embeddings, the rows of
three ids boosted along ln_f's shift so that hypotheses complete -- a random model almost never emits an eos) is loaded into
the reference's ``GPT2LMHeadModel`` (models/modeling_gpt2.py, imported from the reference tree and called, not copied), and
``generate`` runs every case of tests/_beam_ref.CASES on the CPU.  The fixture holds the weights, the prompts, the arguments and
the reference's ids.  It is written only if
  - the float64 restatement tests/_beam_ref.py gives the reference's ids in every case;
  - every decision of every step of the restatement -- neighbours among the sorted best 2n + 1, ``score > worst``,
    ``worst >= cur_score``, the final sort -- has a margin of at least 1e-3 in log-probability, some hundred times fp32's error
    on scores of magnitude 10: a correct device path has to give the ids EXACTLY;
  - across the cases a prompt is done before max_length, a hypothesis displaces a worse one, a call pads rows of different
    lengths, and a case ends without a finished hypothesis.
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True

import _beam_ref as br  # noqa: E402


def main():
    from oracle.gen_golden import GOLD, _install_stubs, _ref_model
    _install_stubs()
    sd = br.make_weights()
    ref = _ref_model("gpt2", br.N_LAYER, br.N_HEAD, br.N_EMBD, br.VOCAB, br.N_POSITIONS, sd)
    step = br.logits_fn(sd)
    out = {"weights/" + k: v.numpy() for k, v in sd.items() if k != "lm_head.weight"}
    seen = dict(done_early=0, displaced=0, pads=0, unfinished=0)
    for name, case in br.CASES.items():
        prompts, kw = br.case_inputs(case)
        with torch.no_grad():
            got = ref.generate(input_ids=torch.tensor(prompts), do_sample=False, **kw).numpy()
        res = br.beam_search(step, prompts, kw["num_beams"], kw["max_length"], kw.get("eos_token_ids"), kw.get("length_penalty", 1.0),
                             kw.get("repetition_penalty", 1.0), kw.get("pad_token_id"), kw.get("num_return_sequences", 1))
        assert res["ids"].shape == got.shape and np.array_equal(res["ids"], got), (name, res["ids"], got)
        assert res["margin"] >= br.MARGIN, (name, res["margin"])
        for k in seen:
            seen[k] += int(res["stats"][k])
        print(f"  {name}: margin {res['margin']:.2e} {res['stats']} -> {got.shape}")
        out[f"{name}/prompts"], out[f"{name}/ids"] = np.asarray(prompts, dtype=np.int64), got.astype(np.int64)
        out[f"{name}/args"] = np.asarray(json.dumps(kw, sort_keys=True))
    assert all(v > 0 for v in seen.values()), seen
    path = os.path.join(os.environ.get("R4D_GOLDEN_OUT") or GOLD, "g16_beam_search.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", seen)


if __name__ == "__main__":
    main()
