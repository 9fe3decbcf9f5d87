"""Training workspace of the shipped script shapes in the four mode combinations (attention stored / recompute x activations
stored / recompute), from the library's three size queries alone: no GPU, no allocation.  The table of DESIGN.md section 7.4.

    python tools/train_workspace_table.py [--json]

Rows are the padded worst case of each script (every sequence at the block size); the retriever step is its five forwards in
one call.  Each cell is the fp32 store's size; the `bf16 store` column beside it is the same query with ``precision="bf16"``,
``act_store="bf16"`` (ln1 of layers >= 1, ln2 and f as bf16 wherever d % 256 == 0).  The `fused` column is the
fp32 store under ``precision="fp32+attn"``, ``attention_kernel="fused"`` (no P-shaped block, one log-sum-exp
per query per layer), which the attention word does not change: it stands beside the two P recompute cells.  The words are those of
``rag4dyg_amd.training.TRAIN_MODE_AXES``, selected through ``TrainModes.select()``; the library's switches are put back afterwards.
Vocabularies: rag4dyg_amd/synth.py (retriever flavour with [MASK], SimpleDyG / generator flavour without)."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rag4dyg_amd import _lib, synth                                            # noqa: E402
from rag4dyg_amd.lm_training import padded_vocab                               # noqa: E402
from rag4dyg_amd.training import TrainModes, saved_library_modes              # noqa: E402

# (kind, label, L, H, d, vocab, batches)
ROWS = [("retriever", "UCI_13 L4 H2 d512 5x(64, 512)", 4, 2, 512, synth.UCI_13.vocab, [(64, 512)] * 5),
        ("retriever", "wikiv2 L2 H6 d768 5x(128, 512)", 2, 6, 768, synth.WIKIV2.vocab, [(128, 512)] * 5),
        ("retriever", "hepth L12 H2 d256 5x(128, 1024)", 12, 2, 256, synth.HEPTH.vocab, [(128, 1024)] * 5),
        ("lm", "UCI_13 L6 H8 d768 (32, 512)", 6, 8, 768, synth.UCI_13.vocab_generator, [(32, 512)]),
        ("lm", "hepth L12 H2 d256 (32, 512)", 12, 2, 256, synth.HEPTH.vocab_generator, [(32, 512)]),
        ("generator", "UCI_13 L6 H8 d768 (32, 513)", 6, 8, 768, synth.UCI_13.vocab_generator, [(32, 513)])]
MODES = [("stored", "stored"), ("recompute", "stored"), ("stored", "recompute"), ("recompute", "recompute")]   # (attention, activations)
# the cells of one (attention, activations) pair, as words of training.TRAIN_MODE_AXES (every axis named: the environment has no say):
# key suffix -> words; the attention_kernel="fused" cell stands beside "recompute" only (the attention word changes nothing there)
BASE = dict(precision="fp32", head_precision="fp32", act_store="fp32", attention_kernel="products")
CELLS = {"": BASE, "_act_store_bf16": dict(BASE, precision="bf16", act_store="bf16")}       # (the layer switch alone changes no size)
FUSED = dict(BASE, precision="fp32+attn", attention_kernel="fused")


def workspace_bytes(lib, kind, L, H, d, V, batches):
    cfg = _lib.GPT2ConfigC(L, H, d, V, 1024, 1e-5)
    if kind == "retriever":
        n = len(batches)
        Bs = (ctypes.c_int32 * n)(*[b for b, _ in batches])
        Ts = (ctypes.c_int32 * n)(*[t for _, t in batches])
        return int(lib.r4d_gpt2_train_workspace_bytes(ctypes.byref(cfg), n, Bs, Ts))
    (B, T), = batches
    fn = lib.r4d_gpt2_lm_train_workspace_bytes if kind == "lm" else lib.r4d_rag_train_workspace_bytes
    return int(fn(ctypes.byref(cfg), B, T, padded_vocab(V)))


def table():
    lib = _lib.load()
    out = []
    with saved_library_modes():
        for kind, label, L, H, d, V, batches in ROWS:
            rec = dict(step=kind, shape=label)

            def cell(**words):
                TrainModes.resolve(**words).select()
                return workspace_bytes(lib, kind, L, H, d, V, batches)
            for att, act in MODES:
                for suffix, words in CELLS.items():
                    rec[f"attention_{att}_activations_{act}{suffix}"] = cell(attention=att, activations=act, **words)
                if att == "recompute":
                    rec[f"attention_fused_activations_{act}"] = cell(attention=att, activations=act, **FUSED)
            out.append(rec)
    return out


def main():
    rows = table()
    if "--json" in sys.argv:
        for r in rows:
            print(json.dumps(r))
        return
    print("| step | shape | P stored, activations stored | bf16 store | P recompute, activations stored | bf16 store | "
          "P stored, activations recompute | bf16 store | P recompute, activations recompute | bf16 store | fused, activations stored | "
          "fused, activations recompute |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        cells = [f"{r[k] / 1e9:.2f} GB" for att, act in MODES
                 for k in (f"attention_{att}_activations_{act}", f"attention_{att}_activations_{act}_act_store_bf16")]
        cells += [f"{r[f'attention_fused_activations_{act}'] / 1e9:.2f} GB" for act in ("stored", "recompute")]
        print(f"| {r['step']} | {r['shape']} | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    main()
