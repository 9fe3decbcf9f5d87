#!/usr/bin/env python3
"""RAG generator training step (``GeneratorTrainer.step``: weighted bag, GCN projection, the spliced step, fusion backward) at the
reference's script shapes with synthetic inputs: ms per step and tokens/s, frozen (``--freeze``, untied head: the shipped
configuration) and unfrozen (tied); the per-class breakdown of ``r4d_profile_*`` of a frozen step; and as a yardstick the same
frozen step in torch autograd, fp32 on the GPU (a plain-torch GPT-2 with fused causal attention, ``oracle.generator_ref``'s GCN).  Eval mode: no
dropout launches in either.

    python tools/gen_train_bench.py [--steps 10] [--warmup 3] [--shapes uci13,reddit] [--one-step uci13] [--attention stored|recompute] [--activations stored|recompute] [--precision fp32|bf16|fp32+attn|bf16+attn] [--head-precision fp32|bf16] [--act-store fp32|bf16] [--attention-kernel products|fused]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# train_rag_graphpooling_*_seed.sh: UCI_13 L6/H8/d768, reddit L2/H8/d512; batch 32, top-7, one GCN layer, m = 1
SHAPES = {"uci13": dict(L=6, H=8, d=768, V=1800, B=32, T=128),
          "reddit": dict(L=2, H=8, d=512, V=11919, B=32, T=128)}


def _profile(lib):
    out = {}
    for c in range(lib.r4d_profile_num_classes()):
        ms, n, w = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        lib.r4d_profile_read(c, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(w))
        if n.value:
            out[lib.r4d_profile_class_name(c).decode()] = dict(ms=round(ms.value, 4), launches=n.value)
    return dict(sorted(out.items(), key=lambda kv: -kv[1]["ms"]))


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def _setup(s, dev, freeze):
    from oracle import gpt2_ref
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModelRAG
    L, H, d, V, B, T = (s[k] for k in ("L", "H", "d", "V", "B", "T"))
    sd = gpt2_ref.make_state_dict(L, d, V, n_positions=1024, seed=1, random_affine=True)
    sd.pop("lm_head.weight", None)
    m = GPT2LMHeadModelRAG(GPT2Config(vocab_size=V, n_positions=1024, n_ctx=1024, n_embd=d, n_layer=L, n_head=H))
    m.load_state_dict(sd, strict=False)
    m.tie_weights()
    m.get_gnn(d, d // 2, d, 1, 0.2)
    if freeze:
        m.lm_head.weight = torch.nn.Parameter(m.transformer.wte.weight.detach().clone())
    m = m.to(dev).eval()
    rng = np.random.default_rng(0)
    src = [rng.integers(0, V - 1, int(rng.integers(8, 40))).tolist() for _ in range(2000)]
    idx = [rng.choice(len(src), 7, replace=False).tolist() for _ in range(B)]
    tok = torch.from_numpy(rng.integers(0, V - 1, (B, T))).to(dev)
    return m, src, idx, tok


def _gpt2_hidden(sd, x, H, L, eps=1e-5):
    """GPT-2 on inputs_embeds in plain torch ops on the device (fp32, fused causal attention): the yardstick's forward."""
    F = torch.nn.functional
    B, T, d = x.shape
    x = x + sd["transformer.wpe.weight"][:T]
    for i in range(L):
        p = f"transformer.h.{i}."
        h = F.layer_norm(x, (d,), sd[p + "ln_1.weight"], sd[p + "ln_1.bias"], eps)
        q, k, v = (h @ sd[p + "attn.c_attn.weight"] + sd[p + "attn.c_attn.bias"]).split(d, dim=-1)
        q, k, v = (t.view(B, T, H, d // H).transpose(1, 2) for t in (q, k, v))
        a = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(B, T, d)
        x = x + a @ sd[p + "attn.c_proj.weight"] + sd[p + "attn.c_proj.bias"]
        h = F.layer_norm(x, (d,), sd[p + "ln_2.weight"], sd[p + "ln_2.bias"], eps)
        f = F.gelu(h @ sd[p + "mlp.c_fc.weight"] + sd[p + "mlp.c_fc.bias"], approximate="tanh")
        x = x + f @ sd[p + "mlp.c_proj.weight"] + sd[p + "mlp.c_proj.bias"]
    return F.layer_norm(x, (d,), sd["transformer.ln_f.weight"], sd["transformer.ln_f.bias"], eps)


def _torch_step(m, src, idx, tok, H, L):
    """The frozen step in torch autograd, fp32 on the device: the one-layer GCN on a dense A_norm per query, the spliced
    forward, CE over the augmented labels, backward into the head and the GCN weights."""
    from oracle import generator_ref
    dev = tok.device
    sd = {k: v.detach() for k, v in m.named_parameters() if k.startswith("transformer.")}
    conv = m.gnn_fusion.convs[0]
    W = conv.lin.weight.detach().clone().requires_grad_(True)
    b = conv.bias.detach().clone().requires_grad_(True)
    head = m.lm_head.weight.detach().clone().requires_grad_(True)
    graphs = []
    for ix in idx:
        order, edges = generator_ref.star_union_graph(src, ix)
        graphs.append((torch.tensor(order, device=dev), generator_ref.gcn_norm_dense(len(order), edges).to(dev)))
    labels = torch.cat([tok[:, :2], torch.full((tok.shape[0], 1), -100, device=dev), tok[:, 2:]], dim=1)[:, 1:].reshape(-1)

    def step():
        wte = sd["transformer.wte.weight"]
        rows = torch.stack([generator_ref.gcn_conv(wte[o], a, W, b).mean(dim=0) for o, a in graphs])
        Ht = wte[tok]
        h = _gpt2_hidden(sd, torch.cat([Ht[:, :2], rows[:, None], Ht[:, 2:]], dim=1), H, L)
        lg = (h @ head.t())[:, :-1].reshape(-1, head.shape[0])
        torch.nn.functional.cross_entropy(lg, labels, ignore_index=-100).backward()
    return step


def main():
    from rag4dyg_amd import _lib, ops, training
    from rag4dyg_amd.generator_training import GeneratorTrainer, PreparedBags
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="uci13,reddit")
    ap.add_argument("--one-step", default="", metavar="SHAPE",
                    help="one warm-up and ONE timed frozen step at SHAPE, print nothing else (for a kernel trace)")
    training.add_mode_arguments(ap)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    if a.one_step:
        m, src, idx, tok = _setup(SHAPES[a.one_step], dev, freeze=True)
        tr = GeneratorTrainer(m, freeze=True, **training.modes_from_args(a))
        bags = PreparedBags(idx, src, 7).batch(range(len(idx)), dev)
        for _ in range(2):
            tr.step(tok, bags)
            torch.cuda.synchronize()
        return
    for name in a.shapes.split(","):
        s = SHAPES[name]
        rec = dict(shape=name, mode=ops.gemm_mode(), **s, topK=7)
        tokens = s["B"] * (s["T"] + 1)
        for freeze in (True, False):
            m, src, idx, tok = _setup(s, dev, freeze)
            torch.cuda.reset_peak_memory_stats()
            tr = GeneratorTrainer(m, freeze=freeze, **training.modes_from_args(a))
            bags = PreparedBags(idx, src, 7).batch(range(len(idx)), dev)
            ms = _time(lambda: tr.step(tok, bags), a.steps, a.warmup)
            key = "frozen" if freeze else "unfrozen"
            rec[key + "_ms_per_step"] = round(ms, 4)
            rec[key + "_tokens_per_s"] = round(tokens / (ms / 1e3), 1)
            rec[key + "_workspace_bytes"] = int(tr._ws.numel())
            rec[key + "_max_memory_allocated"] = int(torch.cuda.max_memory_allocated())      # model, trainer and the timed steps
            rec.update(tr.modes.record())
            if freeze:
                lib.r4d_profile_enable(1)
                tr.step(tok, bags)
                torch.cuda.synchronize()
                rec["frozen_classes"] = _profile(lib)
                lib.r4d_profile_enable(0)
                rec["torch_autograd_frozen_ms_per_step"] = round(_time(_torch_step(m, src, idx, tok, s["H"], s["L"]), a.steps, a.warmup), 4)
            del tr, m
            torch.cuda.empty_cache()
        rec["frozen_over_unfrozen"] = round(rec["frozen_ms_per_step"] / rec["unfrozen_ms_per_step"], 4)
        rec["frozen_over_torch"] = round(rec["frozen_ms_per_step"] / rec["torch_autograd_frozen_ms_per_step"], 4)
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
