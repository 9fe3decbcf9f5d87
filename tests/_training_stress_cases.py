"""Shared case table, input generators and CPU oracles of the training stress tests (``test_host_training_stress.py`` on the
CPU, ``test_gpu_training_stress.py`` on the device).  Nothing here touches the GPU.

A WEIGHT SET is built from committed fixtures plus the committed transforms (``conftest.g13_state_dict``) or from a seed through
``sharpen_attention(stress_transform(make_state_dict(...)), f)``; an ENTRY is one training step on a weight set: which trainer
(``enc`` = EncoderTrainer with a loss linear in the mean-pooled embeddings, ``lm`` = LMTrainer, ``gen`` = frozen GeneratorTrainer
with an untied head, ``gen_tied`` = the unfrozen tied one), the batch sizes and lengths, and which of the absolute caps it
carries beside the yardstick bound.

The oracles are ONE calculus evaluated in float64 (the truth) and in float32 on the CPU under the summation orders a CPU
offers -- 1 and 16 threads, batch rows in given and reversed order -- (the reference's own arithmetic: the yardstick)."""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from conftest import elementwise_err, g13_state_dict, rel_err

# ---------------------------------------------------------------------------------------------------------------- the bounds
# K: allowance of the yardstick bound  e_dev[n] <= K * max(e_ref[n], E_FLOOR)  for "a different but legitimate fp32 summation
# order".  Measured on the CPU from the reference alone, before any device run: 2 x the largest per-tensor ratio
# max(e_ref) / min(e_ref) (both floored at E_FLOOR) over the four CPU orders, over every entry below and the fp16-range case;
# never below 1.5 (tools/h2_check.py's factor for one GEMM), never above 10.  The measurement is the first table of
# profiles/train_stress_parity.md (tools/train_stress_profile.py): largest ratios 3.89 (fp16-range case, attn.c_proj.bias) and
# 3.65 (enc on s6_d512_h2 at T 257, ln_f.bias), every other entry <= 1.89; 2 x 3.89 = 7.79, rounded up.
K = 8.0
E_FLOOR = 2e-6                       # an fp32 dot product against float64 (test_weight_gradient_equals_float64)
LOSS_CAP, NORM_CAP, EW_CAP, HIDDEN_CAP = 1e-5, 1e-3, 1.0, 1e-4
EW_RTOL, EW_ATOL = 1e-3, 1e-4
GELU_SAT_FACTOR = 8.0                # c_fc weight and bias of every block: max |pre-activation| >= 10, >= 1 % in 4 < |x| < 8
ORDERS = ((1, False), (16, False), (1, True), (16, True))           # (CPU threads, batch rows reversed)

# ---------------------------------------------------------------------------------------------------------------- weight sets
G13_CASES = ("hd128_plain", "hd128_stress", "hd128_peaked", "hd64_peaked", "hd32_peaked", "hd256_peaked", "hd96_peaked")
#            name: (L, H, d, V, seed, sharpen factor, c_fc factor)
SEEDED = {"s4_d512_h8": (2, 8, 512, 600, 4108, 4.0, 1.0),
          "s6_d512_h2": (2, 2, 512, 600, 6102, 6.0, 1.0),
          "s6_d768_h6": (2, 6, 768, 600, 6706, 6.0, 1.0),           # the wikiv2 script shape
          "s6_t1024": (1, 2, 256, 300, 6124, 6.0, 1.0),             # head_dim 128: wide enough to be peaked at T = 1024
          "gelusat": (2, 2, 256, 500, 4256, 4.0, GELU_SAT_FACTOR),
          "gelusat_l1": (1, 2, 256, 500, 4257, 4.0, GELU_SAT_FACTOR),
          "s4_l1": (1, 2, 256, 500, 4258, 4.0, 1.0)}


def saturate_gelu(sd, factor):
    """GELU-SATURATION input generator: every block's ``mlp.c_fc`` weight and bias x ``factor`` (pre-activations far into both
    tails of gelu_new and through the 1 - tanh^2 cancellation region).  Like the two committed transforms it is applied
    identically before the oracle and the device load the weights.  Returns a new dict."""
    out = {k: v.clone() for k, v in sd.items() if k != "lm_head.weight"}
    for k in out:
        if ".mlp.c_fc." in k:
            out[k] *= float(factor)
    return out


@functools.lru_cache(maxsize=None)
def weights(name):
    """(state dict without ``lm_head.weight``, n_head) of one weight set."""
    from oracle import gpt2_ref
    if name in G13_CASES:
        return g13_state_dict(name)
    if name == "f16_range":
        return f16_range_weights()[:2]
    L, H, d, V, seed, sharpen, cfc = SEEDED[name]
    sd = gpt2_ref.make_state_dict(L, d, V, n_positions=1024, seed=seed, random_affine=True)
    sd = gpt2_ref.sharpen_attention(gpt2_ref.stress_transform(sd), sharpen)
    sd = {k: v for k, v in sd.items() if k != "lm_head.weight"}
    if cfc != 1.0:
        sd = saturate_gelu(sd, cfc)
    return sd, H


# ---------------------------------------------------------------------------------------------------------------- entries
# kind: enc | lm | gen | gen_tied.  Bs / Ts: one element per group (enc may have several); for gen* T is the length the
# transformer sees (tokens + the one fused row).  A cap is carried only where the float32 reference leaves room for it
# (test_host_training_stress.py asserts K * reference <= cap for every cap an entry carries).  peaked: the oracle's softmax
# row-max median over rows with more than 8 keys is >= 0.3 in some layer.
Entry = namedtuple("Entry", "weights kind Bs Ts caps peaked")
# caps: "e" = the element-wise cap applies, "h" = the embeddings / hidden-rows cap applies (the loss and max-norm caps always do)
ENTRIES = [
    Entry("hd128_plain", "lm", (2,), (129,), "eh", False),
    Entry("hd128_stress", "lm", (2,), (256,), "eh", False),
    Entry("hd128_peaked", "lm", (3,), (128,), "h", True),
    Entry("hd128_peaked", "enc", (4,), (2,), "eh", False),
    Entry("hd64_peaked", "enc", (2,), (127,), "eh", True),
    Entry("hd32_peaked", "gen", (2,), (129,), "eh", True),
    Entry("hd256_peaked", "lm", (2,), (255,), "h", True),
    Entry("hd96_peaked", "lm", (2,), (129,), "h", True),
    Entry("s4_d512_h8", "lm", (2,), (257,), "eh", True),
    Entry("s4_d512_h8", "enc", (2, 3, 1), (129, 37, 256), "eh", True),
    Entry("s4_d512_h8", "gen", (3,), (128,), "eh", True),
    Entry("s4_d512_h8", "gen_tied", (2,), (130,), "eh", True),
    Entry("s6_d512_h2", "lm", (1,), (509,), "h", True),
    Entry("s6_d512_h2", "enc", (2,), (257,), "eh", True),
    Entry("s6_d768_h6", "lm", (2,), (160,), "h", True),
    Entry("s6_d768_h6", "gen", (2,), (256,), "e", True),
    Entry("s6_t1024", "lm", (1,), (1024,), "eh", True),
    Entry("s6_t1024", "gen", (1,), (1024,), "eh", True),
    Entry("gelusat", "lm", (3,), (40,), "eh", False),
    Entry("gelusat_l1", "enc", (3,), (40,), "eh", False),
    Entry("gelusat_l1", "enc", (3,), (1,), "eh", False),
]


def entry_id(e):
    return f"{e.weights}-{e.kind}-T{'_'.join(str(t) for t in e.Ts)}"


ENTRY_IDS = [entry_id(e) for e in ENTRIES]


def _ids(V, B, T, seed):
    """Random ids over V - 2 tokens, rows 1.. right-padded with V - 1 (as the ``_ids`` helpers of the step tests)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V - 2, (B, T), generator=g)
    for i in range(1, B):
        lo = min(max(3, T // 2), T)
        n = int(torch.randint(lo, T + 1, (1,), generator=g))
        ids[i, n:] = V - 1
    return ids


@functools.lru_cache(maxsize=None)
def inputs(e):
    """Everything one entry's step needs beside the weights, as CPU tensors / lists (deterministic in the entry)."""
    sd, H = weights(e.weights)
    V, d = sd["transformer.wte.weight"].shape
    seed = 1000 * len(e.Ts) + sum(e.Ts) + 7 * sum(e.Bs) + d
    g = torch.Generator().manual_seed(seed + 1)
    if e.kind == "enc":
        ids = [_ids(V, B, T, seed + 10 * j) for j, (B, T) in enumerate(zip(e.Bs, e.Ts))]
        return {"ids": ids, "G": torch.randn(sum(e.Bs), d, generator=g)}
    if e.kind == "lm":
        return {"ids": _ids(V, e.Bs[0], e.Ts[0], seed)}
    B, T = e.Bs[0], e.Ts[0] - 1
    rng = np.random.default_rng(seed)
    src = [rng.integers(0, V - 2, int(rng.integers(5, 16))).tolist() for _ in range(40)]
    idx = [rng.choice(40, 7, replace=False).tolist() for _ in range(B)]
    out = {"tok": _ids(V, B, T, seed), "idx": idx, "src": src,
           "gcn_w": torch.randn(d, d, generator=g) * 0.05, "gcn_b": torch.randn(d, generator=g) * 0.05}
    if e.kind == "gen":
        out["head"] = torch.randn(V, d, generator=g) * 0.05               # the untied head of load_and_freeze_params
    return out


# ---------------------------------------------------------------------------------------------------------------- oracles
def _leaves(sd, dtype, grad=True):
    sdg = {k: v.detach().clone().to(dtype).requires_grad_(grad) for k, v in sd.items() if k != "lm_head.weight"}
    sdg["lm_head.weight"] = sdg["transformer.wte.weight"]
    return sdg


def _grads(sdg):
    return {k: v.grad.double().numpy() for k, v in sdg.items() if k != "lm_head.weight"}


def oracle(e, dtype=torch.float64, reverse=False):
    """One entry's step in ``dtype`` on the CPU: {"loss", "grads" (name -> float64 numpy), "emb" / "hidden" where the device
    hands them out}.  ``reverse``: the batch rows in reversed order (the same sums in another order); row-indexed outputs are
    returned in the GIVEN order."""
    from oracle import generator_ref, gpt2_ref
    sd, H = weights(e.weights)
    x = inputs(e)
    fwd = gpt2_ref.gpt2_forward.__wrapped__                                 # grad-enabled
    flip = (lambda t: t.flip(0)) if reverse else (lambda t: t)
    if e.kind == "enc":
        sdg = _leaves(sd, dtype)
        groups = list(reversed(x["ids"])) if reverse else x["ids"]
        embs = [fwd(sdg, flip(ids), H, want_logits=False)["hidden"].mean(dim=1) for ids in groups]
        embs = [flip(t) for t in embs]
        emb = torch.cat(list(reversed(embs)) if reverse else embs)          # given order
        loss = (emb * x["G"].to(dtype)).sum()
        loss.backward()
        return {"loss": float(loss.detach()), "grads": _grads(sdg), "emb": emb.detach().double().numpy()}
    if e.kind == "lm":
        sdg = _leaves(sd, dtype)
        ids = flip(x["ids"])
        loss = gpt2_ref.lm_loss(fwd(sdg, ids, H, want_logits=True)["logits"], ids)
        loss.backward()
        return {"loss": float(loss.detach()), "grads": _grads(sdg)}
    freeze = e.kind == "gen"
    sdg = _leaves(sd, dtype, grad=not freeze)
    W = x["gcn_w"].detach().clone().to(dtype).requires_grad_(True)
    b = x["gcn_b"].detach().clone().to(dtype).requires_grad_(True)
    wte = sdg["transformer.wte.weight"]
    tok = flip(x["tok"])
    rows = []
    for ix in (list(reversed(x["idx"])) if reverse else x["idx"]):
        order, edges = generator_ref.star_union_graph(x["src"], ix[:7])
        a = generator_ref.gcn_norm_dense(len(order), edges).to(dtype)
        rows.append(generator_ref.gcn_conv(wte[torch.tensor(order)], a, W, b).mean(dim=0))
    Ht = wte[tok]
    H_aug = torch.cat([Ht[:, :2], torch.stack(rows)[:, None], Ht[:, 2:]], dim=1)
    head = None
    if freeze:
        head = x["head"].detach().clone().to(dtype).requires_grad_(True)
        sdg["lm_head.weight"] = head
    r = fwd(sdg, None, H, inputs_embeds=H_aug, want_logits=True)
    labels = torch.cat([tok[:, :2], torch.full((tok.shape[0], 1), -100), tok[:, 2:]], dim=1)
    lg = r["logits"][:, :-1].reshape(-1, r["logits"].shape[-1])
    loss = torch.nn.functional.cross_entropy(lg, labels[:, 1:].reshape(-1), ignore_index=-100)
    loss.backward()
    grads = {"gnn_fusion.convs.0.lin.weight": W.grad.double().numpy(), "gnn_fusion.convs.0.bias": b.grad.double().numpy()}
    if freeze:
        grads["lm_head.weight"] = head.grad.double().numpy()
    else:
        grads.update(_grads(sdg))
    return {"loss": float(loss.detach()), "grads": grads, "hidden": flip(r["hidden"].detach()).double().numpy()}


def max_norm_errs(got, ref):
    """e[n] = max |g - g64| / max |g64| per tensor."""
    return {n: rel_err(got[n], ref[n]) for n in ref}


Profile = namedtuple("Profile", "ref64 e_orders e_ref ew_ref loss_ref hidden_ref")


@functools.lru_cache(maxsize=None)
def reference_profile(e):
    """The float64 oracle of an entry and the float32 reference's errors against it under every CPU order:
    ``e_orders`` (list of {name: e}), ``e_ref`` (their max per tensor: the yardstick, independent of the thread count of the
    machine that runs the test), ``ew_ref`` / ``loss_ref`` / ``hidden_ref`` (the worst value of each capped measure)."""
    was = torch.get_num_threads()
    try:
        torch.set_num_threads(16)
        ref64 = oracle(e, torch.float64)
        e_orders, ew, lo, hid = [], 0.0, 0.0, 0.0
        for threads, rev in ORDERS:
            torch.set_num_threads(threads)
            r = oracle(e, torch.float32, reverse=rev)
            e_orders.append(max_norm_errs(r["grads"], ref64["grads"]))
            ew = max(ew, max(elementwise_err(r["grads"][n], ref64["grads"][n], rtol=EW_RTOL, atol=EW_ATOL) for n in ref64["grads"]))
            if e.kind != "enc":                                             # enc: the "loss" is the test's own sum(emb * G), not an output
                lo = max(lo, abs(r["loss"] / ref64["loss"] - 1))
            for key in ("emb", "hidden"):
                if key in ref64:
                    hid = max(hid, rel_err(r[key], ref64[key]))
    finally:
        torch.set_num_threads(was)
    e_ref = {n: max(o[n] for o in e_orders) for n in ref64["grads"]}
    return Profile(ref64, e_orders, e_ref, ew, lo, hid)


def order_spread(p):
    """Per tensor: largest / smallest float32-reference error over the CPU orders, both floored at E_FLOOR (below the floor
    the bound does not look at the reference).  Returns (worst ratio, its tensor name)."""
    worst, name = 1.0, None
    for n in p.e_ref:
        vals = [max(o[n], E_FLOOR) for o in p.e_orders]
        r = max(vals) / min(vals)
        if r > worst:
            worst, name = r, n
    return worst, name


# ---------------------------------------------------------------------------------------------------------------- statistics
@torch.no_grad()
def attention_and_gelu_statistics(e):
    """float64, no grad, first group of the entry: per layer the median softmax row maximum over rows with more than 8 keys
    (None when T <= 9), and all ``c_fc`` pre-activations (flat)."""
    from oracle import gpt2_ref
    sd, H = weights(e.weights)
    sd = {k: v.double() for k, v in sd.items()}
    x = inputs(e)
    if e.kind == "enc":
        emb = sd["transformer.wte.weight"][x["ids"][0]]
    elif e.kind == "lm":
        emb = sd["transformer.wte.weight"][x["ids"]]
    else:
        emb = torch.from_numpy(oracle_h_aug(e))
    layers = gpt2_ref.gpt2_forward(sd, None, H, inputs_embeds=emb, want_logits=False, want_layers=True)["layers"]
    medians, pre = [], []
    for i in range(gpt2_ref.n_layers_of(sd)):
        p = f"transformer.h.{i}."
        xin = layers[i]
        B, T, d = xin.shape
        hd = d // H
        ln1 = gpt2_ref.layer_norm(xin, sd[p + "ln_1.weight"], sd[p + "ln_1.bias"])
        q, k, _v = gpt2_ref.conv1d(ln1, sd[p + "attn.c_attn.weight"], sd[p + "attn.c_attn.bias"]).split(d, dim=2)
        q = q.view(B, T, H, hd).permute(0, 2, 1, 3)
        k = k.view(B, T, H, hd).permute(0, 2, 3, 1)
        w = torch.matmul(q, k) / math.sqrt(hd)
        mask = torch.tril(torch.ones(T, T, dtype=w.dtype))
        w = torch.softmax(w * mask - 1e4 * (1 - mask), dim=-1)
        medians.append(float(w.max(dim=-1).values[:, :, 9:].median()) if T > 9 else None)
        x_mid = xin + gpt2_ref.attention(ln1, sd, p + "attn.", H)
        ln2 = gpt2_ref.layer_norm(x_mid, sd[p + "ln_2.weight"], sd[p + "ln_2.bias"])
        pre.append(gpt2_ref.conv1d(ln2, sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"]).reshape(-1))
    return medians, torch.cat(pre).numpy()


@torch.no_grad()
def oracle_h_aug(e):
    """The spliced input embeddings of a gen* entry in float64 (tokens, the fused row at position 2)."""
    from oracle import generator_ref
    sd, _H = weights(e.weights)
    x = inputs(e)
    wte = sd["transformer.wte.weight"].double()
    rows = []
    for ix in x["idx"]:
        order, edges = generator_ref.star_union_graph(x["src"], ix[:7])
        a = generator_ref.gcn_norm_dense(len(order), edges).double()
        rows.append(generator_ref.gcn_conv(wte[torch.tensor(order)], a, x["gcn_w"].double(), x["gcn_b"].double()).mean(dim=0))
    Ht = wte[x["tok"]]
    return torch.cat([Ht[:, :2], torch.stack(rows)[:, None], Ht[:, 2:]], dim=1).numpy()


# ---------------------------------------------------------------------------------------------------------------- fp16 range
F16_RANGE_WEIGHTS, F16_RANGE_B, F16_RANGE_T, F16_RANGE_COLUMN = "s4_l1", 2, 24, 5
F16_RANGE_LIMIT = 2.0 ** 18          # csrc/gemm_h2.hip: the A operand's hi term overflows fp16 beyond it


@functools.lru_cache(maxsize=None)
def f16_range_weights():
    """The one-layer weight set with ONE ``c_fc`` output column (weight and bias) scaled until the float64 oracle's GELU output
    in that column exceeds 1.5 x 2^18: an activation the f16x2 forward GEMM of ``mlp.c_proj`` cannot represent.  The factor is
    chosen from the float64 oracle on the CPU.  Returns (state dict, n_head, largest GELU output)."""
    from oracle import gpt2_ref
    sd, H = weights(F16_RANGE_WEIGHTS)
    e = f16_range_entry(base=True)
    _med, pre = attention_and_gelu_statistics(e)
    d = sd["transformer.wte.weight"].shape[1]
    col = pre.reshape(-1, 4 * d)[:, F16_RANGE_COLUMN]
    factor = 1.5 * F16_RANGE_LIMIT / float(col.max())
    assert col.max() > 0 and factor > 1
    out = {k: v.clone() for k, v in sd.items()}
    out["transformer.h.0.mlp.c_fc.weight"][:, F16_RANGE_COLUMN] *= factor
    out["transformer.h.0.mlp.c_fc.bias"][F16_RANGE_COLUMN] *= factor
    top = float(gpt2_ref.gelu_new(torch.from_numpy(col * factor)).max())
    return out, H, top


def f16_range_entry(base=False):
    return Entry(F16_RANGE_WEIGHTS if base else "f16_range", "lm", (F16_RANGE_B,), (F16_RANGE_T,), "", False)
