"""The test-side reference of the encoder's opt-in bf16 precision (tests/test_gpu_encode_bf16.py, tests/test_host_encode_bf16.py).

"The emulation": the oracle's forward (oracle/gpt2_ref.py) with ``gpt2_ref.conv1d`` replaced, while a context manager is active,
by a version that rounds ``x`` and ``weight`` through ``torch.bfloat16`` before ``addmm`` -- the oracle's functions call ``conv1d``
by module name, so the file under oracle/ is not edited.  Everything else (LayerNorm, attention, gelu_new, the residual adds, the
LM head) stays in the dtype of the state dict: float64 or float32.  The "exact" forward is the unpatched oracle in float64.

Fixtures, emulation results and the error table are computed once per process and shared (callers must not modify them).
"""
import contextlib
import functools
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import gpt2_ref  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


@contextlib.contextmanager
def patched_conv1d(rounded_rows="all", record=None):
    """``rounded_rows``: "all" -- every row's product is bf16(x) . bf16(W); an int n -- only the first n rows of the (batch of
    one) call, the others take the exact product (greedy decoding: bf16 prefill of the prompt, unchanged steps); None -- no
    rounding (only ``record``).  ``record``: a list that receives every c_attn output (weight [d, 3d]) in call order."""
    orig = gpt2_ref.conv1d

    def conv1d(x, weight, bias):
        x2 = x.reshape(-1, x.shape[-1])
        if rounded_rows == "all":
            y = torch.addmm(bias, bf16_round(x2), bf16_round(weight))
        else:
            y = torch.addmm(bias, x2, weight)
            if rounded_rows:
                n = min(int(rounded_rows), x2.shape[0])
                y[:n] = torch.addmm(bias, bf16_round(x2[:n]), bf16_round(weight))
        y = y.view(x.shape[:-1] + (weight.shape[1],))
        if record is not None and weight.shape[1] == 3 * weight.shape[0]:
            record.append(y)
        return y
    gpt2_ref.conv1d = conv1d
    try:
        yield
    finally:
        gpt2_ref.conv1d = orig


def cast_sd(sd, dtype):
    out = {k: v.to(dtype) for k, v in sd.items() if k != "lm_head.weight"}
    out["lm_head.weight"] = sd["lm_head.weight"].to(dtype) if "lm_head.weight" in sd and not torch.equal(
        sd["lm_head.weight"], sd["transformer.wte.weight"]) else out["transformer.wte.weight"]
    return out


def forward(sd, ids, H, dtype, rounded):
    """-> dict of named tensors: hidden, meanpool, logits, layer<l> (the residual stream ENTERING block l), qkv<l>."""
    qkv = []
    with patched_conv1d("all" if rounded else None, qkv):
        r = gpt2_ref.gpt2_forward(cast_sd(sd, dtype), ids, H, want_logits=True, want_layers=True)
    out = {"hidden": r["hidden"], "meanpool": r["hidden"].mean(dim=1), "logits": r["logits"]}
    L = gpt2_ref.n_layers_of(sd)
    assert len(qkv) == L
    for l in range(L):
        out[f"layer{l}"] = r["layers"][l]
        out[f"qkv{l}"] = qkv[l]
    return out


def g10_state_dict(stress=False):
    gw = np.load(os.path.join(GOLDEN, "g10_trained_small.npz"))
    sd = {n[2:]: torch.from_numpy(gw[n]) for n in gw.files if n.startswith("w:")}
    sd["lm_head.weight"] = sd["transformer.wte.weight"]
    if stress:
        sd = gpt2_ref.stress_transform(sd)
    return sd, int(gw["n_layer"]), int(gw["n_head"])


# name -> (L, H, d, V, n_positions, B, T, ids seed)
SEEDED = {"L2_d64_T40": (2, 2, 64, 60, 160, 3, 40, 101), "L2_d256_T130": (2, 2, 256, 60, 160, 3, 130, 102),
          "L4_d512_T96": (4, 2, 512, 60, 160, 3, 96, 103)}
FIXTURES = tuple(SEEDED) + ("g10_trained", "g10_stress")


@functools.lru_cache(maxsize=None)
def fixture(name):
    """-> (state dict, L, H, d, V, n_positions, ids int64 [B, T])"""
    if name in SEEDED:
        L, H, d, V, P, B, T, seed = SEEDED[name]
        sd = gpt2_ref.make_state_dict(L, d, V, n_positions=P, seed=seed, random_affine=True)
    else:
        sd, L, H = g10_state_dict(stress=name == "g10_stress")
        V, d = sd["transformer.wte.weight"].shape
        P, B, T, seed = sd["transformer.wpe.weight"].shape[0], 3, 48, 104
    ids = torch.randint(0, V - 1, (B, T), generator=torch.Generator().manual_seed(seed))
    return sd, L, H, d, V, P, ids


def rel(a, ref):
    a, ref = a.double(), ref.double()
    return float((a - ref).abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=None)
def references(name):
    """-> (exact float64 forward, float64 emulation, float32 emulation) of a fixture"""
    sd, L, H, d, V, P, ids = fixture(name)
    return (forward(sd, ids, H, torch.float64, False), forward(sd, ids, H, torch.float64, True),
            forward(sd, ids, H, torch.float32, True))


@functools.lru_cache(maxsize=None)
def error_table(name):
    """tensor name -> dict(emu32 = max|float32 emulation - exact64| / max|exact64| (the figure the GPU is compared with),
    emu64 = the same of the float64 emulation (the arithmetic's own error), emu32_vs_emu64)"""
    exact, e64, e32 = references(name)
    return {k: dict(emu32=rel(e32[k], exact[k]), emu64=rel(e64[k], exact[k]), emu32_vs_emu64=rel(e32[k], e64[k])) for k in exact}


# ------------------------------------------------------------------------------------------- greedy decoding (test 12)
GREEDY_SEED = 1                       # chosen so that the float32 and the float64 emulation give the same ids on all 8 prompts
GREEDY_LENGTHS = (5, 11, 17, 23, 29, 36, 42, 48)
EOS_ID = 1781                         # <|endoftext|> of the UCI_13 vocabulary the g10 checkpoint was trained on


def greedy_prompts(seed=GREEDY_SEED):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 1781, (n,), generator=g).tolist() for n in GREEDY_LENGTHS]       # ordinary tokens only


def emulated_greedy(sd, H, prompt, dtype):
    """The oracle's val-mode greedy loop (full forward on the growing sequence) with the rows of the PROMPT positions rounded and
    the rows of generated positions exact: the bf16 prefill plus the unchanged fp32 cached steps.  -> the generated ids."""
    with patched_conv1d(len(prompt)):
        return gpt2_ref.greedy_decode(cast_sd(sd, dtype), H, prompt, EOS_ID, "val")[len(prompt):]


def emulated_logits_at(sd, H, prompt):
    """``logits_at`` of conftest.assert_tokens_equal_or_tie: the float64 emulation's last-position logits behind a prefix."""
    sd64 = cast_sd(sd, torch.float64)

    def at(prefix):
        with patched_conv1d(len(prompt)):
            return gpt2_ref.gpt2_forward(sd64, torch.tensor([list(prompt) + list(prefix)]), H)["logits"][0, -1].numpy()
    return at
