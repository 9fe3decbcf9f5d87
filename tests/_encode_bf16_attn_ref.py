"""The test-side reference of the encoder's ``"bf16+attn"`` precision (tests/test_gpu_encode_bf16_attn.py,
tests/test_host_encode_bf16_attn.py).  It extends tests/_encode_bf16_ref.py (``R``) and tests/_train_bf16_attn_ref.py (``A``) and
modifies nothing of them.

"The emulation": the oracle's forward with ``R.patched_conv1d`` (both operands of the four Conv1D GEMMs rounded through
``torch.bfloat16``) TOGETHER WITH ``gpt2_ref.attn_core`` replaced by ``A.attn_core_bf16`` without dropout -- the oracle's attention
line by line with its two ``matmul``s on bf16-rounded operands: q and k, and the (normalised) probabilities and v.  Both are
patched into ``oracle.gpt2_ref`` by module name while a context manager is active; the file under oracle/ is not edited.  The scale
division, the mask and the softmax stay in the dtype of the state dict.  (The device rounds the UNNORMALISED probabilities and
divides by the fp32 row sum afterwards -- csrc/attention_b1.hip; the emulation's rounding of the normalised ones is the same
arithmetic up to where one 2^-9 rounding falls, which is what the factor 2 of the GPU gate is for.)

References per fixture: the exact float64 forward, the float64 emulation, the float32 emulation -- computed once per process and
shared (callers must not modify them).
"""
import contextlib
import functools

import torch

import _encode_bf16_ref as R
import _train_bf16_attn_ref as A

gpt2_ref = R.gpt2_ref
WORD = "bf16+attn"
# A tensor is GATED on the GPU where the arithmetic's own error (float64 emulation against the exact float64 forward, max-norm,
# relative) is at least this: 100 x the 1e-6 of the fp32-accurate modes, a twentieth of one bf16 rounding (2^-9 = 2e-3).  Below
# it the float32 emulation's figure is fp32 noise and "2 x" of it gates nothing meaningful (layer0, qkv0's upstream).
GATE_FLOOR = 1e-4

# name -> (L, H, d, V, n_positions, B, T, ids seed): head dims 64 and 96 beside R's 32, 128 and 256
SEEDED = {"L2_hd64_T70": (2, 2, 128, 60, 160, 3, 70, 201), "L2_hd96_T45": (2, 2, 192, 60, 160, 3, 45, 202)}
PEAKED = "L2_hd128_peaked_T100"           # stress_transform + sharpen_attention(4): every logit x 16, as G13's hd128_peaked
FIXTURES = R.FIXTURES + tuple(SEEDED) + (PEAKED,)


@functools.lru_cache(maxsize=None)
def fixture(name):
    """-> (state dict, L, H, d, V, n_positions, ids int64 [B, T]), as ``R.fixture``"""
    if name in R.FIXTURES:
        return R.fixture(name)
    if name == PEAKED:
        L, H, d, V, P, B, T, seed = 2, 1, 128, 60, 160, 3, 100, 203
        sd = gpt2_ref.sharpen_attention(gpt2_ref.stress_transform(gpt2_ref.make_state_dict(L, d, V, n_positions=P, seed=seed, random_affine=True)), 4.0)
    else:
        L, H, d, V, P, B, T, seed = SEEDED[name]
        sd = gpt2_ref.make_state_dict(L, d, V, n_positions=P, seed=seed, random_affine=True)
    ids = torch.randint(0, V - 1, (B, T), generator=torch.Generator().manual_seed(seed))
    return sd, L, H, d, V, P, ids


def attn_core_bf16_rows(n):
    """``gpt2_ref.attn_core`` whose first ``n`` query rows take ``A.attn_core_bf16`` over the first n keys (the bf16+attn PREFILL of
    a prompt of n tokens) and whose later rows stay exact (the fp32 cached decode step); n = None: every row"""
    orig = gpt2_ref.attn_core

    def attn_core(q, k, v, drop=None):
        assert drop is None
        if n is None or n >= q.shape[2]:
            return A.attn_core_bf16(q, k, v)
        a = orig(q, k, v).clone()
        a[:, :, :n] = A.attn_core_bf16(q[:, :, :n], k[..., :n], v[:, :, :n])
        return a
    return attn_core


@contextlib.contextmanager
def patched(rounded_rows="all", record=None):
    """The emulation of ``"bf16+attn"``: ``R.patched_conv1d(rounded_rows, record)`` and the attention of the same rows"""
    orig = gpt2_ref.attn_core
    with R.patched_conv1d(rounded_rows, record):
        gpt2_ref.attn_core = attn_core_bf16_rows(None if rounded_rows == "all" else int(rounded_rows))
        try:
            yield
        finally:
            gpt2_ref.attn_core = orig


def forward(sd, ids, H, dtype, rounded):
    """``R.forward`` under this module's emulation -> dict: hidden, meanpool, logits, layer<l>, qkv<l>"""
    if not rounded:
        return R.forward(sd, ids, H, dtype, False)
    qkv = []
    with patched("all", qkv):
        r = gpt2_ref.gpt2_forward(R.cast_sd(sd, dtype), ids, H, want_logits=True, want_layers=True)
    out = {"hidden": r["hidden"], "meanpool": r["hidden"].mean(dim=1), "logits": r["logits"]}
    L = gpt2_ref.n_layers_of(sd)
    assert len(qkv) == L
    for l in range(L):
        out[f"layer{l}"] = r["layers"][l]
        out[f"qkv{l}"] = qkv[l]
    return out


@functools.lru_cache(maxsize=None)
def references(name):
    """-> (exact float64 forward, float64 emulation, float32 emulation) of a fixture"""
    sd, L, H, d, V, P, ids = fixture(name)
    exact = R.references(name)[0] if name in R.FIXTURES else forward(sd, ids, H, torch.float64, False)
    return exact, forward(sd, ids, H, torch.float64, True), forward(sd, ids, H, torch.float32, True)


@functools.lru_cache(maxsize=None)
def error_table(name):
    """tensor name -> dict(emu32, emu64, emu32_vs_emu64), as ``R.error_table``"""
    exact, e64, e32 = references(name)
    return {k: dict(emu32=R.rel(e32[k], exact[k]), emu64=R.rel(e64[k], exact[k]), emu32_vs_emu64=R.rel(e32[k], e64[k])) for k in exact}


def gated(name):
    """The tensors of a fixture the GPU gate holds: those whose float64-emulation error reaches ``GATE_FLOOR``"""
    return tuple(k for k, e in error_table(name).items() if e["emu64"] >= GATE_FLOOR)


def must_gate(name):
    """What every fixture has to gate at the least: hidden, meanpool and the qkv of every layer behind an attention"""
    return ("hidden", "meanpool") + tuple(f"qkv{l}" for l in range(1, fixture(name)[1]))


# ------------------------------------------------------------------------------------------- greedy decoding
GREEDY_SEED = 1                       # chosen so that the float32 and the float64 emulation give the same ids on all 8 prompts
GREEDY_LENGTHS = R.GREEDY_LENGTHS
EOS_ID = R.EOS_ID


def greedy_prompts(seed=GREEDY_SEED):
    return R.greedy_prompts(seed)


def emulated_greedy(sd, H, prompt, dtype):
    """``R.emulated_greedy`` under this module's emulation: a bf16+attn prefill of the prompt rows, exact steps behind it"""
    with patched(len(prompt)):
        return gpt2_ref.greedy_decode(R.cast_sd(sd, dtype), H, prompt, EOS_ID, "val")[len(prompt):]


def emulated_logits_at(sd, H, prompt):
    sd64 = R.cast_sd(sd, torch.float64)

    def at(prefix):
        with patched(len(prompt)):
            return gpt2_ref.gpt2_forward(sd64, torch.tensor([list(prompt) + list(prefix)]), H)["logits"][0, -1].numpy()
    return at
