"""CPU-side checks of the bf16 encoder's activation store (``ops.set_encode_act_store``, ``r4d_set_encode_act_bf16``; the GPU side
is tests/test_gpu_encode_bf16_act.py): the word through its three doors and the library switch behind it, the declared symbols and
branch counters, and the one fact the store rests on -- rounding to bf16 (nearest even) is idempotent, so an activation rounded
once where it is produced gives the bf16 GEMM the operand it would have rounded while staging, and the emulations the GPU gates
of ``"bf16"`` and ``"bf16+attn"`` compare with are unchanged."""
import os
import subprocess
import sys

import pytest
import torch

import _encode_bf16_attn_ref as E
import _encode_bf16_ref as R
from conftest import REPO


def _switches():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    return int(lib.r4d_get_encode_bf16()), int(lib.r4d_get_encode_attention_bf16()), int(lib.r4d_get_encode_act_bf16())


@pytest.fixture(autouse=True)
def restore():
    from rag4dyg_amd import ops
    prec, store = ops.encode_precision(), ops.encode_act_store()
    yield
    ops.set_encode_precision(prec)
    ops.set_encode_act_store(store)


def test_default_is_fp32_and_the_setter_returns_the_previous_word():
    from rag4dyg_amd import ops
    if not os.environ.get("R4D_ENCODE_ACT_STORE"):
        assert ops.encode_act_store() == "fp32" and ops.resolve_encode_act_store() == "fp32"
    ops.set_encode_act_store("fp32")
    assert _switches()[2] == 0
    assert ops.set_encode_act_store("bf16") == "fp32" and ops.encode_act_store() == "bf16" and _switches()[2] == 1
    assert ops.set_encode_act_store("bf16") == "bf16" and _switches()[2] == 1
    assert ops.set_encode_act_store("fp32") == "bf16" and ops.encode_act_store() == "fp32" and _switches()[2] == 0


def test_a_refused_word_raises_and_changes_nothing():
    from rag4dyg_amd import ops
    for held in ("bf16", "fp32"):
        ops.set_encode_act_store(held)
        for bad in ("bf16+attn", "BF16", "fp16", "bf16 ", "", "on", None, 1, True):
            with pytest.raises(ValueError):
                ops.set_encode_act_store(bad)
            assert ops.encode_act_store() == held and _switches()[2] == (held == "bf16")


def test_the_store_and_the_precision_word_do_not_move_each_other():
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    ops.set_encode_precision("fp32")
    ops.set_encode_act_store("bf16")
    assert _switches() == (0, 0, 1)                                       # alone it is only a flag
    for word, pair in (("bf16", (1, 0)), ("bf16+attn", (1, 1)), ("fp32", (0, 0))):
        ops.set_encode_precision(word)
        assert _switches() == pair + (1,) and ops.encode_act_store() == "bf16"
    ops.set_encode_precision("bf16+attn")
    ops.set_encode_act_store("fp32")
    assert _switches() == (1, 1, 0) and ops.encode_precision() == "bf16+attn"
    assert lib.r4d_set_encode_act_bf16(7) == 0 and _switches() == (1, 1, 1)      # on != 0; the library setter returns the previous setting
    assert lib.r4d_set_encode_act_bf16(0) == 1 and _switches() == (1, 1, 0)


def test_resolve_reads_the_word_from_the_environment(monkeypatch):
    from rag4dyg_amd import ops
    monkeypatch.delenv("R4D_ENCODE_ACT_STORE", raising=False)
    assert ops.resolve_encode_act_store() == "fp32"
    monkeypatch.setenv("R4D_ENCODE_ACT_STORE", "")
    assert ops.resolve_encode_act_store() == "fp32"
    monkeypatch.setenv("R4D_ENCODE_ACT_STORE", "bf16")
    assert ops.resolve_encode_act_store() == "bf16" and ops.resolve_encode_act_store("fp32") == "fp32"
    for bad in ("bf16 ", "1", "bf16+attn"):
        monkeypatch.setenv("R4D_ENCODE_ACT_STORE", bad)
        with pytest.raises(ValueError):
            ops.resolve_encode_act_store()


@pytest.mark.parametrize("env, want", (({"R4D_ENCODE_ACT_STORE": "bf16", "R4D_ENCODE_PRECISION": "bf16+attn"}, "bf16+attn bf16 1 1 1"),
                                        ({"R4D_ENCODE_ACT_STORE": "bf16"}, "fp32 bf16 0 0 1"), ({}, "fp32 fp32 0 0 0")))
def test_environment_variable_is_read_at_the_first_use_of_the_precision_word_in_a_fresh_process(env, want):
    """The encoder entries ask for ``ops.encode_precision()``: that first call resolves the store as well."""
    base = {k: v for k, v in os.environ.items() if k not in ("R4D_ENCODE_ACT_STORE", "R4D_ENCODE_PRECISION")}
    code = ("from rag4dyg_amd import ops, _lib; p = ops.encode_precision(); lib = _lib.load(); "
            "print(p, ops._ENCODE_ACT_STORE, lib.r4d_get_encode_bf16(), lib.r4d_get_encode_attention_bf16(), lib.r4d_get_encode_act_bf16())")
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=dict(base, **env), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == want


def test_an_invalid_environment_value_raises_in_a_fresh_process():
    env = dict(os.environ, R4D_ENCODE_ACT_STORE="half")
    r = subprocess.run([sys.executable, "-c", "from rag4dyg_amd import ops; ops.encode_act_store()"], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "ValueError" in r.stderr and "half" in r.stderr


def test_declared_symbols_branches_and_abi():
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    assert lib.r4d_abi_version() == 6 == _lib.R4D_ABI_VERSION            # additive symbols only
    header = open(os.path.join(REPO, "include", "r4d.h")).read()
    for sym in ("r4d_set_encode_act_bf16", "r4d_get_encode_act_bf16"):
        assert hasattr(lib, sym), sym
        assert sym in header and sym in open(os.path.join(REPO, "INTEGRATION.md")).read(), sym
    assert callable(ops.encode_act_store) and callable(ops.set_encode_act_store) and callable(ops.resolve_encode_act_store)
    names = [lib.r4d_dispatch_branch_name(i).decode() for i in range(lib.r4d_dispatch_num_branches())]
    mine = [n for n in names if n.startswith("tuning:encode_act_bf16:")]
    assert mine == ["tuning:encode_act_bf16:ln1", "tuning:encode_act_bf16:ln2", "tuning:encode_act_bf16:f", "tuning:encode_act_bf16:kept fp32"]


def test_route_rule_is_the_plain_bf16_route_of_producer_and_consumer():
    """``r4d_conv1d_route`` (kind 0 encode, bf16 = 1): the route the rule of csrc/conv1d_route.h asks of c_attn, c_fc and mlp.c_proj.
    With the bf16x3 planes (have bit 2) every encoder shape with K % 32 == 0 is on the bf16 kernel (route 3), without them none is."""
    from rag4dyg_amd import _lib
    lib = _lib.load()
    for d in (64, 256, 320, 768):
        for M in (1, 5, 129, 4000):
            for K, N, epi in ((d, 3 * d, 0), (d, 4 * d, 1), (4 * d, d, 2)):
                assert lib.r4d_conv1d_route(0, M, K, N, epi, 1 | 2 | 8, 1) == 3, (d, M, K, N)
                assert lib.r4d_conv1d_route(0, M, K, N, epi, 1 | 8, 1) != 3, (d, M, K, N)


def test_rounding_to_bf16_is_idempotent_on_the_emulations_tensors():
    """RN_bf16(RN_bf16(t)) == RN_bf16(t), bit for bit, on every tensor of the emulations (and on the values rounding treats apart:
    ties, the largest finite bf16, subnormals, signed zeros, infinities); NaN stays NaN."""
    for name in ("L2_d64_T40", "L2_d256_T130"):
        for ref in R.references(name)[1:] + E.references(name)[1:]:
            for k, t in ref.items():
                once = t.to(torch.bfloat16)
                assert torch.equal(once.to(t.dtype).to(torch.bfloat16).view(torch.int16), once.view(torch.int16)), (name, k)
    edge = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.3895e38, 3.4e38, 1e-40, -1e-40, 0.0, -0.0, float("inf"), -float("inf"),
                         2.0 ** -133, 65504.0, -1.0 - 2.0 ** -9])
    once = edge.to(torch.bfloat16)
    assert torch.equal(once.float().to(torch.bfloat16).view(torch.int16), once.view(torch.int16))
    assert bool(torch.tensor([float("nan")]).to(torch.bfloat16).float().to(torch.bfloat16).isnan().all())


@pytest.mark.parametrize("module", (R, E), ids=("bf16", "bf16+attn"))
def test_storing_once_at_the_producer_leaves_the_emulation_unchanged(module):
    """The emulation with every Conv1D input rounded to bf16 BEFORE it reaches the (rounding) patched ``conv1d`` -- the producer's
    store -- returns the tensors of the emulation itself, exactly, in float32 and in float64: the references of the existing GPU
    gates hold for the switch on as they do for the switch off."""
    name = "L2_d64_T40"
    sd, L, H, d, V, P, ids = module.fixture(name)
    gpt2_ref = R.gpt2_ref
    for i, dtype in ((1, torch.float64), (2, torch.float32)):
        want = module.references(name)[i]
        qkv = []
        ctx = R.patched_conv1d("all", qkv) if module is R else E.patched("all", qkv)
        with ctx:
            inner = gpt2_ref.conv1d
            gpt2_ref.conv1d = lambda x, w, b: inner(R.bf16_round(x), w, b)
            try:
                r = gpt2_ref.gpt2_forward(R.cast_sd(sd, dtype), ids, H, want_logits=True, want_layers=True)
            finally:
                gpt2_ref.conv1d = inner
        assert torch.equal(r["hidden"], want["hidden"]) and torch.equal(r["logits"], want["logits"]), (name, dtype)
        for l in range(L):
            assert torch.equal(qkv[l], want[f"qkv{l}"]) and torch.equal(r["layers"][l], want[f"layer{l}"]), (name, dtype, l)
