"""CPU-side checks of the encoder's ``"bf16+attn"`` precision (``ops.set_encode_precision``; the GPU side is
tests/test_gpu_encode_bf16_attn.py): the word through its three doors and the library's switch pair behind it, the declared
symbols, the emulation's error table with the conditions the GPU gate rests on, and the prompt seed of the greedy-decoding test."""
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
    return int(lib.r4d_get_encode_bf16()), int(lib.r4d_get_encode_attention_bf16())


def test_the_word_is_accepted_and_the_switch_pair_follows_it():
    from rag4dyg_amd import ops
    was = ops.encode_precision()
    try:
        assert ops.resolve_encode_precision("bf16+attn") == "bf16+attn"
        ops.set_encode_precision("fp32")
        assert _switches() == (0, 0)
        assert ops.set_encode_precision("bf16+attn") == "fp32" and ops.encode_precision() == "bf16+attn" and _switches() == (1, 1)
        assert ops.set_encode_precision("bf16") == "bf16+attn" and ops.encode_precision() == "bf16" and _switches() == (1, 0)
        assert ops.set_encode_precision("bf16+attn") == "bf16" and _switches() == (1, 1)
        assert ops.set_encode_precision("fp32") == "bf16+attn" and ops.encode_precision() == "fp32" and _switches() == (0, 0)
        ops.set_encode_precision("bf16+attn")
        for bad in ("bf16+", "bf16+attention", "fp32+attn", "attn", "BF16+ATTN", "bf16 +attn", None, 2):
            with pytest.raises(ValueError):
                ops.set_encode_precision(bad)
            assert ops.encode_precision() == "bf16+attn" and _switches() == (1, 1)           # a refused word changes nothing
    finally:
        ops.set_encode_precision(was)


def test_the_library_setter_returns_the_previous_setting_and_alone_is_only_a_flag():
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    was = ops.encode_precision()
    try:
        ops.set_encode_precision("fp32")
        assert lib.r4d_set_encode_attention_bf16(1) == 0 and _switches() == (0, 1)           # the GEMM switch is not moved by it
        assert lib.r4d_set_encode_attention_bf16(7) == 1 and _switches() == (0, 1)           # on != 0
        assert lib.r4d_set_encode_attention_bf16(0) == 1 and _switches() == (0, 0)
    finally:
        lib.r4d_set_encode_attention_bf16(0)
        ops.set_encode_precision(was)


def test_resolve_encode_precision_reads_the_word_from_the_environment(monkeypatch):
    from rag4dyg_amd import ops
    monkeypatch.setenv("R4D_ENCODE_PRECISION", "bf16+attn")
    assert ops.resolve_encode_precision() == "bf16+attn" and ops.resolve_encode_precision("bf16") == "bf16"
    monkeypatch.setenv("R4D_ENCODE_PRECISION", "bf16+attn ")
    with pytest.raises(ValueError):
        ops.resolve_encode_precision()


def test_environment_variable_sets_both_library_switches_in_a_fresh_process():
    env = dict(os.environ, R4D_ENCODE_PRECISION="bf16+attn")
    code = ("from rag4dyg_amd import ops, _lib; p = ops.encode_precision(); lib = _lib.load(); "
            "print(p, lib.r4d_get_encode_bf16(), lib.r4d_get_encode_attention_bf16())")
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "bf16+attn 1 1"


def test_declared_symbols_branches_and_abi():
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    assert lib.r4d_abi_version() == 6 == _lib.R4D_ABI_VERSION
    for sym in ("r4d_set_encode_attention_bf16", "r4d_get_encode_attention_bf16", "r4d_attention_bf16_groups"):
        assert hasattr(lib, sym), sym
        assert sym in open(os.path.join(REPO, "include", "r4d.h")).read(), sym
    assert callable(ops.attention_bf16)
    names = [lib.r4d_dispatch_branch_name(i).decode() for i in range(lib.r4d_dispatch_num_branches())]
    mine = [n for n in names if n.startswith("tuning:encode_bf16_attn:")]
    assert len(mine) == 3 and any("fallback" in n for n in mine), mine
    assert [n for n in names if n.startswith("tuning:encode_bf16:")] == ["tuning:encode_bf16:128x256x32", "tuning:encode_bf16:128x128x32"]


def test_emulation_is_the_oracle_with_rounded_conv1d_and_attention_operands_only():
    """The two patches are active only inside the context manager; the attention patch rounds q, k, the probabilities and v and
    nothing else; with ``rounded_rows = n`` the rows behind the prompt take the exact attention."""
    gpt2_ref = E.gpt2_ref
    o_conv, o_attn = gpt2_ref.conv1d, gpt2_ref.attn_core
    g = torch.Generator().manual_seed(4)
    q, k, v = (torch.randn(2, 2, 9, 16, generator=g, dtype=torch.float64) for _ in range(3))
    kt = k.transpose(2, 3)
    with E.patched():
        assert gpt2_ref.conv1d is not o_conv
        a = gpt2_ref.attn_core(q, kt, v)
    assert gpt2_ref.conv1d is o_conv and gpt2_ref.attn_core is o_attn
    bf = R.bf16_round
    w = torch.softmax((bf(q) @ bf(kt) / 4.0).masked_fill(~torch.tril(torch.ones(9, 9, dtype=torch.bool)), float("-inf")), dim=-1)
    assert torch.allclose(a, bf(w) @ bf(v), rtol=0, atol=1e-12) and not torch.allclose(a, o_attn(q, kt, v), rtol=0, atol=1e-6)
    with E.patched(5):
        a5 = gpt2_ref.attn_core(q, kt, v)
    assert torch.equal(a5[:, :, 5:], o_attn(q, kt, v)[:, :, 5:])
    assert torch.allclose(a5[:, :, :5], a[:, :, :5], rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", E.FIXTURES)
def test_emulation_error_table(name):
    """Per fixture and tensor: the float32 and the float64 emulation's distance from the exact float64 forward (max-norm, relative)
    and from each other.  What the GPU gate (e_gpu <= 2 x emu32 on every GATED tensor) rests on: every fixture gates hidden,
    meanpool and the qkv of every layer behind an attention (``E.GATE_FLOOR`` = 1e-4: 100 x the fp32-accurate modes' 1e-6) -- a
    fixture that gates fewer fails here --; on a gated tensor the arithmetic's own error is a bf16 rounding's (below 3e-2), two
    faithful executions differ by less than it, and the float32 figure is within 0.8 .. 1.25 of the float64 one."""
    tab = E.error_table(name)
    L = E.fixture(name)[1]
    assert set(tab) == {"hidden", "meanpool", "logits"} | {f"layer{l}" for l in range(L)} | {f"qkv{l}" for l in range(L)}
    gated = E.gated(name)
    for k, e in tab.items():
        print(f"[encode bf16+attn] {name} {k}: emu32 {e['emu32']:.3e} emu64 {e['emu64']:.3e} emu32 vs emu64 {e['emu32_vs_emu64']:.3e}"
              f"{' GATED' if k in gated else ''}")
    assert E.GATE_FLOOR >= 1e-6
    missing = [k for k in E.must_gate(name) if k not in gated]
    assert not missing, (name, missing)
    assert "layer0" not in gated and tab["layer0"]["emu64"] == 0.0          # the embedding output: no GEMM and no attention has run
    for k in gated:
        e = tab[k]
        assert E.GATE_FLOOR <= e["emu64"] < 3e-2, (name, k, e)
        assert 0.8 < e["emu32"] / e["emu64"] < 1.25, (name, k, e)
        assert e["emu32_vs_emu64"] < e["emu64"], (name, k, e)


def test_layer0_qkv_lies_upstream_of_any_attention():
    """qkv0 of the new word's emulation equals qkv0 of the ``"bf16"`` word's, exactly: the GPU test asks the same of the device."""
    for name in R.FIXTURES:
        for i in (1, 2):
            assert torch.equal(E.references(name)[i]["qkv0"], R.references(name)[i]["qkv0"]), name
            assert not torch.equal(E.references(name)[i]["qkv1"], R.references(name)[i]["qkv1"]), name


def test_greedy_prompt_seed_gives_the_same_ids_in_both_emulations():
    """Test 7 of the GPU file compares the device with the float64 emulation (a bf16+attn prefill of the prompt rows, exact steps):
    with this seed the float32 emulation already agrees with it on all 8 prompts, so a difference on the GPU is the kernel's."""
    sd, _L, H = R.g10_state_dict()
    prompts = E.greedy_prompts()
    assert [len(p) for p in prompts] == list(E.GREEDY_LENGTHS) == [5, 11, 17, 23, 29, 36, 42, 48]
    for p in prompts:
        g32, g64 = E.emulated_greedy(sd, H, p, torch.float32), E.emulated_greedy(sd, H, p, torch.float64)
        assert g32 == g64 and 1 <= len(g64) <= 11, (p, g32, g64)
