"""CPU-side checks of the encoder's opt-in bf16 precision (``ops.set_encode_precision``; the GPU side is
tests/test_gpu_encode_bf16.py): the emulation's error table -- the numbers the GPU test compares the kernels with --, the
switch's argument validation, the environment variable, and the prompt seed of the greedy-decoding test."""
import os
import subprocess
import sys

import pytest
import torch

import _encode_bf16_ref as R
from conftest import REPO


@pytest.mark.parametrize("name", R.FIXTURES)
def test_emulation_error_table(name):
    """Per fixture and tensor: the float32 emulation's and the float64 emulation's distance from the exact float64 forward
    (max-norm, relative), and the two emulations' distance from each other.  What must hold for the GPU test's margin of 2 to
    mean anything: the arithmetic's own error is the bf16 rounding's (1e-3 .. 2e-2, not fp32's 1e-7), two faithful executions
    of it differ by less than that error, and the float32 emulation's error is within 0.8 .. 1.25 of the float64 one's."""
    tab = R.error_table(name)
    L = R.fixture(name)[1]
    assert set(tab) == {"hidden", "meanpool", "logits"} | {f"layer{l}" for l in range(L)} | {f"qkv{l}" for l in range(L)}
    for k, e in tab.items():
        print(f"{name} {k}: emu32 {e['emu32']:.3e} emu64 {e['emu64']:.3e} emu32 vs emu64 {e['emu32_vs_emu64']:.3e}")
        if k == "layer0":                                   # the embedding output: no GEMM has run, fp32 rounding of one add
            assert e["emu64"] == 0.0 and e["emu32"] < 2.0 ** -23
            continue
        assert 5e-4 < e["emu64"] < 2e-2, (name, k, e)
        assert 0.8 < e["emu32"] / e["emu64"] < 1.25, (name, k, e)
        assert e["emu32_vs_emu64"] < e["emu64"], (name, k, e)


def test_emulation_is_the_oracle_with_rounded_conv1d_operands_only():
    """The patch is active only inside the context manager, rounds both operands, and leaves the oracle's file alone."""
    from oracle import gpt2_ref
    orig = gpt2_ref.conv1d
    g = torch.Generator().manual_seed(3)
    x, w, b = torch.randn(5, 64, generator=g), torch.randn(64, 32, generator=g), torch.randn(32, generator=g)
    with R.patched_conv1d():
        y = gpt2_ref.conv1d(x, w, b)
    assert gpt2_ref.conv1d is orig
    assert torch.equal(y, torch.addmm(b, x.bfloat16().float(), w.bfloat16().float()))
    assert not torch.equal(y, gpt2_ref.conv1d(x, w, b))
    with R.patched_conv1d(2):                               # rows 0, 1 rounded, the rest exact
        y2 = gpt2_ref.conv1d(x, w, b)
    assert torch.equal(y2[:2], y[:2]) and torch.equal(y2[2:], gpt2_ref.conv1d(x, w, b)[2:])


def test_set_encode_precision_validates_its_argument():
    from rag4dyg_amd import ops
    was = ops.encode_precision()
    try:
        for bad in ("fp16", "BF16", "", None, 1, "f32"):
            with pytest.raises(ValueError):
                ops.set_encode_precision(bad)
            assert ops.encode_precision() == was            # a refused value changes nothing
        assert ops.set_encode_precision("bf16") == was and ops.encode_precision() == "bf16"
        assert ops.set_encode_precision("fp32") == "bf16" and ops.encode_precision() == "fp32"
    finally:
        ops.set_encode_precision(was)


def test_resolve_encode_precision_reads_the_environment(monkeypatch):
    from rag4dyg_amd import ops
    monkeypatch.delenv("R4D_ENCODE_PRECISION", raising=False)
    assert ops.resolve_encode_precision() == "fp32"
    monkeypatch.setenv("R4D_ENCODE_PRECISION", "")
    assert ops.resolve_encode_precision() == "fp32"
    monkeypatch.setenv("R4D_ENCODE_PRECISION", "bf16")
    assert ops.resolve_encode_precision() == "bf16" and ops.resolve_encode_precision("fp32") == "fp32"
    monkeypatch.setenv("R4D_ENCODE_PRECISION", "half")
    with pytest.raises(ValueError):
        ops.resolve_encode_precision()


@pytest.mark.parametrize("value,want", [(None, "fp32 0"), ("bf16", "bf16 1"), ("fp32", "fp32 0")])
def test_environment_variable_sets_the_library_switch_in_a_fresh_process(value, want):
    """``R4D_ENCODE_PRECISION`` is read once, at the first ``ops.encode_precision()``, and reaches ``r4d_set_encode_bf16``."""
    env = {k: v for k, v in os.environ.items() if k != "R4D_ENCODE_PRECISION"}
    if value is not None:
        env["R4D_ENCODE_PRECISION"] = value
    code = ("from rag4dyg_amd import ops, _lib; p = ops.encode_precision(); "
            "print(p, _lib.load().r4d_get_encode_bf16())")
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == want


def test_greedy_prompt_seed_gives_the_same_ids_in_both_emulations():
    """Test 12 of the GPU file compares the device with the float64 emulation: with this seed the float32 emulation already
    agrees with it on all 8 prompts, so a difference on the GPU is the kernel's."""
    sd, _L, H = R.g10_state_dict()
    prompts = R.greedy_prompts()
    assert [len(p) for p in prompts] == list(R.GREEDY_LENGTHS) == [5, 11, 17, 23, 29, 36, 42, 48]
    for p in prompts:
        g32, g64 = R.emulated_greedy(sd, H, p, torch.float32), R.emulated_greedy(sd, H, p, torch.float64)
        assert g32 == g64 and 1 <= len(g64) <= 11, (p, g32, g64)
