"""CPU-side checks of the training steps' opt-in bf16 precision (``training.resolve_train_precision``; the GPU side is
tests/test_gpu_train_bf16.py): the library's new symbols and its unchanged ABI, the resolver and its environment variable, the
emulations' error table with the margin K the GPU gate uses, and the refusal of ``--fp16`` on the three command lines."""
import argparse
import os
import subprocess
import sys

import pytest
import torch

import _train_bf16_ref as R
from conftest import REPO

NEW_SYMBOLS = ("r4d_set_train_bf16", "r4d_get_train_bf16", "r4d_conv1d_bf16_keep_f32", "r4d_conv1d_bf16_dgrad_f32",
               "r4d_weight_grad_bf16_workspace_bytes", "r4d_weight_grad_bf16_f32")


def test_symbols_exist_and_the_abi_is_6():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    assert lib.r4d_abi_version() == 6 and _lib.R4D_ABI_VERSION == 6
    hdr = open(os.path.join(REPO, "include", "r4d.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _lib.PROTOTYPES and hasattr(lib, s) and s + "(" in hdr, s
    names = [lib.r4d_dispatch_branch_name(i).decode() for i in range(lib.r4d_dispatch_num_branches())]
    assert {"tuning:train_bf16:fwd", "tuning:train_bf16:dgrad", "tuning:train_bf16:wgrad", "tuning:train_bf16:wgrad_fallback"} <= set(names)
    classes = [lib.r4d_profile_class_name(c).decode() for c in range(lib.r4d_profile_num_classes())]
    assert "gemm_bf16tn_32" in classes and "gemm_bf16_32" in classes


def test_switch_returns_the_previous_value_and_defaults_to_off():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    was = lib.r4d_get_train_bf16()
    try:
        assert was == 0
        assert lib.r4d_set_train_bf16(1) == 0 and lib.r4d_get_train_bf16() == 1
        assert lib.r4d_set_train_bf16(7) == 1 and lib.r4d_get_train_bf16() == 1          # any non-zero value is "on"
        assert lib.r4d_set_train_bf16(0) == 1 and lib.r4d_get_train_bf16() == 0
    finally:
        lib.r4d_set_train_bf16(was)


def test_weight_gradient_size_query_follows_the_shape_contract():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    q = lib.r4d_weight_grad_bf16_workspace_bytes
    assert q(390, 256, 768) > 0 and q(32, 128, 256) > 0
    assert q(4100, 128, 256) > q(390, 128, 256)                         # more slices, more partials
    for rows, i, j in ((390, 64, 256), (390, 128, 192), (31, 128, 256), (0, 128, 256), (390, 0, 256)):
        assert q(rows, i, j) == 0, (rows, i, j)


def test_resolver_and_its_environment_variable(monkeypatch):
    from rag4dyg_amd import training
    monkeypatch.delenv("R4D_TRAIN_PRECISION", raising=False)
    assert training.resolve_train_precision() == "fp32"
    assert training.resolve_train_precision("bf16") == "bf16" and training.resolve_train_precision("fp32") == "fp32"
    monkeypatch.setenv("R4D_TRAIN_PRECISION", "")
    assert training.resolve_train_precision() == "fp32"
    monkeypatch.setenv("R4D_TRAIN_PRECISION", "bf16")
    assert training.resolve_train_precision() == "bf16"
    assert training.resolve_train_precision("fp32") == "fp32"          # an explicit argument wins
    for bad in ("fp16", "BF16", "f32", "half", 1):
        with pytest.raises(ValueError):
            training.resolve_train_precision(bad)
    monkeypatch.setenv("R4D_TRAIN_PRECISION", "fp16")
    with pytest.raises(ValueError):
        training.resolve_train_precision()


def test_fp16_is_still_refused_on_the_three_command_lines():
    from rag4dyg_amd import generator_training, lm_training, training
    args = argparse.Namespace(fp16=True, should_continue=False, fusion="graphpooling", gnn_layers=1, m=1)
    for train in (training.train, lm_training.train, generator_training.train):
        with pytest.raises(NotImplementedError):
            train(args, None, None, None)
        with pytest.raises(NotImplementedError):
            train(args, None, None, None, precision="bf16")          # the project's own mixed precision does not stand in for apex


def test_emulation_patches_conv1d_with_one_flag_per_product():
    from oracle import gpt2_ref
    orig = gpt2_ref.conv1d
    g = torch.Generator().manual_seed(3)
    bf = R.bf16_round
    for (M, K, N), flags in (((40, 128, 256), (True, True, True)), ((40, 64, 256), (True, True, False)),
                             ((31, 128, 256), (True, True, False)), ((40, 128, 192), (True, True, False))):
        assert R.dispatched(M, K, N) == flags
        x = torch.randn(M, K, generator=g, dtype=torch.float64, requires_grad=True)
        w = torch.randn(K, N, generator=g, dtype=torch.float64, requires_grad=True)
        b = torch.randn(N, generator=g, dtype=torch.float64, requires_grad=True)
        dy = torch.randn(M, N, generator=g, dtype=torch.float64)
        with R.patched_conv1d(M):
            y = gpt2_ref.conv1d(x, w, b)
        assert gpt2_ref.conv1d is orig
        y.backward(dy)
        xd, wd = x.detach(), w.detach()
        assert torch.equal(y.detach(), torch.addmm(b.detach(), bf(xd), bf(wd)))
        assert torch.equal(x.grad, bf(dy) @ bf(wd).t())
        assert torch.equal(w.grad, bf(xd).t() @ bf(dy) if flags[2] else xd.t() @ dy)
        assert torch.equal(b.grad, dy.sum(0))                            # the unrounded dy


def test_margin_table():
    """K of the GPU gate, from the two emulations alone: 2 x the largest per-quantity max(e_emu32 / e_emu64, e_emu64 / e_emu32)
    over the gated fixtures (floored at 1e-6), never below 2.  Inside [2, 4]: beyond 4 a fixture leaves the gate and is recorded.
    The arithmetic's own error is the bf16 rounding's, not fp32's: every case has gated gradients of 1e-4 .. 3e-2."""
    print(R.format_table())
    K = R.margin()
    assert 2.0 <= K <= 4.0, K
    assert set(R.GATED) <= set(R.WEIGHTS) and len(R.CASES) == len(R.WEIGHTS) * len(R.KINDS)
    for c in R.CASES:
        t = R.error_table(c)
        gated = [v["emu64"] for n, v in t.items() if v["emu64"] >= R.GATE_FLOOR and n not in ("loss", "emb", "hidden")]
        assert len(gated) >= 2 and max(gated) < 3e-2, (R.case_id(c), gated)     # (the frozen generator step has three gradients)
        assert R.worst_ratio(c)[0] <= 2.0, (R.case_id(c), R.worst_ratio(c))
    # the d 64 fixture's weight gradients all fall back, the d 256 / d 512 ones are all dispatched, g10 (d 128) has both
    d = {w: [R.dispatched(390, K_, N_)[2] for K_, N_ in ((dd, 3 * dd), (dd, dd), (dd, 4 * dd), (4 * dd, dd))]
         for w, dd in (("L2_d64_T40", 64), ("L2_d256_T130", 256), ("L4_d512_T96", 512), ("g10_trained", 128))}
    assert not any(d["L2_d64_T40"]) and all(d["L2_d256_T130"]) and all(d["L4_d512_T96"]) and d["g10_trained"] == [False, False, True, False]


def test_tools_take_the_precision_option():
    from _train_modes import tool_mode_choices
    for tool in ("bench_components.py", "lm_train_bench.py", "gen_train_bench.py", "train_uci13_demo.py"):
        text, words = tool_mode_choices(tool, "--precision")               # from the mode table, or (the demo) spelled out in the tool
        assert "--precision" in text and (words[:2] == ("fp32", "bf16") if words else '"fp32", "bf16"' in text), tool
