"""CPU-side checks of the training steps' opt-in bf16 attention products (the ``+attn`` precisions of
``training.resolve_train_precision``; the GPU side is tests/test_gpu_train_bf16_attn.py): the four precision names and the
environment variable, the library's new switch beside the untouched ``r4d_set_train_bf16``, its new symbols and unchanged ABI, the
two emulations' error tables with the margins K the GPU gates use, and the emulation's product function against float64 autograd."""
import argparse
import os

import pytest
import torch

import _train_bf16_attn_ref as A
import _train_bf16_ref as R
from conftest import REPO

NEW_SYMBOLS = ("r4d_set_train_attention_bf16", "r4d_get_train_attention_bf16", "r4d_train_attn_probs_ld",
               "r4d_train_attn_product_bf16_f32")


def test_the_four_names_resolve_and_bad_names_raise(monkeypatch):
    from rag4dyg_amd import training
    monkeypatch.delenv("R4D_TRAIN_PRECISION", raising=False)
    assert training.resolve_train_precision() == "fp32"
    for name in ("fp32", "bf16", "fp32+attn", "bf16+attn"):
        assert training.resolve_train_precision(name) == name
        monkeypatch.setenv("R4D_TRAIN_PRECISION", name)
        assert training.resolve_train_precision() == name
        assert training.resolve_train_precision("fp32") == "fp32"          # an explicit argument wins
    # two independent axes: the layer GEMMs (and with them the plane bookkeeping) and the attention products
    assert training.TRAIN_PRECISIONS == {"fp32": 0, "bf16": 1, "fp32+attn": 0, "bf16+attn": 1}
    assert training.TRAIN_ATTENTION_BF16 == {"fp32": 0, "bf16": 0, "fp32+attn": 1, "bf16+attn": 1}
    for bad in ("BF16", "fp16", "half", "attn", "bf16+", "+attn", "bf16+ATTN", "bf16 + attn", 1):
        with pytest.raises(ValueError):
            training.resolve_train_precision(bad)
    monkeypatch.setenv("R4D_TRAIN_PRECISION", "fp16+attn")
    with pytest.raises(ValueError):
        training.resolve_train_precision()


def test_switch_round_trips_and_leaves_train_bf16_alone():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    was = (lib.r4d_get_train_attention_bf16(), lib.r4d_get_train_bf16())
    try:
        assert was == (0, 0)                                                # both default to off
        assert lib.r4d_set_train_attention_bf16(1) == 0 and lib.r4d_get_train_attention_bf16() == 1
        assert lib.r4d_get_train_bf16() == 0
        assert lib.r4d_set_train_attention_bf16(7) == 1 and lib.r4d_get_train_attention_bf16() == 1      # any non-zero value is "on"
        assert lib.r4d_set_train_bf16(1) == 0 and lib.r4d_get_train_bf16() == 1 and lib.r4d_get_train_attention_bf16() == 1
        assert lib.r4d_set_train_attention_bf16(0) == 1 and lib.r4d_get_train_attention_bf16() == 0
        assert lib.r4d_get_train_bf16() == 1
        assert lib.r4d_set_train_bf16(0) == 1 and lib.r4d_get_train_attention_bf16() == 0
    finally:
        lib.r4d_set_train_attention_bf16(was[0])
        lib.r4d_set_train_bf16(was[1])


def test_symbols_exist_and_the_abi_is_still_6():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    assert lib.r4d_abi_version() == 6 and _lib.R4D_ABI_VERSION == 6
    hdr = open(os.path.join(REPO, "include", "r4d.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _lib.PROTOTYPES and hasattr(lib, s) and s + "(" in hdr, s
    names = [lib.r4d_dispatch_branch_name(i).decode() for i in range(lib.r4d_dispatch_num_branches())]
    assert {n for n in names if n.startswith("tuning:train_bf16_attn:")} == {"tuning:train_bf16_attn:nt", "tuning:train_bf16_attn:nn"}
    # the layer axis' own prefix keeps exactly its four names
    assert {n for n in names if n.startswith("tuning:train_bf16:")} == {"tuning:train_bf16:" + s for s in ("fwd", "dgrad", "wgrad", "wgrad_fallback")}
    classes = [lib.r4d_profile_class_name(c).decode() for c in range(lib.r4d_profile_num_classes())]
    assert "gemm_bf16h_nt" in classes and "gemm_bf16h_nn" in classes
    for T, ld in ((1, 128), (128, 128), (129, 256), (340, 384), (1024, 1024), (0, 0), (-3, 0)):
        assert lib.r4d_train_attn_probs_ld(T) == ld, T


def test_fp16_is_still_refused_whatever_the_precision():
    from rag4dyg_amd import generator_training, lm_training, training
    args = argparse.Namespace(fp16=True, should_continue=False, fusion="graphpooling", gnn_layers=1, m=1)
    for train in (training.train, lm_training.train, generator_training.train):
        for precision in ("fp32+attn", "bf16+attn"):
            with pytest.raises(NotImplementedError):
                train(args, None, None, None, precision=precision)


def test_tools_take_the_new_names():
    from _train_modes import tool_mode_choices
    for tool in ("bench_components.py", "lm_train_bench.py", "gen_train_bench.py"):
        assert tool_mode_choices(tool, "--precision")[1] == ("fp32", "bf16", "fp32+attn", "bf16+attn"), tool


def test_emulation_patches_attn_core_and_restores_it():
    from oracle import gpt2_ref
    orig_core, orig_conv = gpt2_ref.attn_core, gpt2_ref.conv1d
    with A.patched("fp32+attn", 40):
        assert gpt2_ref.attn_core is A.attn_core_bf16 and gpt2_ref.conv1d is orig_conv
    with A.patched("bf16+attn", 40):
        assert gpt2_ref.attn_core is A.attn_core_bf16 and gpt2_ref.conv1d is not orig_conv
    assert gpt2_ref.attn_core is orig_core and gpt2_ref.conv1d is orig_conv
    # on operands that ARE bf16 numbers the patched function is the original one (float64: the products are then exact sums)
    g = torch.Generator().manual_seed(5)
    q, k, v = (R.bf16_round(torch.randn(2, 3, 9, 16, generator=g, dtype=torch.float64)) for _ in range(3))
    kt = k.transpose(-1, -2)
    assert torch.equal(A.product(q, kt), torch.matmul(q, kt))
    # the whole function: only P (never a bf16 number) is rounded, by at most 2^-9 relative per element
    out, ref = A.attn_core_bf16(q, kt, v), orig_core(q, kt, v)
    assert out.shape == ref.shape and 0.0 < float((out - ref).abs().max()) <= 2.0 ** -9 * float(v.abs().max())


def test_product_backward_agrees_with_float64_autograd_of_the_rounded_operands():
    """da = bf16(dc) . bf16(b)^T and db = bf16(a)^T . bf16(dc) are the autograd gradients of bf16(a) . bf16(b) taken at the ROUNDED
    operands under the rounded upstream gradient -- in float64 both are sums of exactly representable products, so they agree to
    the last bit up to the order of summation (1e-12 relative)."""
    g = torch.Generator().manual_seed(11)
    for shape_a, shape_b in (((5, 16), (16, 7)), ((2, 3, 33, 48), (2, 3, 48, 33)), ((1, 2, 17, 17), (1, 2, 17, 64))):
        a = torch.randn(*shape_a, generator=g, dtype=torch.float64, requires_grad=True)
        b = torch.randn(*shape_b, generator=g, dtype=torch.float64, requires_grad=True)
        dc = torch.randn(*shape_a[:-1], shape_b[-1], generator=g, dtype=torch.float64) * 1e-3
        c = A.product(a, b)
        c.backward(dc)
        ah = R.bf16_round(a.detach()).requires_grad_(True)
        bh = R.bf16_round(b.detach()).requires_grad_(True)
        ch = torch.matmul(ah, bh)
        ch.backward(R.bf16_round(dc))
        assert torch.equal(c.detach(), ch.detach())
        for got, want in ((a.grad, ah.grad), (b.grad, bh.grad)):
            assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
        # and they are NOT the gradients of the unrounded product
        a2 = a.detach().clone().requires_grad_(True)
        torch.matmul(a2, b.detach()).backward(dc)
        assert float((a.grad - a2.grad).abs().max()) > 1e-6 * float(a2.grad.abs().max())


@pytest.mark.parametrize("mode", A.MODES)
def test_margin_tables(mode):
    """K of the GPU gates, from the two emulations alone (as tests/test_host_train_bf16.py::test_margin_table): inside [2, 4], and
    every one of the sixteen cases gates at least four quantities, so that no gate passes by gating nothing."""
    print(A.format_table(mode))
    K = A.margin(mode)
    assert 2.0 <= K <= 4.0, K
    assert len(R.CASES) == 16
    for c in R.CASES:
        g = A.gated(c, mode)
        assert len(g) >= A.MIN_GATED, (mode, R.case_id(c), g)
        assert max(g.values()) < 5e-2, (mode, R.case_id(c), g)
        assert A.references(c, mode)[0] is R.references(c)[0]               # ONE exact oracle for every gate
