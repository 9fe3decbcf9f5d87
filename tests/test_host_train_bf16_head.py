"""CPU-side checks of the training steps' opt-in bf16 LM head (``head_precision="bf16"``, ``training.resolve_train_head_precision``,
``r4d_set_train_head_bf16``; the GPU side is tests/test_gpu_train_bf16_head.py): the two names and the environment variable, the
library's third switch beside the two it leaves alone, the new symbols and the unchanged ABI, the head's routes behind the new value
of ``r4d_conv1d_route``'s precision argument, the emulation's head function against float64 autograd, and the emulations' error
tables with the margins K the GPU gates use."""
import argparse
import os

import pytest
import torch

import _train_bf16_head_ref as Hd
import _train_bf16_ref as R
from conftest import REPO

NEW_SYMBOLS = ("r4d_set_train_head_bf16", "r4d_get_train_head_bf16", "r4d_lm_head_train_workspace_bytes", "r4d_lm_head_train_f32")
WT, W3, W3T, H2 = 1, 2, 4, 8


def test_the_two_names_resolve_and_bad_names_raise(monkeypatch):
    from rag4dyg_amd import training
    monkeypatch.delenv("R4D_TRAIN_HEAD_PRECISION", raising=False)
    assert training.resolve_train_head_precision() == "fp32"
    monkeypatch.setenv("R4D_TRAIN_HEAD_PRECISION", "")
    assert training.resolve_train_head_precision() == "fp32"                # empty counts as unset
    for name in ("fp32", "bf16"):
        assert training.resolve_train_head_precision(name) == name
        monkeypatch.setenv("R4D_TRAIN_HEAD_PRECISION", name)
        assert training.resolve_train_head_precision() == name
        assert training.resolve_train_head_precision("fp32") == "fp32"      # an explicit argument wins
    assert training.TRAIN_HEAD_PRECISIONS == {"fp32": 0, "bf16": 1}
    # the head is an axis of its own: the layer / attention table keeps its four names and the resolver of it reads its own variable
    assert training.TRAIN_PRECISIONS == {"fp32": 0, "bf16": 1, "fp32+attn": 0, "bf16+attn": 1}
    assert training.TRAIN_ATTENTION_BF16 == {"fp32": 0, "bf16": 0, "fp32+attn": 1, "bf16+attn": 1}
    monkeypatch.setenv("R4D_TRAIN_HEAD_PRECISION", "bf16")
    monkeypatch.delenv("R4D_TRAIN_PRECISION", raising=False)
    assert training.resolve_train_precision() == "fp32"
    for bad in ("BF16", "fp16", "half", "bf16+attn", "fp32+attn", "bf16 ", 1):
        with pytest.raises(ValueError, match="fp32"):
            training.resolve_train_head_precision(bad)
    monkeypatch.setenv("R4D_TRAIN_HEAD_PRECISION", "fp16")
    with pytest.raises(ValueError, match="bf16"):
        training.resolve_train_head_precision()


def test_switch_round_trips_and_leaves_the_other_two_alone():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    was = (lib.r4d_get_train_head_bf16(), lib.r4d_get_train_bf16(), lib.r4d_get_train_attention_bf16())
    try:
        assert was == (0, 0, 0)                                             # all three default to off
        assert lib.r4d_set_train_head_bf16(1) == 0 and lib.r4d_get_train_head_bf16() == 1
        assert (lib.r4d_get_train_bf16(), lib.r4d_get_train_attention_bf16()) == (0, 0)
        assert lib.r4d_set_train_head_bf16(7) == 1 and lib.r4d_get_train_head_bf16() == 1      # any non-zero value is "on"
        assert lib.r4d_set_train_head_bf16(-1) == 1 and lib.r4d_get_train_head_bf16() == 1
        for setter, getter in ((lib.r4d_set_train_bf16, lib.r4d_get_train_bf16),
                               (lib.r4d_set_train_attention_bf16, lib.r4d_get_train_attention_bf16)):
            assert setter(1) == 0 and getter() == 1 and lib.r4d_get_train_head_bf16() == 1
            assert setter(0) == 1 and getter() == 0 and lib.r4d_get_train_head_bf16() == 1
        assert lib.r4d_set_train_head_bf16(0) == 1 and lib.r4d_get_train_head_bf16() == 0
        assert (lib.r4d_get_train_bf16(), lib.r4d_get_train_attention_bf16()) == (0, 0)
        assert lib.r4d_set_train_bf16(1) == 0 and lib.r4d_set_train_attention_bf16(1) == 0 and lib.r4d_get_train_head_bf16() == 0
    finally:
        lib.r4d_set_train_head_bf16(was[0])
        lib.r4d_set_train_bf16(was[1])
        lib.r4d_set_train_attention_bf16(was[2])


def test_symbols_exist_and_the_abi_is_still_6():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    assert lib.r4d_abi_version() == 6 and _lib.R4D_ABI_VERSION == 6
    hdr = open(os.path.join(REPO, "include", "r4d.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _lib.PROTOTYPES and hasattr(lib, s) and s + "(" in hdr, s
    names = [lib.r4d_dispatch_branch_name(i).decode() for i in range(lib.r4d_dispatch_num_branches())]
    assert {n for n in names if n.startswith("tuning:train_head_bf16:")} == \
        {"tuning:train_head_bf16:" + s for s in ("logits", "dgrad", "wgrad", "wgrad_fallback")}
    # the size query is host arithmetic and does not depend on the switch
    was = lib.r4d_get_train_head_bf16()
    try:
        for N, d, ldV in ((31, 256, 128), (130, 256, 384), (32, 64, 16000), (4096, 768, 50048)):
            lib.r4d_set_train_head_bf16(0)
            off = lib.r4d_lm_head_train_workspace_bytes(N, d, ldV)
            lib.r4d_set_train_head_bf16(1)
            assert lib.r4d_lm_head_train_workspace_bytes(N, d, ldV) == off
            assert off >= 4 * N * min(ldV, Hd.CE_CHUNK)                    # one chunk of logits at the least
        for bad in ((0, 256, 128), (32, 0, 128), (32, 256, 0), (-1, -1, -1)):
            assert lib.r4d_lm_head_train_workspace_bytes(*bad) == 0
    finally:
        lib.r4d_set_train_head_bf16(was)


def test_the_heads_routes_sit_behind_the_new_value_of_the_precision_argument():
    """``r4d_conv1d_route`` with bf16 = 2 asks as the head under its switch: kind 2 the logits, kind 4 dh, kind 5 dwte.  With the
    planes and a supported shape the three take b1 / dgrad_b1 / wgrad_b1tn in EVERY gemm mode; each falls back on its own to what
    bf16 = 0 gives.  The values 0 and 1 keep their answers: kind 4 under 1 (the layers' switch) never takes plain bf16, and the
    planes change no route in exact-f32 mode while the switch is off."""
    from rag4dyg_amd import _lib
    lib = _lib.load()
    was = lib.r4d_get_gemm_split3()

    def route(kind, M, K, N, have, bf16):
        return lib.r4d_conv1d_route_name(lib.r4d_conv1d_route(kind, M, K, N, 0, have, bf16)).decode()
    try:
        for mode in (0, 1, 2):
            lib.r4d_set_gemm_split3(mode)
            off = {0: ("f32_kcopy", "dgrad_f32", "wgrad_f32tn"), 1: ("s3", "dgrad_s3", "wgrad_s3tn"), 2: ("h2", "dgrad_s3", "wgrad_s3tn")}[mode]
            have = WT | W3 | W3T | H2
            for N, d, Ck in ((130, 256, 384), (4096, 768, 15872), (32, 256, 128)):
                assert route(2, N, d, Ck, have, 2) == "b1" and route(4, N, d, Ck, have, 2) == "dgrad_b1"
                assert route(5, N, Ck, d, have, 2) == "wgrad_b1tn"
                assert route(4, N, d, Ck, have, 1) == off[1]               # the layers' switch never moves the head's dh
            N, d, Ck = 4096, 768, 15872
            assert (route(2, N, d, Ck, have, 0), route(4, N, d, Ck, have, 0), route(5, N, Ck, d, have, 0)) == off
            # per-product fallback: no w3 -> the logits alone; no w3t -> dh alone; d % 256, rows < 32 -> dwte alone
            assert route(2, N, d, Ck, WT | W3T | H2, 2) == ("h2" if mode == 2 else "f32_kcopy") and route(4, N, d, Ck, WT | W3T | H2, 2) == "dgrad_b1"
            assert route(4, N, d, Ck, WT | W3 | H2, 2) == "dgrad_f32" and route(2, N, d, Ck, WT | W3 | H2, 2) == "b1"
            assert route(5, 130, 384, 64, have, 2) == route(5, 130, 384, 64, have, 0) != "wgrad_b1tn"
            assert route(5, 31, 128, 256, have, 2) == "wgrad_f32tn" and route(5, 32, 128, 256, have, 2) == "wgrad_b1tn"
            assert route(2, 130, 48, 384, have, 2) == "f32_kcopy"          # d % 32
            # the planes kernels' 2^29 bound on rows x contraction: dh (contraction Ck) leaves first, to the exact-f32 kernel
            assert route(4, 40000, 768, 15872, have, 2) == "dgrad_f32" and route(2, 40000, 768, 15872, have, 2) == "b1"
        lib.r4d_set_gemm_split3(0)
        for have in (0, W3, W3T, W3 | W3T, W3 | W3T | H2):                  # exact f32, switch off: the planes' presence moves nothing
            assert (route(2, 130, 256, 384, WT | have, 0), route(4, 130, 256, 384, WT | have, 0)) == ("f32_kcopy", "dgrad_f32")
        assert lib.r4d_conv1d_route(6, 32, 256, 256, 0, 0, 2) == -1
    finally:
        lib.r4d_set_gemm_split3(was)


def test_dispatched_follows_the_routes():
    """The reference's per-product flags are the library's routes for the same (N, d, V)."""
    from rag4dyg_amd import _lib
    lib = _lib.load()
    for N, d, V in ((31, 256, 100), (32, 256, 100), (130, 256, 300), (130, 64, 300), (32, 256, 15900), (32, 64, 15900), (390, 512, 500)):
        flags = Hd.dispatched(N, d, V)
        for _c0, cn in Hd.chunks(Hd.padded_vocab(V)):
            got = tuple(lib.r4d_conv1d_route_name(lib.r4d_conv1d_route(kind, N, K, Nn, 0, W3 | W3T, 2)).decode() == want
                        for kind, K, Nn, want in ((2, d, cn, "b1"), (4, d, cn, "dgrad_b1"), (5, cn, d, "wgrad_b1tn")))
            assert got == flags, (N, d, V, cn, got, flags)
    assert Hd.dispatched(130, 256, 300, planes=False) == (False, False, True)      # dwte needs no plane
    assert Hd.chunks(16000) == [(0, 15872), (15872, 128)] and Hd.chunks(15872) == [(0, 15872)]


def test_fp16_is_still_refused_whatever_the_head_precision():
    from rag4dyg_amd import generator_training, lm_training
    args = argparse.Namespace(fp16=True, should_continue=False, fusion="graphpooling", gnn_layers=1, m=1)
    for train in (lm_training.train, generator_training.train):
        for hp in ("fp32", "bf16"):
            with pytest.raises(NotImplementedError):
                train(args, None, None, None, precision="bf16+attn", head_precision=hp)


def test_tools_take_the_head_precision():
    import argparse
    from _train_modes import tool_mode_choices
    from rag4dyg_amd import training
    for tool in ("lm_train_bench.py", "gen_train_bench.py"):
        text, words = tool_mode_choices(tool, "--head-precision")
        assert words == ("fp32", "bf16") and "**training.modes_from_args(a)" in text, tool
    assert training.modes_from_args(argparse.Namespace(head_precision="bf16", steps=3)) == {"head_precision": "bf16"}


def test_head_function_agrees_with_float64_autograd_of_the_rounded_operands():
    """With all three flags: logits, dh and dW are the autograd results of bf16(h) . bf16(W)^T taken at the ROUNDED operands under
    the rounded upstream gradient (float64: sums of exactly representable products, equal up to the order of summation); with no
    flag the function is the plain product; each flag moves its own product and no other."""
    g = torch.Generator().manual_seed(13)
    for N, d, V in ((5, 16, 7), (33, 64, 130)):
        h = torch.randn(N, d, generator=g, dtype=torch.float64)
        W = torch.randn(V, d, generator=g, dtype=torch.float64) * 0.05
        dl = torch.randn(N, V, generator=g, dtype=torch.float64) * 1e-3

        def run(flags):
            a, b = h.clone().requires_grad_(True), W.clone().requires_grad_(True)
            out = Hd.head(a, b, flags)
            out.backward(dl)
            return out.detach(), a.grad, b.grad
        ah, bh = R.bf16_round(h).requires_grad_(True), R.bf16_round(W).requires_grad_(True)
        ref = ah @ bh.t()
        ref.backward(R.bf16_round(dl))
        out, dh, dW = run((True, True, True))
        assert torch.equal(out, ref.detach())
        for got, want in ((dh, ah.grad), (dW, bh.grad)):
            assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
        p_out, p_dh, p_dW = run((False, False, False))
        assert torch.equal(p_out, h @ W.t()) and torch.equal(p_dh, dl @ W) and torch.equal(p_dW, dl.t() @ h)
        assert float((out - p_out).abs().max()) > 1e-6 * float(p_out.abs().max())
        for i in range(3):
            flags = tuple(j == i for j in range(3))
            one = run(flags)
            for j, (x, rounded, plain) in enumerate(zip(one, (out, dh, dW), (p_out, p_dh, p_dW))):
                assert torch.equal(x, rounded if j == i else plain), (flags, j)


@pytest.mark.parametrize("mode", Hd.MODES)
def test_margin_tables(mode):
    """K of the GPU gates, from the emulations alone.  The head alone ("fp32"): float64 and float32 of the same step differ by far
    less than the arithmetic's own error (ratios 1.00 .. 1.01), so K sits at its floor of 2 (found 2.00 .. 2.02); asserted inside
    [2, 3].  "bf16+attn" carries the layer and attention emulations with it and lands where their table does (found 2.78; that
    table's own runs gave 2.75 .. 2.95); asserted inside [2, 4] like theirs.  Every case gates at least four quantities, so that
    no gate passes by gating nothing, and the GPU tests' step cases are among them."""
    print(Hd.format_table(mode))
    K = Hd.margin(mode)
    assert 2.0 <= K <= (3.0 if mode == "fp32" else 4.0), K
    assert len(Hd.CASES) == 11 and all(c in R.CASES for c in Hd.CASES)
    ids = {R.case_id(c) for c in Hd.CASES}
    assert {"L2_d256_T130-lm", "g10_trained-lm", "L4_d512_T96-gen_tied", "L2_d256_T130-gen"} <= ids
    for c in Hd.CASES:
        g = Hd.gated(c, mode)
        assert len(g) >= Hd.MIN_GATED, (mode, R.case_id(c), g)
        assert max(g.values()) < 5e-2, (mode, R.case_id(c), g)
        exact = Hd.references(c, mode)[0]
        assert exact["loss"] == R.references(c)[0]["loss"]                  # ONE exact oracle for every gate ...
        for n, v in R.references(c)[0]["grads"].items():
            assert exact["grads"][n] is v, n                                # ... its very arrays, plus d_fused where there is one
        assert ("d_fused" in exact["grads"]) == (c.kind != "lm")
