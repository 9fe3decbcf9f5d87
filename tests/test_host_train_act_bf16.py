"""The bf16 activation store of the bf16 training steps on the host side (``act_store="bf16"``, ``R4D_TRAIN_ACT_STORE``,
``r4d_set_train_act_bf16``): the switch, the resolver and its pairing with ``precision``, the three workspace queries -- the
saving is exact and derivable -- and the refusal of ``--fp16`` whatever the store.  The library's host functions
load without a GPU.

Bytes saved with both switches on, M rows in the step, where d % 256 == 0 and M >= 32:
    activations stored      (12 L - 2) M d      f: 8 M d, ln2: 2 M d per layer; ln1: 2 M d per layer behind the first
    activations recompute   10 M d (+ 2 M d when L >= 2)      one shared f, ln2 and (layers >= 1) ln1
and nothing anywhere else (d 64, M < 32, the layer switch off)."""
import argparse
import ctypes
import itertools

import pytest

SHAPES = [(2, 256, [(3, 130)]), (4, 512, [(2, 40), (3, 17), (1, 130)]), (1, 256, [(1, 32)]), (2, 64, [(3, 40)])]
NOTHING = [(1, 256, [(1, 31)]), (2, 64, [(3, 40)])]                        # M = 31; d = 64


@pytest.fixture()
def lib():
    from rag4dyg_amd import _lib, training
    with training.saved_library_modes():
        yield _lib.load()


def expected_saving(L, d, M, act_recompute):
    if d % 256 or M < 32:
        return 0
    return (10 + (2 if L >= 2 else 0)) * M * d if act_recompute else (12 * L - 2) * M * d


def sizes(lib, L, d, groups, V=200):
    """(retriever, LM, RAG) workspace bytes of a shape under the current switches; the LM and RAG steps are one batch: the first group"""
    from rag4dyg_amd import _lib
    H = d // 64
    n_pos = max(T for _B, T in groups) + 8
    cfg = _lib.GPT2ConfigC(L, H, d, V, n_pos, 1e-5)
    Bs = (ctypes.c_int32 * len(groups))(*[B for B, _T in groups])
    Ts = (ctypes.c_int32 * len(groups))(*[T for _B, T in groups])
    B0, T0 = groups[0]
    enc = lib.r4d_gpt2_train_workspace_bytes(ctypes.byref(cfg), len(groups), Bs, Ts)
    ldV = (V + 255) // 256 * 256                                           # a padded head width (the queries take it as given)
    lm = lib.r4d_gpt2_lm_train_workspace_bytes(ctypes.byref(cfg), B0, T0, ldV)
    rag = lib.r4d_rag_train_workspace_bytes(ctypes.byref(cfg), B0, T0, ldV)
    assert enc > 0 and lm > 0 and rag > 0
    return enc, lm, rag


def test_switch_defaults_to_off_returns_the_previous_value_and_refuses_other_values(lib):
    assert lib.r4d_abi_version() == 6
    lib.r4d_set_train_act_bf16(0)
    assert lib.r4d_get_train_act_bf16() == 0
    assert lib.r4d_set_train_act_bf16(1) == 0 and lib.r4d_get_train_act_bf16() == 1
    assert lib.r4d_set_train_act_bf16(1) == 1
    for bad in (2, -1, 7):
        assert lib.r4d_set_train_act_bf16(bad) == -1                       # R4D_ERR_INVALID
        assert lib.r4d_get_train_act_bf16() == 1                           # ... and nothing changed
        assert b"set_train_act_bf16" in lib.r4d_last_error()
    assert lib.r4d_set_train_act_bf16(0) == 1 and lib.r4d_get_train_act_bf16() == 0
    assert lib.r4d_get_train_bf16() in (0, 1)                              # the other switches have their own state
    before = lib.r4d_get_train_bf16()
    lib.r4d_set_train_act_bf16(1)
    assert lib.r4d_get_train_bf16() == before


def test_default_in_a_fresh_process_is_off():
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", "from rag4dyg_amd import _lib; print(_lib.load().r4d_get_train_act_bf16())"],
                         cwd=repo, capture_output=True, text=True, check=True)
    assert out.stdout.strip() == "0"


def test_resolver_its_environment_variable_and_the_pairing_with_precision(monkeypatch):
    from rag4dyg_amd import training
    monkeypatch.delenv("R4D_TRAIN_ACT_STORE", raising=False)
    assert training.resolve_train_act_store() == "fp32"
    monkeypatch.setenv("R4D_TRAIN_ACT_STORE", "")
    assert training.resolve_train_act_store() == "fp32"
    monkeypatch.setenv("R4D_TRAIN_ACT_STORE", "bf16")
    assert training.resolve_train_act_store() == "bf16"
    assert training.resolve_train_act_store("fp32") == "fp32"              # the argument wins over the environment
    monkeypatch.setenv("R4D_TRAIN_ACT_STORE", "fp32")
    assert training.resolve_train_act_store("bf16") == "bf16"
    for bad in ("fp16", "BF16", "half", "bf16+attn", 1):
        with pytest.raises(ValueError):
            training.resolve_train_act_store(bad)
    monkeypatch.setenv("R4D_TRAIN_ACT_STORE", "fp16")
    with pytest.raises(ValueError):
        training.resolve_train_act_store()
    for precision in ("fp32", "fp32+attn"):
        with pytest.raises(ValueError, match="bf16 layer precision"):
            training.check_act_store("bf16", precision)
        assert training.check_act_store("fp32", precision) == "fp32"
    for precision in ("bf16", "bf16+attn"):
        assert training.check_act_store("bf16", precision) == "bf16"


def test_a_trainer_refuses_the_bf16_store_under_an_fp32_layer_precision(monkeypatch):
    """The pairing is checked at construction, before anything touches the model or the GPU."""
    from rag4dyg_amd import training
    from rag4dyg_amd.generator_training import GeneratorTrainer
    from rag4dyg_amd.lm_training import LMTrainer

    class Model:                                                           # never looked at: the resolvers come first
        lm_head = None
    monkeypatch.delenv("R4D_TRAIN_ACT_STORE", raising=False)
    for precision in ("fp32", "fp32+attn"):
        with pytest.raises(ValueError, match="bf16 layer precision"):
            training.EncoderTrainer(Model(), precision=precision, act_store="bf16")
    monkeypatch.setenv("R4D_TRAIN_ACT_STORE", "bf16")
    with pytest.raises(ValueError, match="bf16 layer precision"):
        training.EncoderTrainer(Model(), precision="fp32")
    from _train_modes import takes_mode_keyword
    for cls in (training.EncoderTrainer, LMTrainer, GeneratorTrainer):
        assert takes_mode_keyword(cls.__init__, "act_store"), cls
    for fn in (training.train, __import__("rag4dyg_amd.lm_training", fromlist=["train"]).train,
               __import__("rag4dyg_amd.generator_training", fromlist=["train"]).train):
        assert takes_mode_keyword(fn, "act_store"), fn


@pytest.mark.parametrize("L,d,groups", SHAPES + [NOTHING[0]], ids=lambda v: str(v).replace(" ", ""))
def test_workspace_queries_shrink_by_exactly_the_formula(lib, L, d, groups):
    M_all = sum(B * T for B, T in groups)
    M_one = groups[0][0] * groups[0][1]
    for attention, activations in itertools.product((0, 1), (0, 1)):
        assert lib.r4d_set_train_attention(attention) == 0 and lib.r4d_set_train_activations(activations) == 0
        lib.r4d_set_train_bf16(1)
        lib.r4d_set_train_act_bf16(0)
        off = sizes(lib, L, d, groups)
        lib.r4d_set_train_act_bf16(1)
        on = sizes(lib, L, d, groups)
        want = (expected_saving(L, d, M_all, activations), expected_saving(L, d, M_one, activations), expected_saving(L, d, M_one, activations))
        got = tuple(a - b for a, b in zip(off, on))
        print(f"[train_act_bf16] L{L} d{d} {groups} attention={attention} activations={activations}: bytes off {off} on {on} saved {got}")
        assert got == want, (attention, activations, got, want)
        if d == 64 or M_all < 32:
            assert got == (0, 0, 0)
        # the layer switch off: the store switch changes no byte, and the sizes are the fp32 step's
        lib.r4d_set_train_bf16(0)
        with_store = sizes(lib, L, d, groups)
        lib.r4d_set_train_act_bf16(0)
        assert sizes(lib, L, d, groups) == with_store
        lib.r4d_set_train_bf16(1)
        assert sizes(lib, L, d, groups) == off                              # (the layer switch alone never changed a size)
        assert with_store == off


def test_nothing_is_saved_at_d64_or_below_32_rows(lib):
    lib.r4d_set_train_bf16(1)
    for L, d, groups in NOTHING:
        for activations in (0, 1):
            lib.r4d_set_train_activations(activations)
            lib.r4d_set_train_act_bf16(0)
            off = sizes(lib, L, d, groups)
            lib.r4d_set_train_act_bf16(1)
            assert sizes(lib, L, d, groups) == off, (L, d, groups, activations)


def test_fp16_is_still_refused_on_the_three_command_lines_whatever_the_store(monkeypatch):
    from rag4dyg_amd import generator_training, lm_training, training
    args = argparse.Namespace(fp16=True, should_continue=False, fusion="graphpooling", gnn_layers=1, m=1)
    for store in (None, "fp32", "bf16"):
        for env in (None, "bf16"):
            if env is None:
                monkeypatch.delenv("R4D_TRAIN_ACT_STORE", raising=False)
            else:
                monkeypatch.setenv("R4D_TRAIN_ACT_STORE", env)
            for train in (training.train, lm_training.train, generator_training.train):
                with pytest.raises(NotImplementedError):
                    train(args, None, None, None, precision="bf16", act_store=store)
