"""The training modes as ONE table (``rag4dyg_amd.training.TRAIN_MODE_AXES``; the library's is kTrainModes in csrc/train.hip) and what
is derived from it: resolvers, pairing checks, ``TrainModes.select()``, the banner, ``saved_library_modes()``.  CPU only: the built
library, no device.  What a word sets is spelled out HERE a second time (``expected``), so the table is checked against something
that is not the table."""
import ctypes
import itertools
import re

import pytest

import _train_modes
from rag4dyg_amd import _lib, training
from rag4dyg_amd.training import TrainModes

WORDS = dict(attention=("stored", "recompute"), activations=("stored", "recompute"), precision=("fp32", "bf16", "fp32+attn", "bf16+attn"),
             head_precision=("fp32", "bf16"), act_store=("fp32", "bf16"), attention_kernel=("products", "fused"))
ENVS = dict(attention="R4D_TRAIN_ATTENTION", activations="R4D_TRAIN_ACTIVATIONS", precision="R4D_TRAIN_PRECISION",
            head_precision="R4D_TRAIN_HEAD_PRECISION", act_store="R4D_TRAIN_ACT_STORE", attention_kernel="R4D_TRAIN_ATTENTION_KERNEL")
DEFAULTS = dict(attention="stored", activations="stored", precision="fp32", head_precision="fp32", act_store="fp32", attention_kernel="products")
SWITCHES = ("attention", "activations", "bf16", "attention_bf16", "head_bf16", "act_bf16", "attention_fused")
REFUSING = ("attention", "activations", "act_bf16", "attention_fused")        # setters that refuse a value outside 0 / 1 ...
NORMALISING = ("bf16", "attention_bf16", "head_bf16")                          # ... and setters that take it as on != 0
RETURN_PREVIOUS = ("bf16", "attention_bf16", "head_bf16", "act_bf16")          # the others answer R4D_OK

restore = _train_modes.switches_restored()


def expected(attention, activations, precision, head_precision, act_store, attention_kernel):
    return dict(attention=int(attention == "recompute"), activations=int(activations == "recompute"), bf16=int(precision.startswith("bf16")),
                attention_bf16=int(precision.endswith("+attn")), head_bf16=int(head_precision == "bf16"), act_bf16=int(act_store == "bf16"),
                attention_fused=int(attention_kernel == "fused"))


def valid(w):
    return (w["act_store"] == "fp32" or w["precision"].startswith("bf16")) and (w["attention_kernel"] == "products" or w["precision"].endswith("+attn"))


COMBOS = [dict(zip(WORDS, c)) for c in itertools.product(*WORDS.values())]
VALID = [w for w in COMBOS if valid(w)]


@pytest.fixture()
def lib():
    return _lib.load()


def setter(lib, switch):
    return getattr(lib, "r4d_set_train_" + switch)


def clear_env(monkeypatch):
    for env in ENVS.values():
        monkeypatch.delenv(env, raising=False)


def test_every_switch_of_the_binding_belongs_to_exactly_one_axis():
    """An eighth ``r4d_set_train_*`` pair in ``_lib.PROTOTYPES`` without a table row fails here."""
    bound = [m.groups() for m in (re.fullmatch(r"r4d_(set|get)_train_(\w+)", n) for n in _lib.PROTOTYPES) if m]
    assert sorted(s for g, s in bound if g == "set") == sorted(s for g, s in bound if g == "get") == sorted(SWITCHES)
    owners = {s: [a.key for a in training.TRAIN_MODE_AXES if any(s in sets for sets in a.words.values())] for s in SWITCHES}
    assert all(len(o) == 1 for o in owners.values()), owners
    for a in training.TRAIN_MODE_AXES:                                         # every word of an axis sets the same switches, to 0 or 1
        assert len({tuple(sets) for sets in a.words.values()}) == 1 and all(v in (0, 1) for sets in a.words.values() for v in sets.values()), a.key
        assert set(next(iter(a.words.values()))) <= set(SWITCHES), a.key
    assert [a.key for a in training.TRAIN_MODE_AXES] == list(WORDS) and [a.key for a in training.TRAIN_MODE_AXES if a.head] == ["head_precision"]
    assert {a.key: tuple(a.words) for a in training.TRAIN_MODE_AXES} == WORDS
    assert sorted(training.library_modes()) == sorted(SWITCHES)


def test_the_six_word_tables_keep_their_contents():
    assert training.TRAIN_ATTENTION_MODES == {"stored": 0, "recompute": 1} == training.TRAIN_ACTIVATION_MODES
    assert training.TRAIN_PRECISIONS == {"fp32": 0, "bf16": 1, "fp32+attn": 0, "bf16+attn": 1}
    assert training.TRAIN_ATTENTION_BF16 == {"fp32": 0, "bf16": 0, "fp32+attn": 1, "bf16+attn": 1}
    assert training.TRAIN_HEAD_PRECISIONS == {"fp32": 0, "bf16": 1} == training.TRAIN_ACT_STORES
    assert training.TRAIN_ATTENTION_KERNELS == {"products": 0, "fused": 1}


@pytest.mark.parametrize("key", list(WORDS))
def test_argument_then_environment_then_default(monkeypatch, key):
    resolver = getattr(training, "resolve_train_" + key)
    other = next(w for w in WORDS[key] if w != DEFAULTS[key])
    clear_env(monkeypatch)
    assert resolver() == resolver(None) == DEFAULTS[key] and getattr(TrainModes.resolve(), key) == DEFAULTS[key]
    monkeypatch.setenv(ENVS[key], "")                                          # empty counts as unset
    assert resolver() == DEFAULTS[key]
    # (a precision that lets every act_store / attention_kernel word stand, so that only the axis under test decides)
    pairing = {} if key == "precision" else {"precision": "bf16+attn"}
    monkeypatch.setenv(ENVS[key], other)
    assert resolver() == other and getattr(TrainModes.resolve(**pairing), key) == other
    assert resolver(DEFAULTS[key]) == DEFAULTS[key]                            # the argument beats the environment
    assert getattr(TrainModes.resolve(**{**pairing, key: DEFAULTS[key]}), key) == DEFAULTS[key]
    assert getattr(TrainModes.resolve(**{**pairing, key: None}), key) == other  # None is "not given"


@pytest.mark.parametrize("key", list(WORDS))
def test_a_wrong_word_lists_the_sorted_words(monkeypatch, key):
    clear_env(monkeypatch)
    what = {"attention": "train attention mode", "activations": "train activations mode", "precision": "train precision",
            "head_precision": "train head precision", "act_store": "train activation store", "attention_kernel": "train attention kernel"}[key]
    message = re.escape(f"{what} 'fp64': expected one of {sorted(WORDS[key])}")
    with pytest.raises(ValueError, match=message):
        getattr(training, "resolve_train_" + key)("fp64")
    with pytest.raises(ValueError, match=message):
        TrainModes.resolve(**{key: "fp64"})
    monkeypatch.setenv(ENVS[key], "fp64")
    with pytest.raises(ValueError, match=message):
        TrainModes.resolve()


def test_unknown_keywords_and_the_head_word_of_a_headless_step(monkeypatch):
    clear_env(monkeypatch)
    with pytest.raises(TypeError, match="head_dtype"):
        TrainModes.resolve(head_dtype="bf16")
    with pytest.raises(TypeError, match="head_precision"):
        TrainModes.resolve(head=False, head_precision="bf16")
    with pytest.raises(TypeError, match="head_precision"):                     # EncoderTrainer refuses it before it looks at the model
        training.EncoderTrainer(None, head_precision="bf16")
    monkeypatch.setenv("R4D_TRAIN_HEAD_PRECISION", "bf16")                     # ... and a headless value does not read the variable
    m = TrainModes.resolve(head=False)
    assert m.head_precision is None and "head_precision" not in m.record() and "head_bf16" not in m.switches()
    assert TrainModes.resolve(**m.record(), head=False) == m


def test_both_pairing_refusals_keep_their_messages(monkeypatch):
    clear_env(monkeypatch)
    for precision in ("fp32", "fp32+attn"):
        message = re.escape(f"train activation store 'bf16' needs a bf16 layer precision ('bf16' or 'bf16+attn'), not {precision!r}")
        with pytest.raises(ValueError, match=message):
            training.check_act_store("bf16", precision)
        with pytest.raises(ValueError, match=message):
            TrainModes.resolve(precision=precision, act_store="bf16")
    for precision in ("fp32", "bf16"):
        message = re.escape("train attention kernel 'fused' needs a precision with bf16 attention products ('fp32+attn' or 'bf16+attn'), "
                            f"not {precision!r}")
        with pytest.raises(ValueError, match=message):
            training.check_attention_kernel("fused", precision)
        with pytest.raises(ValueError, match=message):
            TrainModes.resolve(precision=precision, attention_kernel="fused")
    assert training.check_act_store("bf16", "bf16+attn") == "bf16" and training.check_attention_kernel("fused", "fp32+attn") == "fused"
    for w in COMBOS:
        if not valid(w):
            with pytest.raises(ValueError):
                TrainModes.resolve(**w)
    # per precision the (act_store, attention_kernel) pairs that stand: fp32 1, bf16 2, fp32+attn 2, bf16+attn 4; times the 8 other words
    assert len(COMBOS) == 128 and len(VALID) == (1 + 2 + 2 + 4) * 8


def test_select_sets_all_seven_switches_for_every_valid_combination(lib):
    for w in VALID:
        for s in SWITCHES:                                                     # the opposite of what is wanted, so that nothing passes by standing still
            setter(lib, s)(1 - expected(**w)[s])
        m = TrainModes.resolve(**w)
        assert m.record() == w and m.switches() == expected(**w)
        m.select()
        assert training.library_modes() == expected(**w), w


@pytest.mark.parametrize("head_was", [0, 1])
def test_a_headless_value_leaves_the_head_switch_alone(lib, head_was):
    for w in VALID:
        enc = {k: v for k, v in w.items() if k != "head_precision"}
        lib.r4d_set_train_head_bf16(head_was)
        TrainModes.resolve(head=False, **enc).select()
        assert training.library_modes() == dict(expected(**w), head_bf16=head_was), w


def test_setters_keep_their_own_conventions(lib):
    for s in REFUSING:
        for keep, bad in itertools.product((1, 0), (2, -1)):
            setter(lib, s)(keep)
            before = training.library_modes()
            assert before[s] == keep
            assert setter(lib, s)(bad) == -1, (s, bad)                         # R4D_ERR_INVALID
            assert training.library_modes() == before, (s, bad)                # a refused value changes nothing
            assert ("set_train_" + s).encode() in lib.r4d_last_error() and str(bad).encode() in lib.r4d_last_error(), (s, bad)
    for s in NORMALISING:
        for bad in (2, -1):
            setter(lib, s)(0)
            assert setter(lib, s)(bad) == 0 and training.library_modes()[s] == 1, (s, bad)       # on != 0; answers the previous value
            assert setter(lib, s)(0) == 1
    for s in SWITCHES:
        setter(lib, s)(0)
        first, second = setter(lib, s)(1), setter(lib, s)(1)
        assert (first, second) == ((0, 1) if s in RETURN_PREVIOUS else (0, 0)), s
        assert training.library_modes()[s] == 1
        setter(lib, s)(0)


def test_saved_library_modes_restores_all_seven_after_an_exception(lib):
    for start in (0, 1):
        for s in SWITCHES:
            setter(lib, s)(start)
        with pytest.raises(KeyError):
            with training.saved_library_modes() as was:
                assert was == dict.fromkeys(SWITCHES, start)
                for s in SWITCHES:
                    setter(lib, s)(1 - start)
                assert training.library_modes() == dict.fromkeys(SWITCHES, 1 - start)
                raise KeyError("the body fails")
        assert training.library_modes() == dict.fromkeys(SWITCHES, start)


def _queries(lib):
    """the three workspace queries at the smallest config: L2 H2 d64, vocab 128, batches (2, 5) and (1, 130)"""
    cfg = _lib.GPT2ConfigC(2, 2, 64, 128, 1024, 1e-5)
    Bs, Ts = (ctypes.c_int32 * 2)(2, 1), (ctypes.c_int32 * 2)(5, 130)
    out = [int(lib.r4d_gpt2_train_workspace_bytes(ctypes.byref(cfg), 2, Bs, Ts))]
    for B, T in ((2, 5), (1, 130)):
        out += [int(lib.r4d_gpt2_lm_train_workspace_bytes(ctypes.byref(cfg), B, T, 128)), int(lib.r4d_rag_train_workspace_bytes(ctypes.byref(cfg), B, T, 128))]
    return out


def test_workspace_queries_under_select_equal_the_setters_called_by_hand(lib):
    seen = set()
    for w in VALID:
        for s, v in expected(**w).items():
            setter(lib, s)(v)
        by_hand = _queries(lib)
        for s in SWITCHES:
            setter(lib, s)(0)
        TrainModes.resolve(**w).select()
        assert _queries(lib) == by_hand and all(b > 0 for b in by_hand), w
        seen.add(tuple(by_hand))
    assert len(seen) > 4                                                       # the modes do move the sizes at this config
    for s in SWITCHES:
        setter(lib, s)(0)
    lib.r4d_set_train_attention_fused(1)                                       # fused without attention-bf16: every query answers 0
    assert _queries(lib) == [0] * 5
    lib.r4d_set_train_bf16(1)                                                  # (the LAYER switch does not stand in for it)
    assert _queries(lib) == [0] * 5
    lib.r4d_set_train_attention_bf16(1)
    assert all(b > 0 for b in _queries(lib))


def test_banner_lines_are_the_text_the_train_functions_printed(monkeypatch):
    """The literals are the ``print`` calls of the three ``train()`` functions before the table (LM and generator: the same five
    lines; the retriever: its own precision line)."""
    clear_env(monkeypatch)
    for w in VALID:
        m = TrainModes.resolve(**w)
        assert m.banner_lines() == [
            "  Attention probabilities = {} (R4D_TRAIN_ATTENTION)".format(w["attention"]),
            "  Layer activations = {} (R4D_TRAIN_ACTIVATIONS)".format(w["activations"]),
            "  Layer GEMM precision = {} (R4D_TRAIN_PRECISION; '+attn': the attention products on bf16 too), LM head precision = {} "
            "(R4D_TRAIN_HEAD_PRECISION)".format(w["precision"], w["head_precision"]),
            "  Saved activations of the bf16 layer GEMMs = {} (R4D_TRAIN_ACT_STORE)".format(w["act_store"]),
            "  Attention kernels = {} (R4D_TRAIN_ATTENTION_KERNEL; 'fused': no T x T block, needs a '+attn' precision)".format(w["attention_kernel"])]
        enc = TrainModes.resolve(head=False, **{k: v for k, v in w.items() if k != "head_precision"})
        assert enc.banner_lines() == [
            "  Attention probabilities = {} (R4D_TRAIN_ATTENTION)".format(w["attention"]),
            "  Layer activations = {} (R4D_TRAIN_ACTIVATIONS)".format(w["activations"]),
            "  Layer GEMM precision = {} (R4D_TRAIN_PRECISION; '+attn': the attention products on bf16 too); "
            "no LM head in this step (R4D_TRAIN_HEAD_PRECISION is not read)".format(w["precision"]),
            "  Saved activations of the bf16 layer GEMMs = {} (R4D_TRAIN_ACT_STORE)".format(w["act_store"]),
            "  Attention kernels = {} (R4D_TRAIN_ATTENTION_KERNEL; 'fused': no T x T block, needs a '+attn' precision)".format(w["attention_kernel"])]
