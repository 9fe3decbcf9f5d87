"""CPU tests of the opt-in recompute mode of the training activations (``r4d_set_train_activations``): the switch itself and its
independence of ``r4d_set_train_attention``, what the three workspace queries answer in the four mode combinations, and how the
trainers pick the mode (keyword / ``R4D_TRAIN_ACTIVATIONS``).  Nothing here touches a GPU; the arithmetic is tested in
``test_gpu_train_activation_recompute.py``."""
import ctypes

import pytest

from rag4dyg_amd import _lib


def _tpad128(T):
    return (T + 127) // 128 * 128


@pytest.fixture()
def lib():
    lib = _lib.load()
    assert lib.r4d_get_train_attention() == 0, "a test before this one left the process in attention recompute mode"
    assert lib.r4d_get_train_activations() == 0, "a test before this one left the process in activations recompute mode"
    yield lib
    assert lib.r4d_set_train_attention(0) == 0
    assert lib.r4d_set_train_activations(0) == 0


def test_setter_and_getter_round_trip_and_refuse_bad_values(lib):
    assert lib.r4d_get_train_activations() == 0                                # stored is the default
    assert lib.r4d_set_train_activations(1) == 0 and lib.r4d_get_train_activations() == 1
    assert lib.r4d_set_train_activations(0) == 0 and lib.r4d_get_train_activations() == 0
    for bad in (2, -1, 7):
        for keep in (1, 0):
            assert lib.r4d_set_train_activations(keep) == 0
            assert lib.r4d_set_train_activations(bad) != 0
            assert lib.r4d_get_train_activations() == keep                     # a refused value changes nothing
            with pytest.raises(_lib.R4DError):
                _lib.check(lib.r4d_set_train_activations(bad), "set_train_activations")
    assert _lib.R4D_ABI_VERSION == lib.r4d_abi_version() == 6                  # new symbols only


def test_the_two_switches_are_independent(lib):
    for att in (0, 1):
        for act in (0, 1):
            assert lib.r4d_set_train_attention(att) == 0                       # either order of setting
            assert lib.r4d_set_train_activations(act) == 0
            assert (lib.r4d_get_train_attention(), lib.r4d_get_train_activations()) == (att, act)
            assert lib.r4d_set_train_attention(1 - att) == 0
            assert (lib.r4d_get_train_attention(), lib.r4d_get_train_activations()) == (1 - att, act)
            assert lib.r4d_set_train_activations(1 - act) == 0
            assert (lib.r4d_get_train_attention(), lib.r4d_get_train_activations()) == (1 - att, 1 - act)
            assert lib.r4d_set_train_attention(2) != 0 and lib.r4d_set_train_activations(2) != 0
            assert (lib.r4d_get_train_attention(), lib.r4d_get_train_activations()) == (1 - att, 1 - act)


def _cfg(L, H, d, V=1000):
    return _lib.GPT2ConfigC(L, H, d, V, 1024, 1e-5)


def _retriever_bytes(lib, cfg, batches):
    n = len(batches)
    Bs = (ctypes.c_int32 * n)(*[b for b, _ in batches])
    Ts = (ctypes.c_int32 * n)(*[t for _, t in batches])
    return int(lib.r4d_gpt2_train_workspace_bytes(ctypes.byref(cfg), n, Bs, Ts))


def _four_modes(lib, query):
    """{(attention, activations): bytes}"""
    out = {}
    for att in (0, 1):
        for act in (0, 1):
            assert lib.r4d_set_train_attention(att) == 0 and lib.r4d_set_train_activations(act) == 0
            out[(att, act)] = query()
    assert lib.r4d_set_train_attention(0) == 0 and lib.r4d_set_train_activations(0) == 0
    assert all(v > 0 for v in out.values())
    return out


CASES = [("tiny", 3, 2, 64, [(2, 7), (3, 33), (2, 129)]),
         ("wikiv2 script", 2, 6, 768, [(128, 512)] * 5),
         ("hepth script", 12, 2, 256, [(128, 1024)] * 5),
         ("one layer, one batch", 1, 2, 64, [(3, 200)])]

# What the three queries answered in stored / stored mode before the activations switch existed (retriever over all batches; LM
# and RAG over the first batch, ldV = padded_vocab(1000)): mode 0 must not move by a byte.
STORED_BYTES = {"tiny": (9_172_736, 1_120_768, 1_120_768),
                "wikiv2 script": (52_099_400_192, 12_527_452_928, 12_527_452_928),
                "hepth script": (202_247_193_088, 43_100_095_232, 43_100_095_232),
                "one layer, one batch": (8_437_504, 12_253_696, 12_253_696)}


def _check_saving(name, what, L, d, M, Ptot, by_mode):
    """stored - recompute >= 4 [(15 (L - 1) - 1) M d + p (L - 1) Ptot] - slack for L >= 2 (p = 1 under stored attention: L - 1 of
    the L P blocks go; the -1: layer 0 may keep a ln1 block of its own); the two totals agree within slack for L == 1.  slack: 256
    bytes (64 floats of rounding) for each block of the stored layout, 9 per layer and 12 behind them."""
    slack = 256 * (9 * L + 12)
    for att in (0, 1):
        stored, rec = by_mode[(att, 0)], by_mode[(att, 1)]
        p = 1 - att
        want = 4 * ((15 * (L - 1) - 1) * M * d + p * (L - 1) * Ptot)
        print(f"{name} / {what} / attention {att}: stored {stored} recompute {rec} bytes, saving {stored - rec} (at least {want})")
        if L == 1:
            assert abs(stored - rec) <= slack
        else:
            assert stored - rec >= want - slack
            assert stored - rec <= want + 4 * M * d + slack                    # and nothing else went missing from the layout
        assert rec > 4 * (L + 15) * M * d                                      # x_in per layer and one shared set are there


@pytest.mark.parametrize("name,L,H,d,batches", CASES, ids=[c[0] for c in CASES])
def test_workspace_queries_follow_both_modes(lib, name, L, H, d, batches):
    from rag4dyg_amd.lm_training import padded_vocab
    cfg = _cfg(L, H, d)
    blocks = [B * H * T * _tpad128(T) for B, T in batches]
    M = sum(B * T for B, T in batches)
    got = _four_modes(lib, lambda: _retriever_bytes(lib, cfg, batches))
    _check_saving(name, "retriever", L, d, M, sum(blocks), got)
    pinned = [got[(0, 0)]]
    ldV = padded_vocab(1000)
    for i, ((B, T), blk) in enumerate(zip(batches, blocks)):
        if i and (B, T) == batches[0]:
            continue                                                            # the script shapes repeat one batch five times
        for what, fn in (("lm", lib.r4d_gpt2_lm_train_workspace_bytes), ("rag", lib.r4d_rag_train_workspace_bytes)):
            one = _four_modes(lib, lambda: int(fn(ctypes.byref(cfg), B, T, ldV)))
            _check_saving(name, f"{what} ({B}, {T})", L, d, B * T, blk, one)
            if i == 0:
                pinned.append(one[(0, 0)])
    assert tuple(pinned) == STORED_BYTES[name]                                 # stored mode: what the queries always answered
    if name == "wikiv2 script":                                                # the identity the attention test pins, unchanged
        assert abs((got[(0, 0)] - got[(1, 0)]) - 4 * (L * sum(blocks) - max(blocks))) <= 256 * (L + 4)


def test_trainer_mode_comes_from_the_keyword_or_the_environment(monkeypatch):
    from rag4dyg_amd import training
    monkeypatch.delenv("R4D_TRAIN_ACTIVATIONS", raising=False)
    assert training.resolve_train_activations() == "stored"
    assert training.resolve_train_activations("recompute") == "recompute"
    monkeypatch.setenv("R4D_TRAIN_ACTIVATIONS", "recompute")
    assert training.resolve_train_activations() == "recompute"
    assert training.resolve_train_activations("stored") == "stored"            # the keyword wins
    monkeypatch.setenv("R4D_TRAIN_ATTENTION", "stored")                        # the attention variable does not reach it
    assert training.resolve_train_activations() == "recompute"
    monkeypatch.setenv("R4D_TRAIN_ACTIVATIONS", "")
    assert training.resolve_train_activations() == "stored"
    for bad in ("checkpoint", "1", "Recompute"):
        with pytest.raises(ValueError):
            training.resolve_train_activations(bad)
        monkeypatch.setenv("R4D_TRAIN_ACTIVATIONS", bad)
        with pytest.raises(ValueError):
            training.resolve_train_activations()
    assert training.TRAIN_ACTIVATION_MODES == {"stored": 0, "recompute": 1}


def test_trainers_and_train_loops_take_the_keyword():
    from _train_modes import takes_mode_keyword
    from rag4dyg_amd import generator_training, lm_training, training
    for fn in (training.EncoderTrainer.__init__, lm_training.LMTrainer.__init__, generator_training.GeneratorTrainer.__init__,
               training.train, lm_training.train, generator_training.train):
        assert takes_mode_keyword(fn, "activations"), fn                        # (named, default None -- or an axis behind **modes)
