"""CPU tests of the opt-in recompute mode of the training attention (``r4d_set_train_attention``): the switch itself, what the
three workspace queries answer in each mode, and how the trainers pick the mode (keyword / ``R4D_TRAIN_ATTENTION``).  Nothing
here touches a GPU; the arithmetic is tested in ``test_gpu_train_attention_recompute.py``."""
import ctypes

import pytest

from rag4dyg_amd import _lib


def _tpad128(T):
    return (T + 127) // 128 * 128


@pytest.fixture()
def lib():
    lib = _lib.load()
    assert lib.r4d_get_train_attention() == 0, "a test before this one left the process in recompute mode"
    yield lib
    assert lib.r4d_set_train_attention(0) == 0


def test_setter_and_getter_round_trip_and_refuse_bad_values(lib):
    assert lib.r4d_get_train_attention() == 0                                  # stored is the default
    assert lib.r4d_set_train_attention(1) == 0 and lib.r4d_get_train_attention() == 1
    assert lib.r4d_set_train_attention(0) == 0 and lib.r4d_get_train_attention() == 0
    for bad in (2, -1, 7):
        assert lib.r4d_set_train_attention(1) == 0
        assert lib.r4d_set_train_attention(bad) != 0
        assert lib.r4d_get_train_attention() == 1                              # a refused value changes nothing
        with pytest.raises(_lib.R4DError):
            _lib.check(lib.r4d_set_train_attention(bad), "set_train_attention")
    assert lib.r4d_set_train_attention(0) == 0
    assert _lib.R4D_ABI_VERSION == lib.r4d_abi_version() == 6                  # new symbols only


def _cfg(L, H, d, V=1000):
    return _lib.GPT2ConfigC(L, H, d, V, 1024, 1e-5)


def _retriever_bytes(lib, cfg, batches):
    n = len(batches)
    Bs = (ctypes.c_int32 * n)(*[b for b, _ in batches])
    Ts = (ctypes.c_int32 * n)(*[t for _, t in batches])
    return int(lib.r4d_gpt2_train_workspace_bytes(ctypes.byref(cfg), n, Bs, Ts))


def _both_modes(lib, query):
    out = []
    for mode in (0, 1):
        assert lib.r4d_set_train_attention(mode) == 0
        out.append(query())
    assert lib.r4d_set_train_attention(0) == 0
    assert out[0] > 0 and out[1] > 0
    return out


CASES = [("tiny", 2, 2, 64, [(2, 7), (3, 33), (2, 129)]),
         ("wikiv2 script", 2, 6, 768, [(128, 512)] * 5),
         ("one layer, one batch", 1, 2, 64, [(3, 200)])]


@pytest.mark.parametrize("name,L,H,d,batches", CASES, ids=[c[0] for c in CASES])
def test_workspace_queries_follow_the_mode(lib, name, L, H, d, batches):
    """stored - recompute == 4 (L Ptot - pmax) bytes for the retriever query over all batches and for the LM / RAG queries over
    each single batch (there Ptot == pmax), up to the 64-float rounding of each block: L kept blocks and 2 + 3 scratch blocks
    can each round, so 256 (L + 4) bytes of slack (every block here is a multiple of 128 floats: the rounding is in fact 0)."""
    from rag4dyg_amd.lm_training import padded_vocab
    cfg = _cfg(L, H, d)
    slack = 256 * (L + 4)
    blocks = [B * H * T * _tpad128(T) for B, T in batches]
    stored, rec = _both_modes(lib, lambda: _retriever_bytes(lib, cfg, batches))
    want = 4 * (L * sum(blocks) - max(blocks))
    print(f"{name}: retriever workspace stored {stored} recompute {rec} bytes, saving {stored - rec} (expected {want})")
    assert abs((stored - rec) - want) <= slack
    ldV = padded_vocab(1000)
    for (B, T), blk in zip(batches, blocks):
        for what, fn in (("lm", lib.r4d_gpt2_lm_train_workspace_bytes), ("rag", lib.r4d_rag_train_workspace_bytes)):
            s1, r1 = _both_modes(lib, lambda: int(fn(ctypes.byref(cfg), B, T, ldV)))
            assert abs((s1 - r1) - 4 * (L - 1) * blk) <= slack, (what, B, T, s1, r1)
    if L == 1 and len(batches) == 1:
        assert abs(stored - rec) <= slack                                      # nothing to save: one P block either way
    if name == "wikiv2 script":
        assert sum(blocks) == 1_006_632_960                                    # 4.0 GB of P per layer in stored mode


def test_trainer_mode_comes_from_the_keyword_or_the_environment(monkeypatch):
    from rag4dyg_amd import training
    monkeypatch.delenv("R4D_TRAIN_ATTENTION", raising=False)
    assert training.resolve_train_attention() == "stored"
    assert training.resolve_train_attention("recompute") == "recompute"
    monkeypatch.setenv("R4D_TRAIN_ATTENTION", "recompute")
    assert training.resolve_train_attention() == "recompute"
    assert training.resolve_train_attention("stored") == "stored"              # the keyword wins
    monkeypatch.setenv("R4D_TRAIN_ATTENTION", "")
    assert training.resolve_train_attention() == "stored"
    for bad in ("flash", "1", "Recompute"):
        with pytest.raises(ValueError):
            training.resolve_train_attention(bad)
        monkeypatch.setenv("R4D_TRAIN_ATTENTION", bad)
        with pytest.raises(ValueError):
            training.resolve_train_attention()
    assert training.TRAIN_ATTENTION_MODES == {"stored": 0, "recompute": 1}
