"""CPU tests of the opt-in fused training attention (``r4d_set_train_attention_fused``, ``attention_kernel="fused"``): the switch
itself, what the three workspace queries answer with it, and how the trainers pick it (keyword / ``R4D_TRAIN_ATTENTION_KERNEL``)
and pair it with the precision.  Nothing here touches a GPU; the kernels are tested in ``test_gpu_train_attention_fused.py``."""
import argparse
import ctypes
import os

import pytest

from conftest import REPO
from rag4dyg_amd import _lib
from test_host_train_attention_recompute import CASES, _cfg, _retriever_bytes

NEW_SYMBOLS = ("r4d_set_train_attention_fused", "r4d_get_train_attention_fused", "r4d_train_attn_fused_fwd_f32",
               "r4d_train_attn_fused_bwd_workspace_bytes", "r4d_train_attn_fused_bwd_f32")


@pytest.fixture()
def lib():
    """the library with every training switch as the test found it afterwards"""
    from rag4dyg_amd import training
    lib = _lib.load()
    with training.saved_library_modes() as was:
        assert was["attention_fused"] == 0, "a test before this one left the fused switch on"
        yield lib
    assert lib.r4d_get_train_attention_fused() == 0


def test_switch_round_trips_refuses_other_values_and_the_abi_is_still_6(lib):
    assert lib.r4d_get_train_attention_fused() == 0                            # off is the default
    assert lib.r4d_set_train_attention_fused(1) == 0 and lib.r4d_get_train_attention_fused() == 1
    for bad in (2, -1, 7):
        assert lib.r4d_set_train_attention_fused(bad) != 0
        assert lib.r4d_get_train_attention_fused() == 1                        # a refused value changes nothing
        with pytest.raises(_lib.R4DError):
            _lib.check(lib.r4d_set_train_attention_fused(bad), "set_train_attention_fused")
    assert lib.r4d_set_train_attention_fused(0) == 0 and lib.r4d_get_train_attention_fused() == 0
    # the other switches did not move, and the stored / recompute setter still knows two modes
    assert lib.r4d_get_train_attention_bf16() == 0 and lib.r4d_get_train_attention() == 0
    assert lib.r4d_set_train_attention(2) != 0 and lib.r4d_get_train_attention() == 0
    assert lib.r4d_abi_version() == 6 and _lib.R4D_ABI_VERSION == 6
    hdr = open(os.path.join(REPO, "include", "r4d.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _lib.PROTOTYPES and hasattr(lib, s) and s + "(" in hdr, s
    names = [lib.r4d_dispatch_branch_name(i).decode() for i in range(lib.r4d_dispatch_num_branches())]
    assert {n for n in names if n.startswith("tuning:train_attn_fused:")} == {"tuning:train_attn_fused:" + s for s in ("fwd", "rowsum", "dkv", "dq")}
    assert {n for n in names if n.startswith("tuning:train_bf16_attn:")} == {"tuning:train_bf16_attn:nt", "tuning:train_bf16_attn:nn"}


def _queries(lib, cfg, batches, ldV):
    """name -> bytes of the retriever query over all batches and the LM / RAG queries over each single batch"""
    out = {"retriever": _retriever_bytes(lib, cfg, batches)}
    for i, (B, T) in enumerate(batches):
        out[f"lm{i}"] = int(lib.r4d_gpt2_lm_train_workspace_bytes(ctypes.byref(cfg), B, T, ldV))
        out[f"rag{i}"] = int(lib.r4d_rag_train_workspace_bytes(ctypes.byref(cfg), B, T, ldV))
    return out


@pytest.mark.parametrize("activations", (0, 1), ids=("activations stored", "activations recompute"))
@pytest.mark.parametrize("name,L,H,d,batches", CASES, ids=[c[0] for c in CASES])
def test_workspace_queries_follow_the_switch(lib, name, L, H, d, batches, activations):
    """recompute - fused == 4 (3 pmax - (L' + 1) M H) bytes: the three P-shaped scratch blocks go, L' log-sum-exp blocks (L' = L,
    or 1 under activations recompute) and the D block of M H floats each come.  Up to the 64-float rounding of each block: 3 + L' + 1
    blocks can each round -> 256 (L + 4) bytes of slack.  The stored / recompute word changes nothing while fused is on; without the
    bf16 attention switch every query answers 0."""
    from rag4dyg_amd.lm_training import padded_vocab
    cfg, ldV = _cfg(L, H, d), padded_vocab(1000)
    slack = 256 * (L + 4)
    Lp = 1 if activations else L
    assert lib.r4d_set_train_activations(activations) == 0
    lib.r4d_set_train_attention_bf16(1)
    assert lib.r4d_set_train_attention(1) == 0
    rec = _queries(lib, cfg, batches, ldV)
    assert lib.r4d_set_train_attention_fused(1) == 0
    fused = _queries(lib, cfg, batches, ldV)
    assert lib.r4d_set_train_attention(0) == 0
    assert _queries(lib, cfg, batches, ldV) == fused                           # stored / recompute: no effect on a size
    blocks = [B * H * T * ((T + 127) // 128 * 128) for B, T in batches]
    want = {"retriever": 4 * (3 * max(blocks) - (Lp + 1) * sum(B * T for B, T in batches) * H)}
    for i, ((B, T), blk) in enumerate(zip(batches, blocks)):
        want[f"lm{i}"] = want[f"rag{i}"] = 4 * (3 * blk - (Lp + 1) * B * T * H)
    for k in rec:
        assert rec[k] > 0 and fused[k] > 0
        assert abs((rec[k] - fused[k]) - want[k]) <= slack, (k, rec[k], fused[k], want[k])
    if name == "wikiv2 script":
        lib.r4d_set_train_attention_fused(0)
        stored = _retriever_bytes(lib, cfg, batches)
        lib.r4d_set_train_attention_fused(1)
        print(f"wikiv2 script shape, activations {'recompute' if activations else 'stored'}: retriever workspace stored {stored} "
              f"recompute {rec['retriever']} fused {fused['retriever']} bytes")
    lib.r4d_set_train_attention_bf16(0)                                        # fused alone: refused by every query
    assert all(v == 0 for v in _queries(lib, cfg, batches, ldV).values())
    lib.r4d_set_train_attention_fused(0)
    assert all(v > 0 for v in _queries(lib, cfg, batches, ldV).values())


def test_single_op_workspace_query():
    lib = _lib.load()
    assert lib.r4d_train_attn_fused_bwd_workspace_bytes(3, 200, 2, 128) >= 4 * 3 * 2 * 200
    for B, T, H, d in ((1, 8, 1, 24), (1, 8, 1, 272), (1, 0, 1, 64), (1, 1025, 1, 64), (65536, 8, 1, 64), (1, 8, 3, 64)):
        assert lib.r4d_train_attn_fused_bwd_workspace_bytes(B, T, H, d) == 0, (B, T, H, d)


def test_resolver_keyword_environment_and_bad_names(monkeypatch):
    from rag4dyg_amd import training
    assert training.TRAIN_ATTENTION_KERNELS == {"products": 0, "fused": 1}
    assert training.TRAIN_ATTENTION_MODES == {"stored": 0, "recompute": 1}
    monkeypatch.delenv("R4D_TRAIN_ATTENTION_KERNEL", raising=False)
    assert training.resolve_train_attention_kernel() == "products"
    monkeypatch.setenv("R4D_TRAIN_ATTENTION_KERNEL", "")
    assert training.resolve_train_attention_kernel() == "products"             # empty means the default
    monkeypatch.setenv("R4D_TRAIN_ATTENTION_KERNEL", "fused")
    assert training.resolve_train_attention_kernel() == "fused"
    assert training.resolve_train_attention_kernel("products") == "products"   # the keyword wins
    for bad in ("Fused", "flash", "1", 1, "recompute"):
        with pytest.raises(ValueError):
            training.resolve_train_attention_kernel(bad)
    monkeypatch.setenv("R4D_TRAIN_ATTENTION_KERNEL", "flash")
    with pytest.raises(ValueError):
        training.resolve_train_attention_kernel()
    for precision in ("fp32+attn", "bf16+attn"):
        assert training.check_attention_kernel("fused", precision) == "fused"
    for precision in ("fp32", "bf16"):
        assert training.check_attention_kernel("products", precision) == "products"
        with pytest.raises(ValueError, match=r"fp32\+attn.*bf16\+attn"):
            training.check_attention_kernel("fused", precision)


def test_fused_without_attn_precision_raises_at_trainer_construction(monkeypatch):
    """All three trainers build a training.EncoderTrainer, whose constructor resolves the modes before it looks at the model: with a
    model of None the pairing error must come first ('fused' under 'bf16' / 'fp32'), and a valid pairing must get past it (to the
    AttributeError of the missing model)."""
    from rag4dyg_amd import generator_training, lm_training, training
    monkeypatch.delenv("R4D_TRAIN_ATTENTION_KERNEL", raising=False)

    class _Model:                                                              # enough of a model for the LM / generator trainers' own checks
        class _T:
            class wte:
                weight = object()
        transformer = _T()

        class _H:
            weight = None
        lm_head = _H()

        class _G:
            n_layers = 1
        gnn_fusion = _G()
    _Model.lm_head.weight = _Model.transformer.wte.weight
    builders = (lambda **kw: training.EncoderTrainer(None, **kw),
                lambda **kw: lm_training.LMTrainer(_Model(), **kw),
                lambda **kw: generator_training.GeneratorTrainer(_Model(), False, **kw))
    for build in builders:
        for precision in ("fp32", "bf16"):
            with pytest.raises(ValueError, match="fused"):
                build(precision=precision, attention_kernel="fused")
            monkeypatch.setenv("R4D_TRAIN_ATTENTION_KERNEL", "fused")
            with pytest.raises(ValueError, match="fused"):
                build(precision=precision)
            monkeypatch.delenv("R4D_TRAIN_ATTENTION_KERNEL")
        with pytest.raises(AttributeError):                                    # past the pairing check, at the model
            build(precision="bf16+attn", attention_kernel="fused")


def test_fp16_is_still_refused():
    from rag4dyg_amd import generator_training, lm_training, training
    args = argparse.Namespace(fp16=True, should_continue=False, fusion="graphpooling", gnn_layers=1, m=1)
    for train in (training.train, lm_training.train, generator_training.train):
        with pytest.raises(NotImplementedError):
            train(args, None, None, None, precision="bf16+attn", attention_kernel="fused")


def test_tools_take_the_option():
    for tool in ("bench_components.py", "lm_train_bench.py", "gen_train_bench.py", "train_workspace_table.py"):
        text = open(os.path.join(REPO, "tools", tool)).read()
        assert "fused" in text and ("attention_kernel" in text or "attention-kernel" in text), tool
