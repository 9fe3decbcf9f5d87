"""Layer 0's repeated pad rows (``include/r4d.h``: r4d_set_layer0_pad_rows; ``csrc/encoder.hip``): with the switch on, the layer-0
c_attn GEMM of the f16x2 path skips the 32-row blocks that hold one repeated token and a copy fills them from a per-call table.
The claim is bit-identity, so every comparison here is ``torch.equal`` between a run with the switch on and one with it off:
mean-pool, hidden states, the per-layer residual stream.  The plan the device built (candidate token, kept and dropped block
lists) is read back from the workspace and compared with the NumPy restatement in tests/_layer0_pad_rows_ref.py.

``out_layers`` exists on the one-batch entry point only (``r4d_gpt2_encode_f32``): it is compared through that entry on each
batch of a call, mean-pool and hidden through ``r4d_gpt2_encode_groups_ex_f32`` on the whole call."""
import ctypes

import numpy as np
import pytest
import torch

import _poison
from _layer0_pad_rows_ref import classify

pytestmark = pytest.mark.gpu

V, P, PAD = 64, 128, 63
BRANCH = "gemm_h2p:row-block map (layer 0 c_attn without the repeated pad-row blocks)"
MODELS = {"L2_H2_d256": (2, 2, 256), "L1_H2_d512": (1, 2, 512)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def f16x2():
    from rag4dyg_amd import ops
    before = ops.gemm_mode()
    ops.set_gemm_mode("f16x2")
    yield
    ops.set_gemm_mode(before)


@pytest.fixture(scope="module", params=sorted(MODELS))
def model(request, dev, f16x2):
    from oracle import gpt2_ref
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModelRAG
    L, H, d = MODELS[request.param]
    sd = gpt2_ref.make_state_dict(L, d, V, n_positions=P, seed=21, random_affine=True)
    m = GPT2LMHeadModelRAG(GPT2Config(vocab_size=V, n_positions=P, n_ctx=P, n_embd=d, n_layer=L, n_head=H))
    m.load_state_dict(sd, strict=False)
    m.tie_weights()
    return m.to(dev).eval().transformer


def _ragged(rng, lens, T, pad=PAD):
    b = np.full((len(lens), T), pad, np.int64)
    for i, n in enumerate(lens):
        b[i, :n] = rng.integers(0, PAD, n)                               # real tokens never equal the pad
    return b


def _calls():
    rng = np.random.default_rng(5)
    calls = {}
    # sequences start in the middle of a block, M = 99 + 280 + 480 = 859, M % 32 = 27
    calls["T33_T70_T96"] = [_ragged(rng, (33, 4, 9), 33), _ragged(rng, (70, 2, 30, 5), 70), _ragged(rng, (3, 96, 7, 2, 50), 96)]
    calls["nearly_all_pad"] = [_ragged(rng, (120, 2, 2, 2), 120), _ragged(rng, (2, 2, 77), 77)]
    calls["no_pad"] = [_ragged(rng, (40, 40, 40), 40), _ragged(rng, (65,) * 4, 65)]
    inside = _ragged(rng, (128, 6, 3), 128)
    inside[0, 20:100] = PAD                                              # a run of 80 pads in mid-sequence: dropped legitimately
    inside[0, 5] = PAD
    calls["pad_inside_sequences"] = [inside, _ragged(rng, (50, 2, 2, 9), 50)]
    other = _ragged(rng, (100,) * 4, 100)
    other[:, -1] = 7                                                     # every sequence is full and ends in 7: the majority is not the pad
    other[1, 10:90] = 7
    calls["majority_is_not_the_pad"] = [other, other[:3, :].copy()]
    calls["T128_n_positions"] = [_ragged(rng, (128, 3, 40, 2), 128), _ragged(rng, (128, 128, 5), 128)]
    return calls


CALLS = _calls()


def _branch_hits():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    for i in range(lib.r4d_dispatch_num_branches()):
        if lib.r4d_dispatch_branch_name(i).decode() == BRANCH:
            return int(lib.r4d_dispatch_branch_hits(i))
    raise AssertionError("no dispatcher branch named " + BRANCH)


def _run(model, dev, batches, on, want_qkv=False):
    """One call with the switch set; returns (outputs, hits of the new branch)."""
    from rag4dyg_amd import ops
    ts = [torch.from_numpy(b).to(dev) for b in batches]
    prev = ops.set_layer0_pad_rows(on)
    try:
        h0 = _branch_hits()
        out = model.encode_groups(ts, want_hidden=True, want_meanpool=True, want_qkv=want_qkv)
        layers = [model.encode(t, want_hidden=False, want_meanpool=True, want_layers=True)["layers"] for t in ts]
        torch.cuda.synchronize()
        hits = _branch_hits() - h0
    finally:
        ops.set_layer0_pad_rows(prev)
    return dict(hidden=out["hidden"], meanpool=out["meanpool"], qkv=out["qkv"], layers=layers), hits


def _plan(model, dev, batches):
    """The plan of the LAST groups call, as the device left it in the workspace."""
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    c, _w, _keep = model._c_structs()
    n = len(batches)
    Bs = (ctypes.c_int32 * n)(*[b.shape[0] for b in batches])
    Ts = (ctypes.c_int32 * n)(*[b.shape[1] for b in batches])
    off = int(lib.r4d_gpt2_layer0_pad_rows_offset(ctypes.byref(c), n, Bs, Ts))
    assert off > 0 and off % 4 == 0
    words = ops._WS[(str(dev), "gpt2")][off:].view(torch.int32).cpu().numpy()
    n_list, n_drop, tok, o_list, o_drop = (int(x) for x in words[:5])
    return dict(c=tok, listed=words[o_list:o_list + n_list], dropped=words[o_drop:o_drop + n_drop])


def _assert_same(a, b, what):
    assert torch.equal(a["meanpool"], b["meanpool"]), what
    assert torch.equal(a["hidden"], b["hidden"]), what
    assert len(a["layers"]) == len(b["layers"])
    for x, y in zip(a["layers"], b["layers"]):
        assert torch.equal(x, y), what
    assert torch.isfinite(a["hidden"]).all() and torch.isfinite(a["meanpool"]).all(), what


@pytest.mark.parametrize("name", sorted(CALLS))
def test_switch_on_equals_switch_off_bit_for_bit(model, dev, name):
    from rag4dyg_amd import ops
    batches = CALLS[name]
    ref = classify(batches)
    on, hits_on = _run(model, dev, batches, True)
    # the groups call of _run came first; the one-batch calls that followed reuse the workspace: read the plan of a fresh call
    prev = ops.set_layer0_pad_rows(True)
    try:
        model.encode_groups([torch.from_numpy(b).to(dev) for b in batches], want_hidden=False, want_meanpool=True)
        plan = _plan(model, dev, batches)
    finally:
        ops.set_layer0_pad_rows(prev)
    off, hits_off = _run(model, dev, batches, False)
    assert hits_on == 1 + len(batches) and hits_off == 0, (hits_on, hits_off)
    _assert_same(on, off, name)
    print(name, "c", plan["c"], "blocks", ref["Mp"] // 32, "dropped", len(plan["dropped"]), "listed", len(plan["listed"]))
    assert plan["c"] == ref["c"]
    assert np.array_equal(plan["listed"], ref["listed"]) and np.array_equal(plan["dropped"], ref["dropped"])
    if name == "no_pad":
        assert ref["dropped"].size == 0
    elif name == "majority_is_not_the_pad":
        assert ref["c"] == 7 and ref["dropped"].size >= 1
    else:
        assert ref["c"] == PAD and ref["dropped"].size >= 1


def test_switch_is_inert_when_qkv_is_handed_out(model, dev):
    batches = CALLS["T33_T70_T96"]
    on, hits_on = _run(model, dev, batches, True, want_qkv=True)
    off, hits_off = _run(model, dev, batches, False, want_qkv=True)
    assert hits_on == len(batches) and hits_off == 0                     # only _run's one-batch calls (no qkv there) take the path
    assert torch.equal(on["qkv"], off["qkv"]) and torch.equal(on["hidden"], off["hidden"]) and torch.equal(on["meanpool"], off["meanpool"])


@pytest.mark.parametrize("pattern", [_poison.NAN, _poison.HUGE, _poison.ONE])
def test_poisoned_workspace_gives_the_same_bits(model, dev, pattern):
    """No dropped row's stale LayerNorm line, list padding entry, row past M or block past M' may reach a result: the plan's
    words are all written on the device before they are read, so every pattern may fill the whole workspace."""
    from rag4dyg_amd import ops
    batches = CALLS["T33_T70_T96"]
    clean, _ = _run(model, dev, batches, True)
    ts = [torch.from_numpy(b).to(dev) for b in batches]
    prev = ops.set_layer0_pad_rows(True)
    try:
        _poison.poison(ops._WS[(str(dev), "gpt2")], pattern)
        out = model.encode_groups(ts, want_hidden=True, want_meanpool=True)
        torch.cuda.synchronize()
    finally:
        ops.set_layer0_pad_rows(prev)
    assert torch.isfinite(out["hidden"]).all() and torch.isfinite(out["meanpool"]).all()
    assert torch.equal(out["hidden"], clean["hidden"]) and torch.equal(out["meanpool"], clean["meanpool"])
