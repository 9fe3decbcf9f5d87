"""The Conv1D routing query against what the dispatchers launch (``r4d_conv1d_route``, csrc/conv1d_route.h): for every gemm mode
and precision, the dispatch counters of one encoder call and one retriever training step equal the counts predicted by summing the
query over the block's Conv1D calls, with the weight forms (`have`) read from the very structs the call receives.

Shapes: the smallest at which every route exists -- one layer, d 128, 4 heads, vocabulary 128, B 4 x T 8 = 32 rows (the TN kernels'
M >= 32; I = 128; c_fc's J = 512 takes the TN kernels, c_attn's J = 384 their fallback); the decode step at d 512, B 2 (skinny
needs K % 256 == 0).

The GELU fusion (csrc/train.hip: c_fc forward with GELU_KEEP, mlp.c_proj data gradient with GELU_GRAD) is covered INDIRECTLY,
through bits: neither the branch table nor the profile classes see the two element-wise GELU launches, and a fused GEMM counts in
the same family as an unfused one.  ``R4D_TRAIN_FUSE_GELU`` is read once per process, so ``test_gelu_fusion_switch`` runs the same
step in two child processes, switch on and off: where the predicates say "fused" (bf16x3 planes) the bits must differ, where they
say "not fusable" (exact f32, no planes) they must be the same.

Every test restores the switches it found."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

WT, W3, W3T, H2, SK = 1, 2, 4, 8, 16
NONE, GELU, RESIDUAL, GELU_KEEP = 0, 1, 2, 5
CONV1D = ("c_attn", "attn_proj", "c_fc", "mlp_proj")
MODES = {"f32": 0, "bf16x3": 1, "f16x2": 2}
# dispatch counters that fire ONCE per launch of a kernel family
FAMILIES = {
    "s3": ("gemm_s3:128x256x32", "gemm_s3:128x256x32 persistent (pipeline across tiles)", "gemm_s3:128x128x32"),
    "h2": ("gemm_h2:128x256x32 (f16x2)", "gemm_h2:128x128x32 (f16x2)", "gemm_h2p:128x256x32 (f16x2, A as lines, LDS-DMA)",
           "gemm_h2p:128x128x32 (f16x2, A as lines, LDS-DMA)"),
    "f32": ("gemm_kc:128x128x16", "gemm_kc:128x64x16", "gemm_kc:64x64x32", "tuning:gemm_kc:128x128x32", "gemm_f32:128x128",
            "gemm_f32:128x64", "gemm_f32:64x64"),
    "b1": ("tuning:encode_bf16:128x256x32", "tuning:encode_bf16:128x128x32"),
    "train_bf16:fwd": ("tuning:train_bf16:fwd",), "train_bf16:dgrad": ("tuning:train_bf16:dgrad",),
    "train_bf16:wgrad": ("tuning:train_bf16:wgrad",), "train_bf16:wgrad_fallback": ("tuning:train_bf16:wgrad_fallback",),
    "s3tn": ("gemm_s3tn:128x256x32 (weight gradients, transposing LDS reads)",), "tn": ("gemm_tn:split-K", "gemm_tn:one slice"),
    "skinny": ("skinny16:ng2", "skinny16:ng3", "skinny16:ng2+layernorm", "skinny16:LayerNorm pre-folded into the weight",
               "skinny16:ng3+layernorm", "skinny8:ng2", "skinny8:ng3", "skinny:plain + epilogue launch"),
}
ROW_SPLIT = "gemm_kc:row-split (two launches)"          # one more tile counter per hit


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def restore_switches(dev):
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    was = (lib.r4d_get_train_bf16(), ops.encode_precision(), ops.gemm_mode())
    yield
    lib.r4d_set_train_bf16(was[0])
    ops.set_encode_precision(was[1])
    ops.set_gemm_mode(was[2])


def model_of(dev, d, H, V=128):
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModelRAG
    torch.manual_seed(d)
    m = GPT2LMHeadModelRAG(GPT2Config(vocab_size=V, n_positions=16, n_ctx=16, n_embd=d, n_layer=1, n_head=H))
    m.tie_weights()
    return m.to(dev).eval()


def launches():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    raw = {lib.r4d_dispatch_branch_name(i).decode(): int(lib.r4d_dispatch_branch_hits(i)) for i in range(lib.r4d_dispatch_num_branches())}
    out = {f: sum(raw[n] for n in names) for f, names in FAMILIES.items()}
    out["f32"] -= raw[ROW_SPLIT]
    return out


def have_of(layer, name):
    return sum(bit for bit, field in ((WT, "_wT"), (W3, "_w3"), (W3T, "_w3t"), (H2, "_h2")) if getattr(layer, name + field))


def route(kind, M, K, N, epilogue, have, bf16):
    from rag4dyg_amd import _lib
    lib = _lib.load()
    return lib.r4d_conv1d_route_name(lib.r4d_conv1d_route(kind, M, K, N, epilogue, have, bf16)).decode()


def shapes(d):
    return {"c_attn": (d, 3 * d), "attn_proj": (d, d), "c_fc": (d, 4 * d), "mlp_proj": (4 * d, d)}


FAMILY_OF = {"skinny": "skinny", "h2": "h2", "s3": "s3", "b1": "b1", "f32_kcopy": "f32", "f32_ref": "f32", "dgrad_b1": "b1",
             "dgrad_s3": "s3", "dgrad_f32": "f32", "wgrad_b1tn": None, "wgrad_s3tn": "s3tn", "wgrad_f32tn": "tn"}


def predicted(routes, extra_f32=0):
    want = {f: 0 for f in FAMILIES}
    want["f32"] = extra_f32
    for r in routes:
        if FAMILY_OF[r]:
            want[FAMILY_OF[r]] += 1
    return want


@pytest.mark.parametrize("precision", ("fp32", "bf16"))
@pytest.mark.parametrize("mode", tuple(MODES))
def test_encoder_call_launches_what_the_query_names(dev, mode, precision):
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    ops.set_gemm_mode(mode)
    ops.set_encode_precision(precision)
    m = model_of(dev, 128, 4)
    ids = torch.randint(0, 128, (4, 8), generator=torch.Generator().manual_seed(1)).to(dev)
    _c, _w, layers = m.transformer._c_structs()
    # (in f16x2 mode c_attn may write h2 words for the f16x2 attention instead: the same route)
    epi = {"c_attn": NONE, "attn_proj": RESIDUAL, "c_fc": GELU, "mlp_proj": RESIDUAL}
    routes = [route(0, 32, *shapes(128)[n], epi[n], have_of(layers[0], n), precision == "bf16") for n in CONV1D]
    lib.r4d_dispatch_reset()
    out = m.transformer.encode(ids, want_hidden=True)["hidden"]
    torch.cuda.synchronize()
    got = launches()
    assert torch.isfinite(out).all()
    assert got == predicted(routes), (routes, got)
    want_route = "b1" if precision == "bf16" else {"f32": "f32_kcopy", "bf16x3": "s3", "f16x2": "h2"}[mode]
    assert routes == [want_route] * 4, routes


@pytest.mark.parametrize("precision", ("fp32", "bf16"))
@pytest.mark.parametrize("mode", tuple(MODES))
def test_training_step_launches_what_the_query_names(dev, mode, precision):
    from rag4dyg_amd import _lib, ops, training
    lib = _lib.load()
    ops.set_gemm_mode(mode)
    m = model_of(dev, 128, 4)
    tr = training.EncoderTrainer(m, precision=precision)
    ids = torch.randint(0, 128, (4, 8), generator=torch.Generator().manual_seed(2)).to(dev)
    G = torch.randn(4, 128, generator=torch.Generator().manual_seed(3)).to(dev)
    layer = tr._structs()[3][0][0]
    bf16, M, sh = precision == "bf16", 32, shapes(128)
    have = {n: have_of(layer, n) for n in CONV1D}
    # csrc/train.hip (layer_forward): c_fc leaves gelu(v) and v from ONE launch where a kernel with that epilogue takes it
    fc_keep = route(2, M, *sh["c_fc"], GELU_KEEP, have["c_fc"], bf16)
    fused = fc_keep in ("b1", "s3") or (fc_keep == "h2" and bool(have["c_fc"] & W3))
    assert fused == (mode != "f32" or bf16)
    epi = {"c_attn": NONE, "attn_proj": RESIDUAL, "c_fc": GELU_KEEP if fused else NONE, "mlp_proj": RESIDUAL}
    fwd = [route(2, M, *sh[n], epi[n], have[n], bf16) for n in CONV1D]
    dgrad = [route(3, M, *sh[n], NONE, have[n], bf16) for n in CONV1D]
    wgrad = [route(5, M, *sh[n], NONE, have[n], bf16) for n in CONV1D]
    # the attention's batched per-head GEMMs are exact-f32 launches too, not Conv1D: 2 forward, 4 backward per block and batch
    want = predicted(fwd + dgrad + wgrad, extra_f32=6)
    want["train_bf16:fwd"] = fwd.count("b1")
    want["train_bf16:dgrad"] = dgrad.count("dgrad_b1")
    want["train_bf16:wgrad"] = wgrad.count("wgrad_b1tn")
    want["train_bf16:wgrad_fallback"] = (4 - wgrad.count("wgrad_b1tn")) if bf16 else 0
    lib.r4d_dispatch_reset()
    emb = tr.forward([ids])
    grads = tr.backward(G)
    torch.cuda.synchronize()
    got = launches()
    assert torch.isfinite(emb).all() and all(torch.isfinite(g).all() for g in grads.values())
    assert got == want, (fwd, dgrad, wgrad, got, want)
    # what the matrix is meant to reach at these shapes
    assert fwd == [("b1" if bf16 else {"f32": "f32_kcopy", "bf16x3": "s3", "f16x2": "h2"}[mode])] * 4, fwd
    assert dgrad == [("dgrad_b1" if bf16 else "dgrad_f32" if mode == "f32" else "dgrad_s3")] * 4, dgrad
    # 32 rows: one slice, so bf16x3 stays on f32tn; b1tn where J % 256 == 0 (c_fc 512; not 384, 128, 128)
    assert wgrad == (["wgrad_f32tn", "wgrad_f32tn", "wgrad_b1tn", "wgrad_f32tn"] if bf16 else ["wgrad_f32tn"] * 4), wgrad


def test_weight_gradient_reaches_s3tn_beyond_one_slice(dev):
    """The single op at 390 rows (two slices): bf16x3 takes gemm_s3tn at J 512, the fallback at J 384; exact f32 never."""
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(4)
    x = torch.randn(390, 128, generator=g).to(dev)
    for mode in ("bf16x3", "f32"):
        ops.set_gemm_mode(mode)
        for J in (512, 384):
            dy = torch.randn(390, J, generator=g).to(dev)
            r = route(5, 390, 128, J, NONE, 0, 0)
            assert r == ("wgrad_s3tn" if mode == "bf16x3" and J == 512 else "wgrad_f32tn")
            dw, db = torch.empty(128, J, device=dev), torch.empty(J, device=dev)
            ws = torch.empty(max(int(lib.r4d_weight_grad_workspace_bytes(390, 128, J)), 256), dtype=torch.uint8, device=dev)
            lib.r4d_dispatch_reset()
            _lib.check(lib.r4d_weight_grad_f32(x.data_ptr(), dy.data_ptr(), 390, 128, J, dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                               ws.numel(), torch.cuda.current_stream().cuda_stream), "weight_grad")
            torch.cuda.synchronize()
            got = launches()
            assert got == predicted([r]), (mode, J, got)
            ref = x.double().t() @ dy.double()
            assert float((dw.double() - ref).abs().max() / ref.abs().max()) < 1e-5
            assert torch.allclose(db.double(), dy.double().sum(0), rtol=1e-5, atol=1e-4)


def _tn_slices(rows, I, J):
    """(wanted slices, k-tiles of each slice that holds rows) of gemm_s3tn under weight_grad: csrc/common.h gemm_tn_slices within
    csrc/conv1d_route.h tn_splits, cut into whole 32-row steps (tn_row_slices)."""
    cdiv = lambda a, b: -(-a // b)
    splits = max(1, min(cdiv(1024, cdiv(I, 128) * cdiv(J, 128)), cdiv(rows, 256), 64))
    S = max(1, min(cdiv(512, (I // 128) * (J // 256)), cdiv(rows, 256), splits))
    kper = cdiv(cdiv(rows, S), 32) * 32
    return S, [cdiv(min(rows, lo + kper) - lo, 32) for lo in range(0, rows, kper)]


@pytest.mark.parametrize("rows", (257, 545))
def test_weight_gradient_on_s3tn_at_uneven_slices(dev, rows):
    """gemm_s3tn as a single op in bf16x3 mode, in 128, out 512, at the row counts where its two-stage loop and its tail differ:
    257 rows = two slices of 5 and 4 k-tiles (both parities of the loop, a last k-tile of ONE row), 545 rows = three slices of 6
    k-tiles, the last one again ending on one row.  The route, the launch counters, dW and db against float64 at the bounds of
    the 390-row test above, and the same bits from a second run."""
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    I, J = 128, 512
    assert _tn_slices(rows, I, J) == {257: (2, [5, 4]), 545: (3, [6, 6, 6])}[rows]
    assert rows % 32 == 1
    ops.set_gemm_mode("bf16x3")
    g = torch.Generator().manual_seed(rows)
    x, dy = torch.randn(rows, I, generator=g).to(dev), torch.randn(rows, J, generator=g).to(dev)
    r = route(5, rows, I, J, NONE, 0, 0)
    assert r == "wgrad_s3tn"
    ws = torch.empty(max(int(lib.r4d_weight_grad_workspace_bytes(rows, I, J)), 256), dtype=torch.uint8, device=dev)
    runs = []
    for _ in range(2):
        dw, db = torch.empty(I, J, device=dev), torch.empty(J, device=dev)
        lib.r4d_dispatch_reset()
        _lib.check(lib.r4d_weight_grad_f32(x.data_ptr(), dy.data_ptr(), rows, I, J, dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                           ws.numel(), torch.cuda.current_stream().cuda_stream), "weight_grad")
        torch.cuda.synchronize()
        got = launches()
        assert got == predicted([r]), (rows, got)
        runs.append((dw, db))
    dw, db = runs[0]
    ref = x.double().t() @ dy.double()
    assert float((dw.double() - ref).abs().max() / ref.abs().max()) < 1e-5
    assert torch.allclose(db.double(), dy.double().sum(0), rtol=1e-5, atol=1e-4)
    assert torch.equal(runs[1][0], dw) and torch.equal(runs[1][1], db)


def test_decode_step_takes_the_skinny_route(dev):
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    ops.set_gemm_mode("bf16x3")
    m = model_of(dev, 512, 8)
    B, d = 2, 512
    ids = torch.randint(0, 128, (B, 4), generator=torch.Generator().manual_seed(5)).to(dev)
    kv = m.transformer.new_kv_cache(B, 16, dev)
    m.transformer.prefill(kv, input_ids=ids)
    _c, _w, layers = m.transformer._c_structs(decode=True)
    epi = {"c_attn": NONE, "attn_proj": RESIDUAL, "c_fc": GELU, "mlp_proj": RESIDUAL}
    routes = [route(1, B, *shapes(d)[n], epi[n], have_of(layers[0], n) | SK, 0) for n in CONV1D]
    assert routes == ["skinny"] * 4
    assert [route(1, 33, *shapes(d)[n], epi[n], have_of(layers[0], n), 0) for n in CONV1D] == ["f32_kcopy"] * 4     # B > 32: no scratch
    pos = torch.full((B,), 4, dtype=torch.int32, device=dev)
    lib.r4d_dispatch_reset()
    h = m.transformer.decode_step(kv, pos, input_ids=ids[:, -1].contiguous())
    torch.cuda.synchronize()
    got = launches()
    assert torch.isfinite(h).all()
    assert got == predicted(routes), got          # (c_fc's LayerNorm-fused launch is the skinny kernel too)


def test_gelu_fusion_switch(dev):
    """One step in two child processes (tests/_fuse_gelu_child.py), R4D_TRAIN_FUSE_GELU=1 and =0, started together.  The fused
    epilogues round differently from GEMM + element-wise launch (the GELU sees the accumulator, not the stored fp32 value's
    reload through another kernel's arithmetic), so in bf16x3 mode -- where the forward predicate (conv1d_fuses_gelu_keep) and the
    backward one (dgrad_route != dgrad_f32) both hold -- the step's bits differ with the switch; in exact-f32 mode the trainer
    carries no planes, neither predicate holds, and the switch must change nothing.  A predicate that fused nowhere would fail
    the first assertion, one that ignored the route the second (or be refused by data_grad)."""
    assert route(2, 32, 128, 512, GELU_KEEP, WT | W3 | W3T, 0) == "s3" and route(3, 32, 512, 128, NONE, WT | W3 | W3T, 0) == "dgrad_s3"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_fuse_gelu_child.py")
    procs = [subprocess.Popen([sys.executable, child], env=dict(os.environ, R4D_TRAIN_FUSE_GELU=v, R4D_TRAIN_SPLIT3="1", R4D_TRAIN_WT="1"),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for v in ("1", "0")]
    res = []
    for p in procs:
        o, e = p.communicate(timeout=120)
        assert p.returncode == 0, e[-2000:]
        res.append(json.loads(o.strip().splitlines()[-1]))
    fused, unfused = res
    assert fused["bf16x3"] != unfused["bf16x3"], "the switch changed nothing where both predicates fuse"
    assert fused["f32"] == unfused["f32"], "the switch changed an exact-f32 step without planes"
