"""The encoder's opt-in bf16 precision on the GPU (``ops.set_encode_precision("bf16")``, ``r4d_conv1d_bf16_f32``,
csrc/gemm_b1.hip): the single op against float64 of the bf16-rounded operands at a derived bound, its row independence,
repeatability, bounds and rejections; the encoder under the switch against "the emulation" (tests/_encode_bf16_ref.py: the
oracle with ``conv1d``'s operands rounded through ``torch.bfloat16``); and the isolation of everything the switch must not touch.

Every test restores the precision switch and the gemm mode it found."""

import pytest
import torch

import _encode_bf16_ref as R
from _poison import HUGE, NAN, ZERO, poison
from conftest import GEMM_MODES, assert_tokens_equal_or_tie, load_state_dict_checked

pytestmark = pytest.mark.gpu

BRANCH_PREFIX = "tuning:encode_bf16:"
EPILOGUE_TOL = 1e-5      # tests/test_gpu_ops.py: the bound of conv1d_s3's / conv1d_h2's GELU and residual epilogues (max-norm, relative)
GELU_SLOPE = 1.13        # max |d gelu_new / dx| = 1.1290


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def restore_switches(dev):
    from rag4dyg_amd import ops
    prec, mode = ops.encode_precision(), ops.gemm_mode()
    yield
    ops.set_encode_precision(prec)
    ops.set_gemm_mode(mode)


def hits(prefix=BRANCH_PREFIX):
    from rag4dyg_amd import _lib
    lib = _lib.load()
    out = {}
    for i in range(lib.r4d_dispatch_num_branches()):
        n = lib.r4d_dispatch_branch_name(i).decode()
        if n.startswith(prefix):
            out[n] = int(lib.r4d_dispatch_branch_hits(i))
    return out


def operands(M, K, N, dev, seed=0):
    g = torch.Generator().manual_seed(1000 * M + 10 * K + N + seed)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(K, N, generator=g) * 0.05
    b = torch.randn(N, generator=g) * 0.1
    r = torch.randn(M, N, generator=g)
    return x.to(dev), w.to(dev), b.to(dev), r.to(dev)


def model_on(dev, name):
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModel
    sd, L, H, d, V, P, ids = R.fixture(name)
    m = GPT2LMHeadModel(GPT2Config(vocab_size=V, n_positions=P, n_ctx=P, n_embd=d, n_layer=L, n_head=H))
    load_state_dict_checked(m, {k: v for k, v in sd.items() if k != "lm_head.weight"})
    m.tie_weights()
    return m.to(dev).eval(), ids


# ------------------------------------------------------------------------------------------------------------ the single op
GRID_M, GRID_K, GRID_N = (1, 31, 128, 129, 300), (32, 64, 96, 512, 2048), (64, 200, 256, 1536)
# The project's tile rule (fewest tile rounds over the CUs, the narrow tile winning ties) gives every shape of the grid above --
# at most 36 tiles -- to the 128 x 128 tile.  The 128 x 256 tile takes over where the narrow one needs a second round: these
# shapes ADD it, with interior tiles only, with edge tiles in M and N, and with one / an odd number of / many k-tiles.
WIDE_SHAPES = ((4096, 64, 1536), (4096, 32, 1536), (4000, 96, 1500), (4000, 512, 1500))


def check_op(M, K, N, dev):
    """One shape, the three epilogues, element-wise against float64 of the bf16-rounded operands.  bf16 x bf16 is exact in
    fp32, so the only roundings are the K - 1 additions of the accumulation and the bias add: |y - y64| <= (K + 2) 2^-24
    (|x^| . |w^|^T + |bias|)."""
    from rag4dyg_amd import ops
    x, w, b, r = operands(M, K, N, dev)
    plane = ops.bf16_plane(w)
    xh, wh = x.bfloat16().double(), w.bfloat16().double()
    y64 = xh @ wh + b.double()
    bound = (K + 2) * 2.0 ** -24 * (xh.abs() @ wh.abs() + b.abs().double())
    y = ops.conv1d_bf16(x, plane, b)
    e_none = float(((y.double() - y64).abs() / bound).max())
    g64 = R.gpt2_ref.gelu_new(y64)
    yg = ops.conv1d_bf16(x, plane, b, "gelu")
    e_gelu = float(((yg.double() - g64).abs() / (GELU_SLOPE * bound + EPILOGUE_TOL * g64.abs().max())).max())
    r64 = y64 + r.double()
    yr = ops.conv1d_bf16(x, plane, b, "residual", r)
    e_res = float(((yr.double() - r64).abs() / (bound + EPILOGUE_TOL * r64.abs().max())).max())
    y0 = ops.conv1d_bf16(x, plane, None)                                 # no bias
    e_nob = float(((y0.double() - (xh @ wh)).abs() / bound).max())
    return e_none, e_gelu, e_res, e_nob


def test_01_conv1d_bf16_sizes_epilogues_and_tiles(dev):
    before = hits()
    worst = {}
    for (M, K, N) in [(M, K, N) for M in GRID_M for K in GRID_K for N in GRID_N] + list(WIDE_SHAPES):
        e = check_op(M, K, N, dev)
        worst[(M, K, N)] = e
        assert max(e) <= 1.0, f"M={M} K={K} N={N}: |error| / bound (none, gelu, residual, no bias) = {e}"
    after = hits()
    w_ = max(worst, key=lambda s: worst[s][0])
    print(f"conv1d_bf16: {len(worst)} shapes; largest |y - y64| / bound {worst[w_][0]:.3f} at {w_}; gelu {max(v[1] for v in worst.values()):.3f} "
          f"residual {max(v[2] for v in worst.values()):.3f}; launches per tile {({n: after[n] - before[n] for n in after})}")
    assert len(after) >= 2 and all(after[n] > before[n] for n in after), (before, after)      # every tile variant the dispatcher has


def test_02_bf16_plane_has_the_bits_of_torch_bfloat16(dev):
    from rag4dyg_amd import ops
    g = torch.Generator().manual_seed(5)
    w = torch.randn(96, 200, generator=g) * 0.05
    # ties (round to even), a sign, a subnormal, the largest finite bf16 and a value that rounds up to infinity
    w[0, :8] = torch.tensor([1.00390625, 1.01171875, -1.00390625, 1e-40, 3.3895314e38, 3.4e38, -0.0, 65280.5])
    w = w.to(dev)
    plane = ops.bf16_plane(w)
    assert plane.shape == (200, 96) and plane.dtype == torch.int16 and plane.is_contiguous()
    assert torch.equal(plane, w.t().contiguous().to(torch.bfloat16).view(torch.int16))
    assert torch.equal(plane, ops.split3_planes(w)[0])                  # plane 0 of the bf16x3 planes
    assert torch.equal(ops.bf16_plane(w.t().contiguous(), transposed=True), plane)


@pytest.mark.parametrize("N", GRID_N)
def test_03_rows_do_not_depend_on_the_call_they_travel_in(dev, N):
    """Rows of the M = 300 call == the same rows computed with M = 1 and M = 129 (from either end), and == the rows of a
    4096-row call (N = 1536: that one runs on the other tile shape), bit for bit, for every epilogue."""
    from rag4dyg_amd import ops
    K = 512
    x, w, b, r = operands(4096, K, N, dev)
    plane = ops.bf16_plane(w)
    for epi in ("none", "gelu", "residual"):
        def run(lo, hi):
            return ops.conv1d_bf16(x[lo:hi].contiguous(), plane, b, epi, r[lo:hi].contiguous() if epi == "residual" else None)
        y300 = run(0, 300)
        assert torch.equal(run(0, 1), y300[0:1]) and torch.equal(run(299, 300), y300[299:300]), (N, epi, "M = 1")
        assert torch.equal(run(0, 129), y300[:129]) and torch.equal(run(171, 300), y300[171:]), (N, epi, "M = 129")
        assert torch.equal(run(0, 4096)[:300], y300), (N, epi, "M = 4096")
    if N == 1536:
        assert all(v > 0 for v in hits().values())                       # both tile shapes took part


def test_04_two_launches_give_the_same_bits(dev):
    from rag4dyg_amd import ops
    for (M, K, N) in ((300, 2048, 1536), (4000, 512, 1500)):
        x, w, b, r = operands(M, K, N, dev)
        plane = ops.bf16_plane(w)
        for epi in ("none", "gelu", "residual"):
            a = ops.conv1d_bf16(x, plane, b, epi, r if epi == "residual" else None)
            assert torch.equal(a, ops.conv1d_bf16(x, plane, b, epi, r if epi == "residual" else None)), (M, K, N, epi)


def _raw_conv1d_bf16(x, plane, b, r, epi, y_ptr, M, K, N):
    from rag4dyg_amd import _lib
    return _lib.load().r4d_conv1d_bf16_f32(x.data_ptr(), plane.data_ptr() if plane is not None else None, b.data_ptr(),
                                           r.data_ptr() if r is not None else None, M, K, N, epi, y_ptr,
                                           torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("M,K,N", [(129, 96, 200), (300, 64, 1536), (1, 32, 64), (4000, 64, 1500)])
def test_05_guard_rows_and_columns_stay_untouched_and_poisoned_output_is_overwritten(dev, M, K, N):
    """y [M, N] sits inside a larger buffer, G guard rows of a sentinel above and below it.  The C ABI's output is packed (row
    stride N), so the guard COLUMNS of a row are its neighbours: a store past column N lands in the next row's first columns --
    a wrong value there, or a changed sentinel behind the last row -- and a store before row 0 / past row M in the guard rows.
    Output memory full of NaN bytes gives the bits of a run on zeroed memory."""
    from rag4dyg_amd import _lib, ops
    G = 3
    x, w, b, r = operands(M, K, N, dev)
    plane = ops.bf16_plane(w)
    for epi, name in ((0, "none"), (1, "gelu"), (2, "residual")):
        want = ops.conv1d_bf16(x, plane, b, name, r if epi == 2 else None)
        outs = []
        for fill in (ZERO, NAN):
            buf = torch.empty((M + 2 * G) * N + 64, dtype=torch.float32, device=dev)
            poison(buf, HUGE)
            y = buf[G * N: (G + M) * N]
            poison(y, fill)
            guard = buf.clone()
            _lib.check(_raw_conv1d_bf16(x, plane, b, r if epi == 2 else None, epi, y.data_ptr(), M, K, N), "conv1d_bf16")
            torch.cuda.synchronize()
            assert torch.equal(buf[:G * N].view(torch.int32), guard[:G * N].view(torch.int32)), (name, fill, "rows above")
            assert torch.equal(buf[(G + M) * N:].view(torch.int32), guard[(G + M) * N:].view(torch.int32)), (name, fill, "rows below")
            outs.append(y.view(M, N).clone())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], want), name


def test_06_bad_shapes_and_a_null_plane_are_refused_without_a_launch(dev):
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    x, w, b, r = operands(16, 64, 64, dev)
    plane = ops.bf16_plane(w)
    y = torch.full((16, 64), 7.0, device=dev)
    before = hits()
    for K in (48, 16, 33):                                               # K % 32 != 0
        rc = _raw_conv1d_bf16(x, plane, b, None, 0, y.data_ptr(), 16, K, 64)
        assert rc == -1 and b"K % 32" in lib.r4d_last_error(), (K, rc, lib.r4d_last_error())
    rc = _raw_conv1d_bf16(x, None, b, None, 0, y.data_ptr(), 16, 64, 64)
    assert rc == -1 and b"null" in lib.r4d_last_error()
    rc = _raw_conv1d_bf16(x, plane, b, None, 2, y.data_ptr(), 16, 64, 64)                    # residual epilogue without a residual
    assert rc == -1 and lib.r4d_last_error() != b""
    rc = _raw_conv1d_bf16(x, plane, b, None, 5, y.data_ptr(), 16, 64, 64)                    # an epilogue this entry does not have
    assert rc == -1 and lib.r4d_last_error() != b""
    with pytest.raises(_lib.R4DError):
        ops.conv1d_bf16(x[:, :48].contiguous(), plane[:, :48].contiguous(), b)
    torch.cuda.synchronize()
    assert hits() == before and bool((y == 7.0).all())                   # nothing was launched, nothing was written


# ------------------------------------------------------------------------------------------------------------ the encoder
def _gpu_tensors(m, ids, dev):
    r = m.transformer.encode(input_ids=ids.to(dev), want_hidden=True, want_meanpool=True, want_layers=True, want_qkv=True)
    out = {"hidden": r["hidden"].cpu(), "meanpool": r["meanpool"].cpu()}
    for l in range(r["layers"].shape[0]):
        out[f"layer{l}"] = r["layers"][l].cpu()
        out[f"qkv{l}"] = r["qkv"][l].cpu()
    return out


@pytest.mark.parametrize("name", R.FIXTURES)
def test_07_encoder_accuracy_against_float64_within_twice_the_emulations(dev, name):
    """``hidden``, ``meanpool``, every layer's residual stream and ``qkv`` under bf16 precision in each of the three gemm modes:
    max|gpu - f64| / max|f64| <= 2 x the same figure of the float32 emulation (two faithful executions of this arithmetic
    differ by flipped bf16 roundings of activations near a rounding boundary: measured 1.00 - 1.11 on the CPU, so a correct
    kernel sits near 1 and a wrong one does not hide under 2).  The kernel that ran is asserted through the branch table."""
    from rag4dyg_amd import ops
    m, ids = model_on(dev, name)
    exact = R.references(name)[0]
    table = R.error_table(name)
    L = R.fixture(name)[1]
    ops.set_encode_precision("bf16")
    for mode in GEMM_MODES:
        ops.set_gemm_mode(mode)
        before = sum(hits().values())
        got = _gpu_tensors(m, ids, dev)
        assert sum(hits().values()) - before == 4 * L, (name, mode)     # the four Conv1D GEMMs of every block, nothing else
        for k, t in got.items():
            e_gpu, e_emu = R.rel(t.view_as(exact[k]), exact[k]), table[k]["emu32"]
            print(f"RATIO {name} {mode} {k} {e_gpu / e_emu:.3f} gpu {e_gpu:.3e} emu32 {e_emu:.3e}")
            assert e_gpu <= 2 * e_emu, (name, mode, k, e_gpu, e_emu)


def test_08_fused_batches_equal_per_batch_calls_bit_for_bit(dev):
    from rag4dyg_amd import ops
    m, _ = model_on(dev, "L2_d256_T130")
    tr = m.transformer
    g = torch.Generator().manual_seed(8)
    batches = [torch.randint(0, 59, s, generator=g).to(dev) for s in ((3, 40), (2, 17), (5, 33), (1, 130))]
    ops.set_encode_precision("bf16")
    for mode in GEMM_MODES:
        ops.set_gemm_mode(mode)
        fused = tr.encode_groups(batches, want_hidden=True, want_qkv=True, want_meanpool=True)
        pooled = tr.encode_groups_meanpool(batches)
        seq0 = 0
        for b_, r0 in zip(batches, fused["row0"]):
            one = tr.encode(input_ids=b_, want_hidden=True, want_meanpool=True, want_qkv=True)
            B, T = b_.shape
            assert torch.equal(fused["hidden"][r0:r0 + B * T], one["hidden"].view(B * T, -1)), mode
            assert torch.equal(fused["qkv"][:, r0:r0 + B * T], one["qkv"].view(one["qkv"].shape[0], B * T, -1)), mode
            assert torch.equal(fused["meanpool"][seq0:seq0 + B], one["meanpool"]) and torch.equal(pooled[seq0:seq0 + B], one["meanpool"]), mode
            seq0 += B


def test_09_inputs_embeds_of_wte_rows_equal_the_ids_form(dev):
    from rag4dyg_amd import ops
    m, ids = model_on(dev, "L2_d64_T40")
    tr = m.transformer
    ops.set_encode_precision("bf16")
    ids = ids.to(dev)
    a = tr.encode(input_ids=ids, want_hidden=True, want_meanpool=True)
    b = tr.encode(inputs_embeds=tr.wte.weight.detach()[ids], want_hidden=True, want_meanpool=True)
    assert torch.equal(a["hidden"], b["hidden"]) and torch.equal(a["meanpool"], b["meanpool"])
    g = tr.encode_groups([tr.wte.weight.detach()[ids]], embeds=True, want_hidden=True)
    assert torch.equal(g["hidden"].view_as(a["hidden"]), a["hidden"])


def _isolated_results(dev):
    """Everything the switch must not touch, computed from seeded inputs: name -> tensor."""
    from rag4dyg_amd import ops, training
    from rag4dyg_amd.lm_training import LMTrainer
    out = {}
    m, ids = model_on(dev, "L2_d64_T40")
    ids = ids[:, :20].contiguous().to(dev)
    enc = training.EncoderTrainer(m)
    emb = enc.forward([ids])
    out["train:embeddings"] = emb.clone()
    for n, t in enc.backward(torch.cos(torch.arange(emb.numel(), device=dev, dtype=torch.float32)).view_as(emb)).items():
        out["train:grad:" + n] = t.clone()
    lm = LMTrainer(m)
    out["lm:loss"] = lm.step(ids).clone()
    for n, t in lm.grads.items():
        out["lm:grad:" + n] = t.clone()
    tr = m.transformer
    g = torch.Generator().manual_seed(10)
    for B in (4, 40):                                                    # 40 rows: the tiled-GEMM fallback of the decode step
        cache = torch.randn(tr.config.n_layer, B, 32, 2 * tr.config.n_embd, generator=g).to(dev)
        pos = torch.full((B,), 20, dtype=torch.int32, device=dev)
        out[f"decode_step:B{B}"] = tr.decode_step(cache, pos, input_ids=torch.randint(0, 59, (B,), generator=g).to(dev)).clone()
        out[f"decode_step:B{B}:cache"] = cache
    x, w, b, r = operands(300, 512, 256, dev)
    out["conv1d"] = ops.conv1d(x, w, b, "gelu", None, w.t().contiguous())
    out["conv1d_s3"] = ops.conv1d_s3(x, ops.split3_planes(w), b, "residual", r)
    out["lm_logits"] = ops.lm_logits(x, torch.randn(70, 512, generator=g).to(dev))
    q, p = ops.normalize_rows(torch.randn(32, 512, generator=g).to(dev)), ops.normalize_rows(torch.randn(700, 512, generator=g).to(dev))
    vals, idx, S = ops.score_topk(q, p, 5, want_scores=True)
    out["score_topk:vals"], out["score_topk:idx"], out["score_topk:scores"] = vals, idx, S
    return out


def test_10_the_switch_leaves_every_other_entry_bit_identical(dev):
    """One EncoderTrainer forward / backward, one LMTrainer.step, decode_step at B = 4 and B = 40, ops.conv1d, ops.conv1d_s3,
    ops.lm_logits and ops.score_topk: the same bits with the switch on as off, and none of them runs the bf16 kernel."""
    from rag4dyg_amd import ops
    ops.set_encode_precision("fp32")
    off = _isolated_results(dev)
    ops.set_encode_precision("bf16")
    before = hits()
    on = _isolated_results(dev)
    assert hits() == before
    assert set(on) == set(off) and len(off) > 30
    for n in off:
        assert torch.equal(on[n], off[n]), n


def test_11_switching_off_returns_to_the_bits_from_before(dev):
    from rag4dyg_amd import ops
    m, ids = model_on(dev, "L2_d256_T130")
    ids = ids.to(dev)
    for mode in GEMM_MODES:
        ops.set_gemm_mode(mode)
        assert ops.set_encode_precision("fp32") in ("fp32", "bf16")
        h0 = m.transformer.encode(input_ids=ids, want_hidden=True, want_meanpool=True)
        assert ops.set_encode_precision("bf16") == "fp32"
        h1 = m.transformer.encode(input_ids=ids, want_hidden=True, want_meanpool=True)
        assert ops.set_encode_precision("fp32") == "bf16"
        h2 = m.transformer.encode(input_ids=ids, want_hidden=True, want_meanpool=True)
        assert not torch.equal(h0["hidden"], h1["hidden"]), mode           # the switch did switch the arithmetic
        assert torch.equal(h0["hidden"], h2["hidden"]) and torch.equal(h0["meanpool"], h2["meanpool"]), mode


class _EosOnly:
    def encode(self, text):
        assert text == "<|endoftext|>"
        return [R.EOS_ID]


def test_12_greedy_decoding_prefills_in_bf16_and_steps_in_fp32(dev):
    """``greedy_decode_batch`` on the g10 trained weights, 8 seeded prompts of lengths 5 .. 48, val mode, against the emulated
    greedy loop whose patched ``conv1d`` rounds only the rows of prompt positions.  A first difference must be a tie of the
    float64 emulation's logits within 2 x the emulation's measured logits error on this fixture; at least 6 of the 8 sequences
    are identical outright.  (tests/test_host_encode_bf16.py checks that the float32 and float64 emulations agree on all 8.)"""
    from rag4dyg_amd import ops
    from rag4dyg_amd.evaluation import greedy_decode_batch
    m, _ = model_on(dev, "g10_trained")
    sd, L, H = R.fixture("g10_trained")[:3]
    prompts = R.greedy_prompts()
    rel_gap = 2 * R.error_table("g10_trained")["logits"]["emu32"]
    ops.set_encode_precision("bf16")
    before = sum(hits().values())
    many = greedy_decode_batch(m, _EosOnly(), prompts, "val", R.fixture("g10_trained")[5], 0, dev)
    assert sum(hits().values()) > before                                  # the prefill ran on the bf16 kernel
    exact = 0
    for p, got in zip(prompts, many):
        assert got[:len(p)] == p
        want = R.emulated_greedy(sd, H, p, torch.float64)
        exact += assert_tokens_equal_or_tie(got[len(p):], want, R.emulated_logits_at(sd, H, p), f"bf16 greedy, prompt of {len(p)}", rel_gap)
    print(f"bf16 greedy decoding: {exact} of {len(prompts)} sequences identical to the float64 emulation (rel_gap {rel_gap:.2e})")
    assert exact >= 6, exact


def test_13_every_encode_bf16_dispatcher_branch_is_exercised(dev):
    """What tests/test_gpu_dispatch.py does for the branches its matrix reaches, for the ``tuning:encode_bf16:`` ones (reachable
    through the process-wide switch only): drive each through the ENCODER under the switch and through the single op, then
    enumerate the library's own table."""
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    names = [lib.r4d_dispatch_branch_name(i).decode() for i in range(lib.r4d_dispatch_num_branches())]
    idx = {n: i for i, n in enumerate(names) if n.startswith(BRANCH_PREFIX)}
    assert len(idx) >= 2, names
    start = {n: int(lib.r4d_dispatch_branch_hits(i)) for n, i in idx.items()}
    ops.set_encode_precision("bf16")
    m, ids = model_on(dev, "L2_d256_T130")                                # 390 rows: the 128 x 128 tile
    m.transformer.encode(input_ids=ids.to(dev), want_meanpool=True, want_hidden=False)
    after_small = {n: int(lib.r4d_dispatch_branch_hits(i)) for n, i in idx.items()}
    big = torch.randint(0, 59, (40, 130), generator=torch.Generator().manual_seed(13)).to(dev)      # 5200 rows: c_fc (1024 columns) takes 128 x 256
    m.transformer.encode(input_ids=big, want_meanpool=True, want_hidden=False)
    for (M, K, N) in ((300, 64, 200), (4096, 64, 1536)):
        assert max(check_op(M, K, N, dev)) <= 1.0
    end = {n: int(lib.r4d_dispatch_branch_hits(i)) for n, i in idx.items()}
    print("encode_bf16 branches:", {n: end[n] - start[n] for n in idx})
    assert sum(after_small.values()) - sum(start.values()) == 8           # 2 layers x 4 GEMMs
    missed = sorted(n for n in idx if end[n] == start[n])
    assert not missed, f"encode_bf16 branches no call reached: {missed}"
