"""The encoder's ``"bf16+attn"`` precision on the GPU (``ops.set_encode_precision("bf16+attn")``, ``r4d_set_encode_attention_bf16``,
``r4d_attention_bf16_groups``, csrc/attention_b1.hip): the kernel alone on planted logits against float64 of the bf16-rounded
inputs at a derived bound, its independence of the launch it travels in, the identity of its fp32 / bf16 routes; the encoder under
the word against "the emulation" (tests/_encode_bf16_attn_ref.py); and the isolation of everything the word must not touch.

Every test restores the precision word, the gemm mode and the training switches it found."""
import math

import pytest
import torch

import _attention_ref as AR
import _encode_bf16_attn_ref as E
import _encode_bf16_ref as R
import _train_modes
import test_gpu_encode_bf16 as T16
from _poison import NAN, ZERO, poison, poisoned_allocations
from conftest import GEMM_MODES, assert_tokens_equal_or_tie, load_state_dict_checked

pytestmark = pytest.mark.gpu

PREFIX = "tuning:encode_bf16_attn:"
BR_BF16, BR_F32, BR_FALLBACK = PREFIX + "bf16 qkv", PREFIX + "fp32 qkv, rounded while staged", PREFIX + "fallback to the exact-f32 attention"
HEAD_DIMS = (16, 64, 96, 128, 256)
SENTINEL = -7777.25


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


restore_switches = _train_modes.switches_restored(ops_too=True)


def hits():
    return T16.hits(PREFIX)


def model_on(dev, name, lm=True):
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModel
    sd, L, H, d, V, P, ids = E.fixture(name)
    m = GPT2LMHeadModel(GPT2Config(vocab_size=V, n_positions=P, n_ctx=P, n_embd=d, n_layer=L, n_head=H))
    load_state_dict_checked(m, {k: v for k, v in sd.items() if k != "lm_head.weight"})
    m.tie_weights()
    return m.to(dev).eval(), ids


def seeded_model(dev, L, H, d, V=60, P=160, seed=77):
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModel
    sd = R.gpt2_ref.make_state_dict(L, d, V, n_positions=P, seed=seed, random_affine=True)
    m = GPT2LMHeadModel(GPT2Config(vocab_size=V, n_positions=P, n_ctx=P, n_embd=d, n_layer=L, n_head=H))
    load_state_dict_checked(m, {k: v for k, v in sd.items() if k != "lm_head.weight"})
    m.tie_weights()
    return m.to(dev).eval()


def bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


# ------------------------------------------------------------------------------------------------------------ the kernel alone
def planted_T(hd):
    """T on both sides of the 32-key tile and of the kernel's 128-query tile; at head_dim 256 also a third query tile"""
    return (1, 31, 32, 33, 127, 128, 129) + ((257,) if hd == 256 else ())


def reference64(qkv, H):
    """float64 causal attention of the bf16-ROUNDED q, k, v of ``qkv`` [B, T, 3d] -> (O [B, T, d], the per-element bound).

    The bound, term by term (that of tests/test_gpu_train_attention_fused.py::test_02 for the same arithmetic):
      2^-8      the probabilities enter P . V rounded to bf16 once (2^-9 relative each); the device rounds BEFORE the normalisation,
                which grants the factor 2;
      2 s_floor the logits carry their fp32 accumulation error s_floor = (hd + 2) 2^-24 max|q| . |k|^T / sqrt(hd), which moves a
                probability by at most 2 s_floor relative (its own exponent and the row sum's);
      2^-13     the fast exponential's argument rounding and the fp32 sums over up to 1024 terms;
    all times sum_j P_ij |v_j|, the size of what the probabilities multiply (the fp32 accumulation of O itself, (T + 2) 2^-24 of
    the same sum, is inside the 2^-13)."""
    B, T, d3 = qkv.shape
    d, hd = d3 // 3, d3 // 3 // H

    def heads(x):
        return x.bfloat16().double().view(B, T, H, hd).permute(0, 2, 1, 3)
    q, k, v = (heads(x) for x in qkv.split(d, dim=2))
    s = (q @ k.transpose(-1, -2) / math.sqrt(hd)).masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool, device=qkv.device)), float("-inf"))
    P = torch.softmax(s, dim=-1)
    s_floor = (hd + 2) * 2.0 ** -24 * float((q.abs() @ k.abs().transpose(-1, -2)).max()) / math.sqrt(hd)
    bound = (2.0 ** -8 + 2.0 * s_floor + 2.0 ** -13) * (P @ v.abs())
    merge = lambda x: x.permute(0, 2, 1, 3).reshape(B, T, d)
    return merge(P @ v), merge(bound)


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_01_kernel_on_planted_logits_against_float64_of_the_rounded_inputs(dev, hd):
    """spike / up / down / dead / wide / flat (tests/_attention_ref.plant) at B x H = 2 x 2: O of the kernel (fp32 qkv in, fp32 out:
    nothing but the kernel's own roundings) against float64 attention of the bf16-rounded q, k, v, element by element at
    ``reference64``'s bound.  A missing rescale, a wrong mask or a dropped tile moves these cases by orders of magnitude more."""
    from rag4dyg_amd import ops
    B, H = 2, 2
    before = hits()
    for T in planted_T(hd):
        for pattern in ("spike", "up", "down", "dead", "wide", "flat"):
            g = torch.Generator().manual_seed(1000 * T + 7 * hd + AR.PATTERNS.index(pattern))
            qkv = AR.plant(B, T, H, hd, pattern, g).to(dev)
            want, bound = reference64(qkv, H)
            got = ops.attention_bf16(qkv.view(B * T, -1), [(B, T)], H).view(B, T, H * hd).double()
            assert torch.isfinite(got).all(), (pattern, T, hd)
            worst = float(((got - want).abs() / bound.clamp_min(1e-300)).max())
            print(f"[encode bf16+attn] planted {pattern} T{T} hd{hd}: largest |error| / bound {worst:.3f}")
            assert worst <= 1.0, (pattern, T, hd, worst)
            if pattern == "flat":                                          # the plain mean: column 0 = 1, column 1 = i / 2
                i = torch.arange(T, dtype=torch.float64, device=dev).view(1, T, 1)
                o = got.view(B, T, H, hd)
                assert float((o[..., 0] - 1.0).abs().max()) <= 2.0 ** -8
                assert float(((o[..., 1] - i / 2).abs() / (i / 2 + 1)).max()) <= 2.0 ** -8
    assert hits()[BR_F32] > before[BR_F32]


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_02_a_sequence_does_not_depend_on_the_launch_it_travels_in(dev, hd):
    """The same (sequence, head)s -- one batch (2, T) -- give the same bits alone, in a launch with batches of other T before and
    after them, and with every byte of qkv that is not their own rows set to NaN or to 3e38; and twice in a row.  fp32 and bf16 qkv."""
    from rag4dyg_amd import ops
    H = 2
    d = H * hd
    for T in (33, 129):
        groups = [(3, 40), (1, 1), (2, T), (2, 130), (1, 31)]
        rows = [b * t for b, t in groups]
        lo = sum(rows[:2])
        g = torch.Generator().manual_seed(11 * T + hd)
        full = torch.randn(sum(rows), 3 * d, generator=g).to(dev)
        for dtype in (torch.float32, torch.bfloat16):
            x = full.to(dtype)
            own = x[lo:lo + 2 * T].contiguous()
            alone = ops.attention_bf16(own, [(2, T)], H)
            assert torch.equal(bits(alone), bits(ops.attention_bf16(own, [(2, T)], H))), (hd, T, dtype, "two launches")
            among = ops.attention_bf16(x, groups, H)
            assert torch.equal(bits(among[lo:lo + 2 * T]), bits(alone)), (hd, T, dtype, "among other batches")
            for fill in (float("nan"), 3e38):
                y = torch.full_like(x, fill)
                y[lo:lo + 2 * T] = own
                got = ops.attention_bf16(y, groups, H)[lo:lo + 2 * T]
                assert torch.equal(bits(got), bits(alone)), (hd, T, dtype, fill)
            # one sequence of the batch alone: its neighbour in the SAME batch does not matter either
            assert torch.equal(bits(ops.attention_bf16(own[T:].contiguous(), [(1, T)], H)), bits(alone[T:])), (hd, T, dtype, "second sequence")


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_03a_fp32_and_bf16_routes_of_the_kernel_agree_after_the_one_rounding(dev, hd):
    """fp32 qkv -> fp32 O and RN(qkv) as bf16 -> bf16 O: the same values rounded once by the same rule either way, so RN(fp32 O)
    has the bf16 O's bits; the mixed forms (fp32 -> bf16, bf16 -> fp32) agree with them too."""
    from rag4dyg_amd import ops
    H = 2
    groups = [(2, 70), (1, 129), (3, 17)]
    g = torch.Generator().manual_seed(hd)
    qkv = (torch.randn(sum(b * t for b, t in groups), 3 * H * hd, generator=g) * 1.5).to(dev)
    before = hits()
    o32 = ops.attention_bf16(qkv, groups, H)
    obf = ops.attention_bf16(qkv.bfloat16(), groups, H)
    assert o32.dtype == torch.float32 and obf.dtype == torch.bfloat16
    assert torch.equal(bits(o32.bfloat16()), bits(obf))
    assert torch.equal(bits(ops.attention_bf16(qkv, groups, H, out_bf16=True)), bits(obf))
    assert torch.equal(bits(ops.attention_bf16(qkv.bfloat16(), groups, H, out_bf16=False)), bits(o32))
    after = hits()
    assert after[BR_F32] - before[BR_F32] == 2 and after[BR_BF16] - before[BR_BF16] == 2


@pytest.mark.parametrize("name", ("L2_d64_T40", "L2_hd96_T45", "L4_d512_T96"))
def test_03b_encoder_routes_agree_and_layer0_qkv_is_the_bf16_words(dev, name):
    """``encode(..., want_qkv=True)`` (c_attn writes fp32, the attention rounds while staging) and ``encode(...)`` (c_attn writes
    bf16) return the same hidden and mean-pool bits under the word; layer 0's qkv under it equals layer 0's under ``"bf16"``."""
    from rag4dyg_amd import ops
    m, ids = model_on(dev, name)
    ids = ids.to(dev)
    L = E.fixture(name)[1]
    for mode in GEMM_MODES:
        ops.set_gemm_mode(mode)
        ops.set_encode_precision("bf16")
        q16 = m.transformer.encode(input_ids=ids, want_hidden=True, want_meanpool=True, want_qkv=True)
        ops.set_encode_precision(E.WORD)
        before = hits()
        a = m.transformer.encode(input_ids=ids, want_hidden=True, want_meanpool=True, want_qkv=True)
        mid = hits()
        b = m.transformer.encode(input_ids=ids, want_hidden=True, want_meanpool=True)
        after = hits()
        assert mid[BR_F32] - before[BR_F32] == L and mid[BR_BF16] == before[BR_BF16], (name, mode)
        assert after[BR_BF16] - mid[BR_BF16] == L and after[BR_F32] == mid[BR_F32] and after[BR_FALLBACK] == before[BR_FALLBACK], (name, mode)
        assert torch.equal(a["hidden"], b["hidden"]) and torch.equal(a["meanpool"], b["meanpool"]), (name, mode)
        assert torch.equal(a["qkv"][0], q16["qkv"][0]), (name, mode)
        assert not torch.equal(a["qkv"][1], q16["qkv"][1]) and not torch.equal(a["hidden"], q16["hidden"]), (name, mode)   # the word did switch the attention


# ------------------------------------------------------------------------------------------------------------ the encoder
@pytest.mark.parametrize("name", E.FIXTURES)
def test_04_encoder_accuracy_against_float64_within_twice_the_emulations(dev, name):
    """Every gated tensor (``E.gated``: at least hidden, meanpool and the qkv of every layer behind an attention) under the word in
    each of the three gemm modes: max|gpu - f64| / max|f64| <= 2 x the same figure of the float32 emulation -- the gate and the
    factor tests/test_gpu_encode_bf16.py::test_07 uses for ``"bf16"``."""
    from rag4dyg_amd import ops
    m, ids = model_on(dev, name)
    exact = E.references(name)[0]
    table = E.error_table(name)
    L = E.fixture(name)[1]
    returned = {"hidden", "meanpool"} | {f"layer{l}" for l in range(L)} | {f"qkv{l}" for l in range(L)}      # (logits: the LM head is not the encoder's)
    gated = [k for k in E.gated(name) if k in returned]
    assert set(E.must_gate(name)) <= set(gated)
    ops.set_encode_precision(E.WORD)
    for mode in GEMM_MODES:
        ops.set_gemm_mode(mode)
        before = hits()
        got = T16._gpu_tensors(m, ids, dev)
        after = hits()
        assert after[BR_F32] - before[BR_F32] == L and after[BR_FALLBACK] == before[BR_FALLBACK], (name, mode)
        bad = {}
        for k in gated:
            e_gpu, e_emu = R.rel(got[k].view_as(exact[k]), exact[k]), table[k]["emu32"]
            print(f"RATIO {name} {mode} {k} {e_gpu / e_emu:.3f} gpu {e_gpu:.3e} emu32 {e_emu:.3e}")
            if not e_gpu <= 2 * e_emu:
                bad[k] = (e_gpu, e_emu)
        assert not bad, (name, mode, bad)


def test_05_fused_batches_equal_per_batch_calls_bit_for_bit(dev):
    from rag4dyg_amd import ops
    m, _ = model_on(dev, "L2_d256_T130")
    tr = m.transformer
    g = torch.Generator().manual_seed(8)
    batches = [torch.randint(0, 59, s, generator=g).to(dev) for s in ((3, 40), (2, 17), (5, 33), (1, 130))]
    ops.set_encode_precision(E.WORD)
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


def test_06_the_word_leaves_every_other_entry_bit_identical_and_switching_back_restores(dev):
    """One EncoderTrainer forward / backward, one LMTrainer.step, decode_step at B = 4 and B = 40, ops.conv1d, ops.conv1d_s3,
    ops.lm_logits and ops.score_topk (tests/test_gpu_encode_bf16.py::_isolated_results): the same bits under the word as under
    ``"fp32"``, none of them on the new kernel; going back to ``"bf16"`` and to ``"fp32"`` restores the encoder's bits from before."""
    from rag4dyg_amd import ops
    ops.set_encode_precision("fp32")
    off = T16._isolated_results(dev)
    ops.set_encode_precision(E.WORD)
    before, before16 = hits(), T16.hits()
    on = T16._isolated_results(dev)
    assert hits() == before and T16.hits() == before16
    assert set(on) == set(off) and len(off) > 30
    for n in off:
        assert torch.equal(on[n], off[n]), n
    m, ids = model_on(dev, "L2_d256_T130")
    ids = ids.to(dev)
    enc = lambda: m.transformer.encode(input_ids=ids, want_hidden=True, want_meanpool=True)
    for mode in GEMM_MODES:
        ops.set_gemm_mode(mode)
        ops.set_encode_precision("fp32")
        h32 = enc()
        assert ops.set_encode_precision("bf16") == "fp32"
        h16 = enc()
        assert ops.set_encode_precision(E.WORD) == "bf16"
        hat = enc()
        assert ops.set_encode_precision("bf16") == E.WORD
        h16b = enc()
        assert ops.set_encode_precision("fp32") == "bf16"
        h32b = enc()
        assert not torch.equal(hat["hidden"], h16["hidden"]) and not torch.equal(hat["hidden"], h32["hidden"]), mode
        assert torch.equal(h16["hidden"], h16b["hidden"]) and torch.equal(h16["meanpool"], h16b["meanpool"]), mode
        assert torch.equal(h32["hidden"], h32b["hidden"]) and torch.equal(h32["meanpool"], h32b["meanpool"]), mode


class _EosOnly:
    def encode(self, text):
        assert text == "<|endoftext|>"
        return [E.EOS_ID]


def test_07_greedy_decoding_prefills_under_the_word_and_steps_in_fp32(dev):
    """``greedy_decode_batch`` on the g10 trained weights, the 8 seeded prompts, val mode, against the emulated greedy loop (a
    bf16+attn prefill of the prompt rows, exact steps).  A first difference must be a tie of the float64 emulation's logits within
    2 x the emulation's measured logits error on this fixture; at least 6 of the 8 sequences are identical outright."""
    from rag4dyg_amd import ops
    from rag4dyg_amd.evaluation import greedy_decode_batch
    m, _ = model_on(dev, "g10_trained")
    sd, L, H = E.fixture("g10_trained")[:3]
    prompts = E.greedy_prompts()
    rel_gap = 2 * E.error_table("g10_trained")["logits"]["emu32"]
    ops.set_encode_precision(E.WORD)
    before = hits()
    many = greedy_decode_batch(m, _EosOnly(), prompts, "val", E.fixture("g10_trained")[5], 0, dev)
    after = hits()
    assert sum(after.values()) > sum(before.values()) and after[BR_FALLBACK] == before[BR_FALLBACK]      # the prefill ran on the new kernel
    exact = 0
    for p, got in zip(prompts, many):
        assert got[:len(p)] == p
        want = E.emulated_greedy(sd, H, p, torch.float64)
        exact += assert_tokens_equal_or_tie(got[len(p):], want, E.emulated_logits_at(sd, H, p), f"bf16+attn greedy, prompt of {len(p)}", rel_gap)
    print(f"bf16+attn greedy decoding: {exact} of {len(prompts)} sequences identical to the float64 emulation (rel_gap {rel_gap:.2e})")
    assert exact >= 6, exact


# ------------------------------------------------------------------------------------------------------------ refusals, fallback
def _raw(qkv, in_bf16, groups, r0, H, d, out, out_bf16, n=None):
    import ctypes
    from rag4dyg_amd import _lib
    k = len(groups)
    Bs = (ctypes.c_int32 * max(k, 1))(*[b for b, _ in groups])
    Ts = (ctypes.c_int32 * max(k, 1))(*[t for _, t in groups])
    rs = (ctypes.c_int64 * max(k, 1))(*r0)
    return _lib.load().r4d_attention_bf16_groups(qkv, int(in_bf16), k if n is None else n, Bs, Ts, rs, H, d, out, int(out_bf16),
                                                 torch.cuda.current_stream().cuda_stream)


def test_08a_bad_shapes_of_the_single_op_are_refused_before_any_launch(dev):
    from rag4dyg_amd import _lib
    lib = _lib.load()
    qkv = torch.randn(64, 3 * 128, device=dev)
    out = torch.full((64, 128), SENTINEL, device=dev)
    before = hits()
    q, o = qkv.data_ptr(), out.data_ptr()
    cases = {"head_dim 24": ([(2, 16)], [0], 2, 48), "head_dim 8": ([(2, 16)], [0], 16, 128), "head_dim 272": ([(1, 16)], [0], 1, 272),
             "d not a multiple of H": ([(2, 16)], [0], 3, 128), "H = 0": ([(2, 16)], [0], 0, 128), "T = 0": ([(2, 0)], [0], 2, 128),
             "T = 1025": ([(1, 1025)], [0], 2, 128), "B = 0": ([(0, 16)], [0], 2, 128), "negative row": ([(2, 16)], [-32], 2, 128),
             "second batch empty": ([(1, 16), (0, 16)], [0, 16], 2, 128)}
    for what, (groups, r0, H, d) in cases.items():
        for in_bf16 in (0, 1):
            rc = _raw(q, in_bf16, groups, r0, H, d, o, 0)
            assert rc == -1 and lib.r4d_last_error() != b"", (what, rc)
    assert _raw(q, 0, [(2, 16)], [0], 2, 128, o, 0, n=0) == -1 and _raw(q, 0, [(1, 1)] * 16, [0] * 16, 2, 128, o, 0, n=17) == -1
    assert _raw(None, 0, [(2, 16)], [0], 2, 128, o, 0) == -1 and b"null" in lib.r4d_last_error()
    assert _raw(q, 0, [(2, 16)], [0], 2, 128, None, 0) == -1 and b"null" in lib.r4d_last_error()
    assert _raw(q + 4, 0, [(2, 16)], [0], 2, 128, o, 0) == -1 and b"aligned" in lib.r4d_last_error()
    assert _raw(q, 0, [(2, 16)], [0], 2, 128, o + 8, 1) == -1 and b"aligned" in lib.r4d_last_error()
    torch.cuda.synchronize()
    assert hits() == before and bool((out == SENTINEL).all())             # nothing was launched, nothing was written
    assert _raw(q, 0, [(2, 16)], [0], 2, 128, o, 0) == 0                   # ... and the good call next to them is taken
    torch.cuda.synchronize()
    assert bool((out[:32] != SENTINEL).all()) and bool((out[32:] == SENTINEL).all())


def test_08b_shapes_the_kernel_does_not_serve_take_the_bf16_words_route(dev):
    """Through the encoder.  The encoder entries refuse a head dim that is no multiple of 16 under EVERY word (``gpt2: head_dim ...
    must be a multiple of 16``: head dim 24 never reaches a routing decision), and more than 65,535 sequences in one launch
    likewise (the final LayerNorm + mean-pool launch has the same grid limit); both are asserted as what they are.  The limit that
    does reach the routing is a head dim above 256 (320 = one head of d 320): the bits of ``"bf16"``, the fallback branch counted
    once per layer."""
    from rag4dyg_amd import _lib, ops
    g = torch.Generator().manual_seed(2)
    m24 = seeded_model(dev, 1, 8, 192)
    ids24 = torch.randint(0, 59, (2, 9), generator=g).to(dev)
    many = seeded_model(dev, 1, 2, 64)
    two = [torch.randint(0, 59, (40000, 1), generator=g).to(dev), torch.randint(0, 59, (30000, 1), generator=g).to(dev)]
    for word in ("fp32", "bf16", E.WORD):
        ops.set_encode_precision(word)
        before = hits()
        with pytest.raises(_lib.R4DError, match="multiple of 16"):
            m24.transformer.encode(input_ids=ids24, want_hidden=True)
        with pytest.raises(_lib.R4DError, match="sequences per launch"):
            many.transformer.encode_groups(two, want_hidden=True, want_meanpool=True)
        assert hits()[BR_BF16] == before[BR_BF16] and hits()[BR_F32] == before[BR_F32]
    torch.cuda.synchronize()
    wide = seeded_model(dev, 2, 1, 320)
    for batches in ([torch.randint(0, 59, (3, 37), generator=g).to(dev)],
                    [torch.randint(0, 59, s, generator=g).to(dev) for s in ((2, 33), (1, 129), (4, 5))]):
        ops.set_encode_precision("bf16")
        want = wide.transformer.encode_groups(batches, want_hidden=True, want_meanpool=True)
        ops.set_encode_precision(E.WORD)
        before = hits()
        got = wide.transformer.encode_groups(batches, want_hidden=True, want_meanpool=True)
        after = hits()
        assert after[BR_FALLBACK] - before[BR_FALLBACK] == 2 and after[BR_BF16] == before[BR_BF16] and after[BR_F32] == before[BR_F32]
        assert torch.equal(got["hidden"], want["hidden"]) and torch.equal(got["meanpool"], want["meanpool"])
        assert bool(torch.isfinite(got["hidden"]).all())


def test_08c_every_encode_bf16_attn_dispatcher_branch_is_exercised(dev):
    """What tests/test_gpu_dispatch.py does for the branches its matrix reaches, for the ``tuning:encode_bf16_attn:`` ones (reachable
    through the process-wide word only): drive each through the encoder, then enumerate the library's own table."""
    from rag4dyg_amd import ops
    start = hits()
    assert set(start) == {BR_BF16, BR_F32, BR_FALLBACK}
    ops.set_encode_precision(E.WORD)
    m, ids = model_on(dev, "L2_d64_T40")
    m.transformer.encode(input_ids=ids.to(dev), want_meanpool=True, want_hidden=False)
    m.transformer.encode(input_ids=ids.to(dev), want_meanpool=True, want_hidden=False, want_qkv=True)
    seeded_model(dev, 1, 1, 320).transformer.encode(input_ids=ids.to(dev), want_meanpool=True, want_hidden=False)
    end = hits()
    print("encode_bf16_attn branches:", {n: end[n] - start[n] for n in end})
    assert {n: end[n] - start[n] for n in end} == {BR_BF16: 2, BR_F32: 2, BR_FALLBACK: 1}


# ------------------------------------------------------------------------------------------------------------ poisoned buffers
@pytest.mark.parametrize("hd", (16, 96, 256))
def test_09a_the_kernel_writes_the_valid_rows_own_columns_and_nothing_else(dev, hd):
    """Output memory full of NaN bytes gives the bits of a run on zeroed memory; guard rows above, between and below the batches'
    rows keep their sentinel, in the fp32 and in the bf16 output."""
    from rag4dyg_amd import _lib
    H, G = 2, 5
    d = H * hd
    groups, r0 = [(2, 33), (1, 129)], [G, G + 66 + G]                      # guard rows before, between and behind the two batches
    rows = G + 66 + G + 129 + G
    qkv = torch.randn(rows, 3 * d, generator=torch.Generator().manual_seed(hd)).to(dev)
    valid = torch.zeros(rows, dtype=torch.bool, device=dev)
    valid[G:G + 66] = True
    valid[G + 66 + G:G + 66 + G + 129] = True
    for in_dtype in (torch.float32, torch.bfloat16):
        x = qkv.to(in_dtype)
        for out_dtype in (torch.float32, torch.bfloat16):
            outs = []
            for fill in (ZERO, NAN):
                out = torch.empty(rows, d, dtype=out_dtype, device=dev)
                poison(out, fill)
                guard = out.clone()
                _lib.check(_raw(x.data_ptr(), in_dtype == torch.bfloat16, groups, r0, H, d, out.data_ptr(), out_dtype == torch.bfloat16), "attention_bf16")
                torch.cuda.synchronize()
                assert torch.equal(bits(out[~valid]), bits(guard[~valid])), (hd, in_dtype, out_dtype, fill, "guard rows")
                outs.append(out[valid].clone())
            assert torch.equal(bits(outs[0]), bits(outs[1])) and bool(torch.isfinite(outs[0].float()).all()), (hd, in_dtype, out_dtype)


@pytest.mark.parametrize("name", ("L2_hd64_T70", "L4_d512_T96"))
def test_09b_encoder_under_the_word_does_not_read_unwritten_memory(dev, name):
    """The workspace and the outputs filled with NaN bytes before the call -- on first allocation and on reuse (tests/_poison.py) --
    give the bits of a zeroed workspace: the bf16 q | k | v and attention-output images live in the fp32 buffers' first halves, and
    nothing reads the halves behind them."""
    from rag4dyg_amd import ops
    m, ids = model_on(dev, name)
    ids = ids.to(dev)
    ops.set_encode_precision(E.WORD)
    batches = [ids, ids[:2, :33].contiguous()]

    def run(pattern):
        out = []
        ops._WS.clear()
        for k in range(2):
            if k:
                for b in list(ops._WS.values()):
                    poison(b, pattern)
            with poisoned_allocations(pattern):
                a = m.transformer.encode(input_ids=ids, want_hidden=True, want_meanpool=True)
                b = m.transformer.encode(input_ids=ids, want_hidden=True, want_meanpool=True, want_qkv=True)
                c = m.transformer.encode_groups(batches, want_hidden=True, want_meanpool=True)
            out.append({"hidden": a["hidden"].clone(), "meanpool": a["meanpool"].clone(), "hidden_q": b["hidden"].clone(), "qkv": b["qkv"].clone(),
                        "groups_hidden": c["hidden"].clone(), "groups_meanpool": c["meanpool"].clone()})
        return out
    for mode in GEMM_MODES:
        ops.set_gemm_mode(mode)
        base = run(ZERO)
        got = run(NAN)
        for k in range(2):
            assert all(bool(torch.isfinite(v).all()) for v in base[k].values()), (name, mode)
            for n in base[k]:
                assert torch.equal(bits(base[k][n]), bits(got[k][n])), (name, mode, k, n)
