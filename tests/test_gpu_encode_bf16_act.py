"""The bf16 encoder's activation store on the GPU (``ops.set_encode_act_store("bf16")``, ``r4d_set_encode_act_bf16``): under the
precision words ``"bf16"`` and ``"bf16+attn"`` a block's ln1, ln2 and GELU output are rounded once where they are produced and read
as the bf16 A operand of csrc/gemm_b1.hip.  The rounding is the one that kernel applies while staging the fp32 form, so the
reference of EVERY comparison here is the same word with the store off, in the same process, and the comparison is ``torch.equal``:
no tolerance anywhere.  Which buffers really were bf16 is read from the ``tuning:encode_act_bf16:`` dispatch counters.

Every test restores the store, the precision word, the gemm mode and the training switches it found."""
import pytest
import torch

import _encode_bf16_ref as R
import _train_modes
import test_gpu_encode_bf16 as T16
import test_gpu_generator_training as GT
from _poison import HUGE, NAN, ONE, ZERO, poison, poisoned_allocations
from conftest import GEMM_MODES, load_state_dict_checked

pytestmark = pytest.mark.gpu

PREFIX = "tuning:encode_act_bf16:"
LN1, LN2, F, KEPT = PREFIX + "ln1", PREFIX + "ln2", PREFIX + "f", PREFIX + "kept fp32"
WORDS = ("bf16", "bf16+attn")
SHAPES = ((1, 5), (3, 37), (1, 128), (1, 129))                            # M = 5, 111, 128, 129: each side of the 128-row tile edge
RAGGED = ((2, 33), (3, 70), (1, 1))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


restore_switches = _train_modes.switches_restored(ops_too=True)


@pytest.fixture(autouse=True)
def restore_store(dev):
    from rag4dyg_amd import ops
    was = ops.encode_act_store()
    yield
    ops.set_encode_act_store(was)


def hits():
    return T16.hits(PREFIX)


def delta(before):
    now = hits()
    return {k: now[k] - before[k] for k in now}


def counted(ln1=0, ln2=0, f=0, kept=0):
    return {LN1: ln1, LN2: ln2, F: f, KEPT: kept}


def bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def same(a, b):
    """Two results of one call -- a tensor, None, or a dict / list / tuple of them -- bit for bit"""
    if isinstance(a, dict):
        return set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))
    return a == b


def clone(r):
    if isinstance(r, dict):
        return {k: clone(v) for k, v in r.items()}
    if isinstance(r, (list, tuple)):
        return [clone(v) for v in r]
    return r.clone() if isinstance(r, torch.Tensor) else r


def off_on(call):
    """``call()`` with the store off, then on -> (off's result, on's result, the counters' advance during the ON call)"""
    from rag4dyg_amd import ops
    ops.set_encode_act_store("fp32")
    before = hits()
    want = clone(call())
    assert delta(before) == counted(), "the store is off: no counter may move"
    ops.set_encode_act_store("bf16")
    before = hits()
    got = clone(call())
    return want, got, delta(before)


def seeded_model(dev, L, H, d, V=60, P=160, seed=77):
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModel
    sd = R.gpt2_ref.make_state_dict(L, d, V, n_positions=P, seed=seed, random_affine=True)
    m = GPT2LMHeadModel(GPT2Config(vocab_size=V, n_positions=P, n_ctx=P, n_embd=d, n_layer=L, n_head=H))
    load_state_dict_checked(m, {k: v for k, v in sd.items() if k != "lm_head.weight"})
    m.tie_weights()
    return m.to(dev).eval()


# (d 256, 512, 768, 1280: one, two, three and five 256-wide quads per row -- every instantiation of the bf16 LayerNorm stores,
#  with an even and an odd last pair)
MODELS = {"L2_d256_T130": None, "L4_d512_T96": None, "L2_d768_H8": (2, 8, 768), "L1_d1280_H5": (1, 5, 1280)}


def model_of(dev, name):
    """-> (model, L, d); vocabulary 60 and 160 positions in all of them"""
    if MODELS[name] is None:
        m, _ids = T16.model_on(dev, name)
        return m, R.fixture(name)[1], R.fixture(name)[3]
    L, H, d = MODELS[name]
    return seeded_model(dev, L, H, d), L, d


def encoder_calls(m, dev, d, seed):
    """name -> thunk: every way into the encoder the store applies to, at the row counts of ``SHAPES``, the ragged groups and
    ``inputs_embeds``"""
    tr = m.transformer
    g = torch.Generator().manual_seed(seed)
    calls = {}
    for B, T in SHAPES:
        ids = torch.randint(0, 59, (B, T), generator=g).to(dev)
        calls[f"encode {B}x{T} +qkv"] = lambda ids=ids: tr.encode(input_ids=ids, want_hidden=True, want_meanpool=True, want_qkv=True, want_layers=True)
        calls[f"encode {B}x{T}"] = lambda ids=ids: tr.encode(input_ids=ids, want_hidden=True, want_meanpool=True)

        def prefill(ids=ids, B=B, T=T):
            cache = tr.new_kv_cache(B, T + 3, dev).zero_()
            return {"hidden": tr.prefill(cache, input_ids=ids), "cache": cache}
        calls[f"prefill {B}x{T}"] = prefill
    ragged = [torch.randint(0, 59, s, generator=g).to(dev) for s in RAGGED]
    calls["groups +qkv"] = lambda: tr.encode_groups(ragged, want_hidden=True, want_qkv=True, want_meanpool=True)
    calls["groups"] = lambda: tr.encode_groups(ragged, want_hidden=True, want_meanpool=True)
    calls["groups meanpool"] = lambda: tr.encode_groups_meanpool(ragged)
    emb = (torch.randn(2, 37, d, generator=g) * 0.1).to(dev)
    calls["inputs_embeds"] = lambda: tr.encode(inputs_embeds=emb, want_hidden=True, want_meanpool=True, want_qkv=True)
    calls["inputs_embeds groups"] = lambda: tr.encode_groups([emb, emb[:1, :9].contiguous()], embeds=True, want_hidden=True, want_meanpool=True)

    def prefill_embeds():
        cache = tr.new_kv_cache(2, 40, dev).zero_()
        return {"hidden": tr.prefill(cache, inputs_embeds=emb), "cache": cache}
    calls["inputs_embeds prefill"] = prefill_embeds
    return calls


# ------------------------------------------------------------------------------------------------------------ 1, 2: the encoder
@pytest.mark.parametrize("name", tuple(MODELS))
def test_01_encoder_outputs_under_both_words_equal_the_store_off_and_the_buffers_are_bf16(dev, name):
    """Mean-pool, hidden, the layers' residual streams and per-layer qkv (``want_qkv``, ``prefill``'s cache) at M = 5, 111, 128, 129,
    one ragged call of groups and the ``inputs_embeds`` forms: the bits of the store off.  And the store is real: each of these
    calls advances the ln1, ln2 and f counters by L (ln1 in layer 0 too) and "kept fp32" by nothing."""
    from rag4dyg_amd import ops
    m, L, d = model_of(dev, name)
    for word in WORDS:
        ops.set_encode_precision(word)
        for what, call in encoder_calls(m, dev, d, seed=len(name)).items():
            want, got, moved = off_on(call)
            assert same(want, got), (name, word, what)
            assert moved == counted(L, L, L, 0), (name, word, what, moved)


@pytest.mark.parametrize("d, H", ((64, 2), (320, 1)))
def test_02a_widths_off_the_16_byte_stores_keep_fp32(dev, d, H):
    """d = 64 (``L2_d64_T40``) and d = 320 are no multiples of 256: none of the three counters moves, every buffer is counted as
    kept fp32 (3 per layer), and the outputs are still those of the store off."""
    from rag4dyg_amd import ops
    if d == 64:
        m, ids = T16.model_on(dev, "L2_d64_T40")
        ids = ids.to(dev)
    else:
        m = seeded_model(dev, 2, H, d)
        ids = torch.randint(0, 59, (3, 37), generator=torch.Generator().manual_seed(d)).to(dev)
    for word in WORDS:
        ops.set_encode_precision(word)
        for qkv in (False, True):
            want, got, moved = off_on(lambda: m.transformer.encode(input_ids=ids, want_hidden=True, want_meanpool=True, want_qkv=qkv))
            assert same(want, got), (d, word, qkv)
            assert moved == counted(0, 0, 0, 6), (d, word, qkv, moved)


def test_02b_a_layer_without_planes_keeps_fp32_for_its_buffers(dev):
    """The rule is per buffer and per layer.  In gemm mode "f32" a layer's only plane is the bf16 one the model adds for the word
    (``GPT2Model._b1``); withheld for ALL of layer 1's weights, layer 1 keeps its three buffers fp32 (and runs the fp32 GEMMs it
    would run anyway) while layer 0 stores bf16; withheld for layer 1's mlp.c_proj ALONE, only that layer's f stays fp32 (c_fc then
    reads bf16 ln2 and writes fp32).  The same bits as the store off each time."""
    from rag4dyg_amd import ops
    m, L, d = model_of(dev, "L2_d256_T130")
    tr = m.transformer
    ids = torch.randint(0, 59, (3, 37), generator=torch.Generator().manual_seed(5)).to(dev)
    blk = tr.h[1]
    cases = {"the whole layer": ((blk.attn.c_attn.weight, blk.attn.c_proj.weight, blk.mlp.c_fc.weight, blk.mlp.c_proj.weight), counted(1, 1, 1, 3)),
             "mlp.c_proj": ((blk.mlp.c_proj.weight,), counted(2, 2, 1, 1)),
             "c_fc": ((blk.mlp.c_fc.weight,), counted(2, 1, 1, 2)),
             "c_attn": ((blk.attn.c_attn.weight,), counted(1, 2, 2, 1))}
    ops.set_gemm_mode("f32")
    original = type(tr)._b1
    try:
        for what, (withheld, expect) in cases.items():
            tr._b1 = lambda w, withheld=withheld: None if any(w is x for x in withheld) else original(tr, w)
            for word in WORDS:
                ops.set_encode_precision(word)
                want, got, moved = off_on(lambda: tr.encode(input_ids=ids, want_hidden=True, want_meanpool=True, want_qkv=(word == "bf16")))
                assert same(want, got), (what, word)
                assert moved == expect, (what, word, moved)
    finally:
        del tr._b1


# ------------------------------------------------------------------------------------------------------------ 3: the single ops
@pytest.mark.parametrize("N, K", ((1024, 256), (3072, 768)))
@pytest.mark.parametrize("M", (5, 111, 129, 2900))
def test_03_single_ops_gelu_and_none_with_a_bf16_output(dev, M, N, K):
    """``conv1d_bf16_act(layernorm_bf16(x), ..., "gelu")`` against ``conv1d_bf16(layernorm(x), ..., "gelu")`` rounded to bf16 by
    torch (nearest even), as bits; ``"none_bf16"`` against ``"none"`` likewise; the kinds that existed keep their bits.  M = 2900
    adds the 128 x 256 tile (and interior tiles) at N = 3072; the others run edge tiles of the 128 x 128 one."""
    from rag4dyg_amd import ops
    g = torch.Generator().manual_seed(M + N)
    x = (torch.randn(M, K, generator=g) * 2.0 + 0.3).to(dev)
    lw, lb = (1.0 + 0.1 * torch.randn(K, generator=g)).to(dev), (0.1 * torch.randn(K, generator=g)).to(dev)
    w = (torch.randn(K, N, generator=g) * 0.05).to(dev)
    b = (torch.randn(N, generator=g) * 0.1).to(dev)
    plane = ops.bf16_plane(w)
    ln32, ln16 = ops.layernorm(x, lw, lb), ops.layernorm_bf16(x, lw, lb)
    assert ln16.dtype == torch.bfloat16 and torch.equal(bits(ln16), bits(ln32.bfloat16()))
    for epi16, epi32 in (("gelu", "gelu"), ("none_bf16", "none")):
        for bias in (b, None):
            y16 = ops.conv1d_bf16_act(ln16, plane, bias, epi16)
            y32 = ops.conv1d_bf16(ln32, plane, bias, epi32)
            assert y16.dtype == torch.bfloat16 and y16.shape == y32.shape
            assert bool(torch.isfinite(y32).all()) and float(y32.abs().max()) > 0.1
            assert torch.equal(bits(y16), bits(y32.bfloat16())), (M, N, epi16, bias is None)
    assert torch.equal(bits(ops.conv1d_bf16_act(ln16, plane, b, "none")), bits(ops.conv1d_bf16(ln32, plane, b, "none")))
    pre, y = ops.conv1d_bf16_act(ln16, plane, b, "gelu_keep")
    assert torch.equal(bits(y), bits(ops.conv1d_bf16_act(ln16, plane, b, "gelu"))) and torch.equal(bits(pre), bits(ops.conv1d_bf16(ln32, plane, b, "none")))


def test_03b_the_bf16_outputs_write_their_own_elements_and_nothing_else(dev):
    """Guard rows behind the M rows of y keep their sentinel bits, for both new kinds, at an odd M with edge tiles in M and N."""
    from rag4dyg_amd import _lib
    lib = _lib.load()
    M, K, N, G = 111, 256, 200, 7
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, K, generator=g).to(dev).bfloat16()
    plane = (torch.randn(N, K, generator=g) * 0.05).to(dev).bfloat16().view(torch.int16)
    b = torch.randn(N, generator=g).to(dev)
    for kind in (3, 4):
        outs = []
        for fill in (ZERO, NAN):
            y = torch.empty(M + G, N, dtype=torch.bfloat16, device=dev)
            poison(y, fill)
            guard = y[M:].clone()
            _lib.check(lib.r4d_conv1d_bf16_act_f32(x.data_ptr(), plane.data_ptr(), b.data_ptr(), M, K, N, kind, None, y.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream), "conv1d_bf16_act")
            torch.cuda.synchronize()
            assert torch.equal(bits(y[M:]), bits(guard)), (kind, fill)
            outs.append(y[:M].clone())
        assert torch.equal(bits(outs[0]), bits(outs[1])) and bool(torch.isfinite(outs[0].float()).all()), kind
    y = torch.full((M, N), 7.0, dtype=torch.bfloat16, device=dev)
    for kind in (-1, 5):
        assert lib.r4d_conv1d_bf16_act_f32(x.data_ptr(), plane.data_ptr(), b.data_ptr(), M, K, N, kind, None, y.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream) == -1
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


# ------------------------------------------------------------------------------------------------------------ 4, 5: isolation
def test_04_the_store_without_a_bf16_word_changes_no_bit_and_counts_nothing(dev):
    from rag4dyg_amd import ops
    m, L, d = model_of(dev, "L2_d256_T130")
    ids = torch.randint(0, 59, (3, 37), generator=torch.Generator().manual_seed(4)).to(dev)
    enc = lambda: m.transformer.encode(input_ids=ids, want_hidden=True, want_meanpool=True, want_qkv=True)
    for mode in GEMM_MODES:
        ops.set_gemm_mode(mode)
        ops.set_encode_precision("fp32")
        want, got, moved = off_on(enc)
        assert same(want, got) and moved == counted(), (mode, moved)
        # ... and through the words and back: every setting returns to its own bits
        seen = {}
        for word, store in (("bf16", "fp32"), ("bf16", "bf16"), ("fp32", "bf16"), ("bf16+attn", "bf16"), ("bf16+attn", "fp32"), ("fp32", "fp32"),
                            ("bf16", "bf16"), ("bf16+attn", "fp32")):
            ops.set_encode_precision(word)
            ops.set_encode_act_store(store)
            r = clone(enc())
            assert same(seen.setdefault(word, r), r), (mode, word, store)
        assert same(seen["fp32"], want) and not same(seen["bf16"], want) and not same(seen["bf16+attn"], seen["bf16"]), mode


def _other_entries(dev):
    """What the store must not touch beyond tests/test_gpu_encode_bf16.py::_isolated_results (one retriever-training forward /
    backward, one LM step, the cached decode step at B = 4 and 40, ops.conv1d*, ops.lm_logits, the scoring kernels): one
    generator-training step, and the greedy step with and without its graph, from a cache and last rows that are given."""
    from rag4dyg_amd.generator_training import GeneratorTrainer
    from rag4dyg_amd.gpt2 import GreedyDecoder
    out = T16._isolated_results(dev)
    m, tok, idx, src = GT._setup(dev, 2, 2, 64, 60, 3, 20, seed=9, freeze=True)
    tr = GeneratorTrainer(m, freeze=True, dropout=(0.0, 0.0, 0.0))
    out["gen:loss"] = tr.step(tok.to(dev), GT._bags(idx, src, dev)).clone()
    for n, t in tr.grads.items():
        out["gen:grad:" + n] = t.clone()
    model, _ids = T16.model_on(dev, "L2_d64_T40")
    g = torch.Generator().manual_seed(12)
    B, cap = 3, 24
    cache = torch.randn(2, B, cap, 128, generator=g).to(dev)
    last = torch.randn(B, 64, generator=g).to(dev)
    for graph in (True, False):
        dec = GreedyDecoder(model.transformer, B, cap)
        try:
            dec.use_graph = graph
            dec.cache.copy_(cache)
            toks = dec.run(last, torch.tensor([5, 9, 12]), max_gen=4, len_limit=cap)
            out[f"greedy:graph{int(graph)}:tokens"] = torch.tensor(toks)
            out[f"greedy:graph{int(graph)}:logits"] = dec.logits.clone()
            out[f"greedy:graph{int(graph)}:cache"] = dec.cache.clone()
        finally:
            dec.close()
    return out


def test_05_every_other_entry_gives_identical_bits_with_the_store_on(dev):
    from rag4dyg_amd import ops
    for word in ("bf16+attn", "bf16"):
        ops.set_encode_precision(word)
        ops.set_encode_act_store("fp32")
        off = _other_entries(dev)
        ops.set_encode_act_store("bf16")
        before, before16, before_attn = hits(), T16.hits(), T16.hits("tuning:encode_bf16_attn:")
        on = _other_entries(dev)
        assert hits() == before and T16.hits() == before16 and T16.hits("tuning:encode_bf16_attn:") == before_attn, word
        assert set(on) == set(off) and len(off) > 30 and {"gen:loss", "lm:loss", "train:embeddings", "decode_step:B4", "greedy:graph1:logits"} <= set(off)
        for n in off:
            assert torch.equal(on[n], off[n]), (word, n)
        assert torch.equal(off["greedy:graph1:tokens"], off["greedy:graph0:tokens"])


class _EosOnly:
    def encode(self, text):
        assert text == "<|endoftext|>"
        return [R.EOS_ID]


# ------------------------------------------------------------------------------------------------------------ 6: greedy decoding
def test_06_greedy_decoding_gives_the_ids_of_the_store_off(dev):
    """``greedy_decode_batch``, val mode, under each word, with the store on: the ids of the store-off run, exactly.  On the g10
    trained weights and the 8 seeded prompts of the words' own greedy tests (d = 128: no multiple of 256, so the prefill keeps
    every buffer fp32 and says so), and on the seeded d = 256 model with 8 prompts of the same lengths, whose prefill does store
    bf16 (one ragged call of several length groups, layer 0 from ids)."""
    from rag4dyg_amd import ops
    from rag4dyg_amd.evaluation import greedy_decode_batch
    g10, _ = T16.model_on(dev, "g10_trained")
    m256, L, d = model_of(dev, "L2_d256_T130")
    g = torch.Generator().manual_seed(R.GREEDY_SEED)
    small = [torch.randint(0, 59, (n,), generator=g).tolist() for n in R.GREEDY_LENGTHS]
    for m, prompts, P, stored in ((g10, R.greedy_prompts(), R.fixture("g10_trained")[5], False), (m256, small, 160, True)):
        for word in WORDS:
            ops.set_encode_precision(word)
            want, got, moved = off_on(lambda: greedy_decode_batch(m, _EosOnly(), prompts, "val", P, 0, dev))
            assert len(want) == 8 and want == got and all(w[:len(p)] == p and len(w) > len(p) for w, p in zip(want, prompts)), (word, stored)
            if stored:
                assert moved[LN1] > 0 and moved[LN1] == moved[LN2] == moved[F] and moved[KEPT] == 0, (word, moved)
            else:
                assert moved[KEPT] > 0 and moved[LN1] == moved[LN2] == moved[F] == 0, (word, moved)


# ------------------------------------------------------------------------------------------------------------ 7: poison
@pytest.mark.parametrize("name", ("L2_d256_T130", "L2_d768_H8"))
def test_07_the_bf16_halves_are_written_before_they_are_read_and_nothing_reads_the_other_half(dev, name):
    """The workspace and the outputs filled with NaN bytes, with 0x7F bytes and with the word 1 before the call -- on first
    allocation and on reuse (tests/_poison.py) -- give the bits of a zeroed workspace under both words with the store on: the bf16
    ln1 / ln2 / f rows fill the first half of the fp32 buffers, and the half behind them is never read."""
    from rag4dyg_amd import ops
    m, L, d = model_of(dev, name)
    g = torch.Generator().manual_seed(17)
    ids = torch.randint(0, 59, (3, 43), generator=g).to(dev)
    batches = [ids, ids[:2, :33].contiguous(), ids[:1, :1].contiguous()]
    emb = (torch.randn(2, 37, d, generator=g) * 0.1).to(dev)
    ops.set_encode_act_store("bf16")

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
                e = m.transformer.encode(inputs_embeds=emb, want_hidden=True, want_meanpool=True)
            out.append(clone({"hidden": a["hidden"], "meanpool": a["meanpool"], "hidden_q": b["hidden"], "qkv": b["qkv"],
                              "groups_hidden": c["hidden"], "groups_meanpool": c["meanpool"], "embeds_hidden": e["hidden"]}))
        return out
    for word in WORDS:
        ops.set_encode_precision(word)
        before = hits()
        base = run(ZERO)
        assert delta(before) == counted(8 * L, 8 * L, 8 * L, 0), (name, word)
        for pattern in (NAN, HUGE, ONE):
            got = run(pattern)
            for k in range(2):
                assert all(bool(torch.isfinite(v).all()) for v in base[k].values()), (name, word)
                assert same(base[k], got[k]), (name, word, pattern, k)
