"""The cached decode step at the contexts greedy generation serves (positions up to 1023), against float64 references.

``decode_attn_kernel`` walks the cache in trips of 128 keys (64 at head_dim 256), carries an online-softmax state per group of
lanes from trip to trip, clamps the loads of a last, partial trip and merges 16 (8) group states at the end.  Here:

  a. planted caches (tests/_decode_ref.py: the LOGIT of every cached key is chosen), one launch per (width, pattern) whose 13
     batch rows sit on every boundary -- an empty cache, the group count, each side of the first and second trip, 640, 1023;
  b. a real two-layer cache: ragged ``prefill_last`` then three steps, on plain and on sharpened attention weights;
  c. ties in the device argmax of the greedy loop: the lowest index wins.

tests/test_host_decode_ref.py shows, without a GPU, that one lost or doubled boundary key of (a) moves the output by 10x or more
of the bound used here.  The measured errors are recorded in profiles/decode_long_context.md."""
import numpy as np
import pytest
import torch

from _decode_ref import PATTERNS, cast_sd, decode_step_ref, plant_cache, trip_of
from conftest import elementwise_err, rel_err

pytestmark = pytest.mark.gpu

V, T_CAP = 40, 1024
NAN_BITS = 0x7FC0BEEF                          # a quiet NaN with a payload, as int32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def build_model(sd, L, H, d, vocab, dev):
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModel
    m = GPT2LMHeadModel(GPT2Config(vocab_size=vocab, n_positions=T_CAP, n_ctx=T_CAP, n_embd=d, n_layer=L, n_head=H))
    m.load_state_dict(sd, strict=False)          # an ``lm_head.weight`` of its own in ``sd`` unties the head
    return m.to(dev).eval()


def nan_cache(tr, B, dev):
    cache = tr.new_kv_cache(B, T_CAP, dev)
    cache.view(torch.int32).fill_(NAN_BITS)
    assert bool(torch.isnan(cache[0, 0, 0, 0]))
    return cache


@pytest.fixture(scope="module")
def planted_model(dev):
    """``get(H, d)`` -> (state dict, its float64 copy, the model on the device), shared by the five patterns of a width.  Only the
    width last asked for stays resident, and nothing does once the module is done."""
    from oracle import gpt2_ref
    held = {}

    def get(H, d):
        if (H, d) not in held:
            held.clear()
            sd = gpt2_ref.make_state_dict(1, d, V, n_positions=T_CAP, seed=H * 1000 + d, random_affine=True)
            held[(H, d)] = (sd, cast_sd(sd, torch.float64), build_model(sd, 1, H, d, V, dev))
        return held[(H, d)]
    yield get
    held.clear()


def drop_greedy_decoders(tr):
    """Forget the transformer's cached ``GreedyDecoder``s (the next one is built under the current ``R4D_DECODE_GRAPH``) and
    destroy their captured graphs now, not whenever the objects are collected."""
    for dec in tr.__dict__.pop("_greedy_decoders", {}).values():
        dec.close()


def branch_hits():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    return {lib.r4d_dispatch_branch_name(i).decode(): int(lib.r4d_dispatch_branch_hits(i)) for i in range(lib.r4d_dispatch_num_branches())}


def positions(head_dim):
    trip = trip_of(head_dim)
    return [0, 1, 15, 16, 17, trip - 1, trip, trip + 1, 2 * trip - 1, 2 * trip, 2 * trip + 1, 640, 1023]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("H,d", [(2, 64), (2, 128), (2, 192), (2, 256), (2, 512), (8, 768)])
def test_planted_cache_every_trip_boundary(dev, planted_model, H, d, pattern):
    """13 sequences = 13 cache lengths in ONE ``decode_step``; rows at and past ``pos`` hold a NaN pattern.  Output rows against
    float64 (rel_err < 2e-5, elementwise_err < 1; no worse than 20x what a float32 CPU evaluation costs), the cache untouched
    outside row ``pos``, the new row equal to the float64 K | V, and a second call bit-identical."""
    sd, sd64, m = planted_model(H, d)
    tr = m.transformer
    pos = positions(d // H)
    B = len(pos)
    g = torch.Generator().manual_seed(d * 10 + PATTERNS.index(pattern))
    ids = torch.randint(0, V, (B,), generator=g)
    cache = nan_cache(tr, B, dev)
    rows = []
    for b, p in enumerate(pos):
        x = sd["transformer.wte.weight"][ids[b]] + sd["transformer.wpe.weight"][p]      # the fp32 sum the device forms itself
        K, Vv = plant_cache(sd, H, x, p, pattern, g)
        cache[0, b, :p] = torch.cat([K, Vv], dim=1).to(dev)
        rows.append((x, K, Vv))
    before = cache.clone()
    pos_d = torch.tensor(pos, dtype=torch.int32, device=dev)
    emb = tr.wte.weight[ids.to(dev)]                                    # the step adds wpe[pos] itself
    h = tr.decode_step(cache, pos_d, inputs_embeds=emb)
    after = cache.clone()
    h2 = tr.decode_step(cache, pos_d, inputs_embeds=emb)
    assert torch.equal(h.view(torch.int32), h2.view(torch.int32)) and torch.equal(after.view(torch.int32), cache.view(torch.int32))
    assert bool(torch.isfinite(h).all())
    untouched = torch.ones(B, T_CAP, dtype=torch.bool, device=dev)
    untouched[torch.arange(B, device=dev), pos_d.long()] = False
    same = (after.view(torch.int32) == before.view(torch.int32)).all(dim=-1)[0]
    assert bool(same[untouched].all()), "a cache row other than row pos was written"
    h, new_rows = h.cpu(), after[0, torch.arange(B, device=dev), pos_d.long()].cpu()
    worst = dict(dev=[0.0, 0.0], f32=[0.0, 0.0])
    for b, (p, (x, K, Vv)) in enumerate(zip(pos, rows)):
        want, _, k_new, v_new = decode_step_ref(sd64, H, x, K, Vv, torch.float64)
        f32 = decode_step_ref(sd, H, x, K, Vv, torch.float32)[0]
        e_dev, w_dev = rel_err(h[b].numpy(), want.numpy()), elementwise_err(h[b].numpy(), want.numpy())
        e_f32, w_f32 = rel_err(f32.numpy(), want.numpy()), elementwise_err(f32.numpy(), want.numpy())
        print(f"[decode-long row] H {H} d {d} {pattern} pos {p}: device {e_dev:.2e} {w_dev:.3f}  float32 {e_f32:.2e} {w_f32:.3f}")
        worst["dev"] = [max(worst["dev"][0], e_dev), max(worst["dev"][1], w_dev)]
        worst["f32"] = [max(worst["f32"][0], e_f32), max(worst["f32"][1], w_f32)]
        assert e_dev < 2e-5 and w_dev < 1, (p, e_dev, w_dev)
        assert e_dev < 20 * max(e_f32, 1e-6), (p, e_dev, e_f32)
        assert elementwise_err(new_rows[b].numpy(), torch.cat([k_new, v_new]).numpy()) < 1, p
    print(f"[decode-long] H {H} d {d} {pattern}: device {worst['dev'][0]:.2e} {worst['dev'][1]:.3f}  "
          f"float32 {worst['f32'][0]:.2e} {worst['f32'][1]:.3f}  ratio {worst['dev'][0] / worst['f32'][0]:.2f}")


@pytest.mark.parametrize("weights", ["plain", "peaked"])
@pytest.mark.parametrize("L,H,d", [(2, 2, 512), (2, 2, 256)])
def test_real_cache_two_layers_ragged_prompts(dev, L, H, d, weights):
    """``prefill_last`` over prompts of 1 .. 1020 tokens, then three cached steps: every step's rows against a float64 forward
    over the extended sequence (by causality ONE forward over the final sequence holds the last row of every prefix) and against
    the library's own ``encode`` of it.  ``peaked``: attention logits x 36 (head_dim 256) / x 16 (head_dim 128), the factors of
    the attention-stress fixtures."""
    from oracle import gpt2_ref
    sd = gpt2_ref.make_state_dict(L, d, V, n_positions=T_CAP, seed=L * 100 + d, random_affine=True)
    if weights == "peaked":
        sd = gpt2_ref.sharpen_attention(sd, 6.0 if d // H == 256 else 4.0)
    sd64 = cast_sd(sd, torch.float64)
    tr = build_model(sd, L, H, d, V, dev).transformer
    lens = [1, 63, 64, 127, 128, 129, 511, 1020]
    B, steps = len(lens), 3
    g = torch.Generator().manual_seed(d)
    seqs = [torch.randint(0, V, (n + steps,), generator=g) for n in lens]
    ids = torch.zeros(B, max(lens), dtype=torch.int64)
    for i, n in enumerate(lens):
        ids[i, :n] = seqs[i][:n]
    cache = nan_cache(tr, B, dev)
    tr.prefill_last(cache, lens, input_ids=ids.to(dev))
    hs = []
    for k in range(steps):
        new = torch.stack([seqs[i][lens[i] + k] for i in range(B)])
        hs.append(tr.decode_step(cache, torch.tensor(lens, dtype=torch.int32) + k, input_ids=new).cpu())
    worst = [0.0, 0.0, 0.0]
    for i, n in enumerate(lens):
        want = gpt2_ref.gpt2_forward(sd64, seqs[i].view(1, -1), H, want_logits=False)["hidden"][0]
        full = tr.encode(seqs[i].view(1, -1).to(dev))["hidden"][0].cpu()
        for k in range(steps):
            got = hs[k][i].numpy()
            e, w = rel_err(got, want[n + k].numpy()), elementwise_err(got, want[n + k].numpy())
            e_own = rel_err(got, full[n + k].numpy())
            print(f"[decode-long real] L {L} H {H} d {d} {weights} prompt {n} step {k}: float64 {e:.2e} {w:.3f}  own encode {e_own:.2e}")
            worst = [max(a, b_) for a, b_ in zip(worst, (e, w, e_own))]
            assert e < 2e-5 and w < 1, (n, k, e, w)
            assert e_own < 1e-5, (n, k, e_own)
    print(f"[decode-long real] L {L} H {H} d {d} {weights}: float64 {worst[0]:.2e} {worst[1]:.3f}  own encode {worst[2]:.2e}")


TIE_OFFSETS = (1, 63, 64, 255, 256, 257)
# one count per launch (the tile shape / the kernel form; the split-K and operand-layout branches count the same launches again)
TILED_GEMM_BRANCHES = ("gemm_kc:128x128x16", "gemm_kc:128x64x16", "gemm_kc:64x64x32", "gemm_f32:128x128", "gemm_f32:128x64", "gemm_f32:64x64")
SKINNY_GEMM_BRANCHES = ("skinny16:ng2", "skinny16:ng3", "skinny16:ng2+layernorm", "skinny16:ng3+layernorm",
                        "skinny16:LayerNorm pre-folded into the weight", "skinny8:ng2", "skinny8:ng3", "skinny:plain + epilogue launch")


def tie_plan(B, vocab):
    """Per sequence the indices that get the same lm_head row, ascending: pairs ``(a, a + offset)`` with the offsets cycling
    through ``TIE_OFFSETS`` (one thread of the 256-wide argmax scan, neighbouring lanes, another wavefront, the next stride of the
    scan); sequence 1's pair ends at the last index, sequence 2 is a triple.  All indices distinct."""
    plan = []
    for i in range(B):
        o = TIE_OFFSETS[i % len(TIE_OFFSETS)]
        a = 2 + 10 * i
        plan.append((a, a + o))
    plan[1] = (vocab - 1 - TIE_OFFSETS[1], vocab - 1)
    plan[2] = plan[2] + (plan[2][1] + TIE_OFFSETS[5],)
    flat = [j for t in plan for j in t]
    assert len(set(flat)) == len(flat) and max(flat) == vocab - 1 and min(flat) >= 0, plan
    assert {t[1] - t[0] for t in plan} == set(TIE_OFFSETS)
    return plan


@pytest.mark.parametrize("vocab", [600, 1000])
@pytest.mark.parametrize("L,H,d,B,tiled,skinny", [(1, 2, 64, 6, 4, 1), (1, 2, 64, 33, 5, 0), (1, 2, 512, 6, 0, 5), (1, 8, 1024, 6, 0, 5)])
def test_device_argmax_takes_the_lowest_index_of_a_tie(dev, monkeypatch, L, H, d, B, tiled, skinny, vocab):
    """``greedy_advance_kernel`` promises the lowest index among equal maxima (CPU ``torch.argmax``).  An untied lm_head gets, for
    sequence i, identical rows 5 h_i / |h_i| at two or three indices (h_i = the prompt's last hidden row): their logits are the
    row's maximum and bit-equal -- asserted on ``ops.lm_logits`` AND on the logits the decoder itself computed -- and the token
    must be the first of them.  Captured graph and kernel by kernel.

    The greedy step computes its logits as a weight stream (``launch_gemm_skinny``) for B <= 32 at d % 256 == 0 -- one k slice at
    d = 512, two slices merged by the last arriver at d = 1024 -- and as the tiled exact-f32 GEMM of ``ops.lm_logits`` otherwise
    (d = 64 at either batch size, any d beyond 32 sequences).  Which one ran is read from the dispatch counters around
    ``GreedyDecoder.run``, which launches five GEMMs (the head, then the four projections of the one layer): ``tiled`` of them on
    the tiled exact-f32 kernels and ``skinny`` as weight streams.  At d = 512 and 1024 no tiled GEMM runs at all: the head is
    skinny.  At d = 64 the head (K = 64: refused by the skinny kernel) is tiled: every projection but the K = 256 one of the MLP
    is too at B = 6, all five GEMMs are at B = 33."""
    from oracle import gpt2_ref
    from rag4dyg_amd import ops
    g = torch.Generator().manual_seed(vocab + B + d)
    sd = gpt2_ref.make_state_dict(L, d, vocab, n_positions=T_CAP, seed=vocab, random_affine=True)
    sd["lm_head.weight"] = 0.02 * torch.randn(vocab, d, generator=g)
    m = build_model(sd, L, H, d, vocab, dev)
    assert not m.lm_head_is_tied()
    tr = m.transformer
    lens = [int(n) for n in torch.randint(1, 30, (B,), generator=g)]
    ids = torch.randint(0, vocab, (B, max(lens)), generator=g).to(dev)
    plan = tie_plan(B, vocab)
    try:
        for graph in ("1", "0"):
            monkeypatch.setenv("R4D_DECODE_GRAPH", graph)
            drop_greedy_decoders(tr)
            dec = tr.greedy_decoder(B, 64)
            last = tr.prefill_last(dec.cache, lens, input_ids=ids)
            if graph == "1":                                              # the head is built once, from the first prefill's rows
                rows = 0.02 * torch.randn(vocab, d, generator=g)
                hn = last.cpu()
                for i, t in enumerate(plan):
                    rows[list(t)] = 5.0 * hn[i] / hn[i].norm()
                m.lm_head.weight.data.copy_(rows.to(dev))
            own = ops.lm_logits(last.contiguous(), m.lm_head.weight).cpu()
            dec.logits.fill_(float("nan"))
            before = branch_hits()
            toks = dec.run(last, torch.tensor(lens), max_gen=1, len_limit=64)
            hits = {k: v - before[k] for k, v in branch_hits().items() if v != before[k]}
            print(f"[decode-long tie] d {d} B {B} V {vocab} graph {graph}: {hits}")
            n_tiled = sum(v for k, v in hits.items() if k in TILED_GEMM_BRANCHES)
            n_skinny = sum(v for k, v in hits.items() if k in SKINNY_GEMM_BRANCHES)
            assert (n_tiled, n_skinny) == (tiled, skinny), (graph, hits)
            assert not [k for k in hits if k.startswith(("gemm_s3", "gemm_h2", "tuning:"))], hits      # no other GEMM family
            for which, logits in (("ops.lm_logits", own), ("decoder", dec.logits.cpu())):       # the precondition, checked
                for i, t in enumerate(plan):
                    tied = logits[i, list(t)]
                    assert torch.equal(tied.view(torch.int32), tied[:1].expand_as(tied).view(torch.int32)), (which, graph, i, tied)
                    rest = logits[i].clone()
                    rest[list(t)] = -float("inf")
                    assert float(rest.max()) < float(tied[0]), (which, graph, i)
            assert dec.use_graph == (graph == "1")
            assert [tk[0] for tk in toks] == [t[0] for t in plan] and all(len(tk) == 1 for tk in toks), (graph, toks, plan)
    finally:
        drop_greedy_decoders(tr)
