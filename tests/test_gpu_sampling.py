"""The sampler on the device (csrc/sampling.hip) against tests/_sampling_ref.py and tests/golden/g15_sampling_filter.npz.

  1. kept sets: exactly the reference's (fixture) and the float64 restatement's, at every size on either side of a wavefront, a
     workgroup pass and the LDS limit; planted ties on the top-k threshold and across the top-p cut;
  2. the draw: the uniform bit for bit, the token inside u Z's interval of the index-order prefix sums, widened by
     eps = (V / 64 + 256) 2^-24 -- the kernel's weights are exact integer sums of floor(expf(y - max) 2^40), so the whole error is
     expf's and the fp32 difference y - max;
  3. degenerate parameters and rows; 4. determinism; 5. frequencies; 6. the decoder; 7. generate; 8. the buffer contract.
"""
import numpy as np
import pytest
import torch

from _poison import PATTERNS, ZERO, poison, poisoned_allocations
from conftest import load_golden

import _sampling_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def run_op(dev, x, seen=None, step=0, stream=None, **kw):
    """x [B, V] (numpy fp32), seen bool [B, V] or None -> tokens [B], keep bool [B, V], u [B], seen afterwards bool [B, V] / None."""
    from rag4dyg_amd import ops
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float32)
    B, V = x.shape
    seen_d = torch.from_numpy(sr.pack_bits(np.broadcast_to(seen, (B, V))).view(np.int32).copy()).to(dev) if seen is not None else None
    step = torch.from_numpy(np.broadcast_to(np.asarray(step, dtype=np.int32), (B,)).copy())
    stream = torch.from_numpy(np.broadcast_to(np.asarray(np.arange(B) if stream is None else stream, dtype=np.int32), (B,)).copy())
    tok, keep, u = ops.sample_logits(torch.from_numpy(x).to(dev), step, stream, seen=seen_d, want_keep=True, want_u=True, **kw)
    torch.cuda.synchronize()
    return (tok.cpu().numpy(), sr.unpack_bits(keep.cpu().numpy(), V), u.cpu().numpy(),
            sr.unpack_bits(seen_d.cpu().numpy(), V) if seen is not None else None)


def ref_kw(kw):
    return dict(do_sample=kw.get("do_sample", True), tau=kw.get("temperature", 1.0), top_k=kw.get("top_k", 0), top_p=kw.get("top_p", 1.0),
                r=kw.get("repetition_penalty", 1.0), seed=kw.get("seed", 0))


def check_rows(dev, x, seen=None, step=0, stream=None, **kw):
    """Run the op and hold every row against the restatement: the uniform, the kept set, the draw.  Returns the tokens.
    The kept sets must be EQUAL, so the rows must leave the kernel's arithmetic no say at the cuts: its weights are off by expf's
    rounding and that of y - max, some 3 x 2^-24 = 1.8e-7 of a cumulative mass; the restatement's own margins are asserted to be
    ten times that (and the top-k threshold is a comparison of fp32 values, exact whenever the values differ)."""
    x = np.atleast_2d(x)
    B, V = x.shape
    tok, keep, u, seen_after = run_op(dev, x, seen, step, stream, **kw)
    steps = np.broadcast_to(np.asarray(step), (B,))
    streams = np.broadcast_to(np.arange(B) if stream is None else np.asarray(stream), (B,))
    worst = 0.0
    for b in range(B):
        sb = None if seen is None else np.broadcast_to(seen, (B, V))[b]
        ref = sr.sample_row(x[b], sb, stream=int(streams[b]), step=int(steps[b]), **ref_kw(kw))
        assert np.float32(ref["u"]) == u[b] and ref["u"] == float(u[b]), (b, ref["u"], u[b])
        assert ref["p_margin"] > 2e-6, ("the test's own row sits on a top-p cut", ref["p_margin"])
        assert np.array_equal(keep[b], ref["keep"]), (b, np.nonzero(keep[b] != ref["keep"])[0][:8])
        assert sr.draw_ok(tok[b], ref), (b, int(tok[b]), ref["token"], ref["u"])
        t = int(tok[b])
        uz = ref["u"] * ref["Z"]
        worst = max(worst, max(ref["C"][t] - ref["w"][t] - uz, uz - ref["C"][t], 0.0) / ref["Z"])
        if seen is not None:
            want = sb.copy()
            want[t] = True
            assert np.array_equal(seen_after[b], want), b
    print(f"[sampling draw] V {V} B {B} {kw}: u Z outside the chosen interval by at most {worst:.3e} Z (eps {sr.eps_of(V):.3e})")
    return tok


# ------------------------------------------------------------------------------------------------------------------ 1. kept sets
@pytest.mark.parametrize("V", sr.ALL_SIZES)
def test_kept_sets_equal_the_reference_and_the_restatement(dev, V):
    x, seen = sr.make_logits(V, sr.SEEDS[V])
    fixture = None
    if V in sr.FIXTURE_SIZES:
        g = load_golden("g15_sampling_filter")
        assert np.array_equal(g[f"x_{V}"], x)
        fixture = sr.unpack_bits(g[f"keep_{V}"], V)
    rows = np.stack([x, x, x])                                        # more than one workgroup
    for i, (k, p, t, r) in enumerate(sr.GRID):
        tok, keep, u, _ = run_op(dev, rows, seen, step=3, top_k=k, top_p=p, temperature=t, repetition_penalty=r, seed=9)
        ref = sr.sample_row(x, seen, True, t, k, p, r)
        for b in range(3):
            assert np.array_equal(keep[b], ref["keep"]), (V, k, p, t, r, b, int(keep[b].sum()), int(ref["keep"].sum()))
            if fixture is not None:
                assert np.array_equal(keep[b], fixture[i]), (V, k, p, t, r, b)
            assert keep[b][tok[b]]


def test_ties_on_the_top_k_threshold_are_all_kept_and_ties_across_the_top_p_cut_go_by_index(dev):
    for V in (7, 300, 20000):
        x = np.full(V, -3.0, np.float32)
        x[[V - 1, 0]] = 5.0, 3.0
        tied = [i for i in (2, 3, 5, V // 2, V - 2) if 0 < i < V - 1]
        x[tied] = 2.0
        _, keep, _, _ = run_op(dev, x, top_k=3)                        # the third largest is one of the tied entries
        assert sorted(np.nonzero(keep[0])[0]) == sorted(set([0, V - 1] + tied)), V
        ref = sr.sample_row(x, top_k=3)
        assert np.array_equal(keep[0], ref["keep"])
    for V in (6, 700, 17000):
        x = np.full(V, -np.inf, np.float32)
        ones = sorted({0, 2, 3, V // 2, V - 1} - {1})
        x[ones] = 0.0
        x[1] = 1.0                                                     # weights e : 1 : 1 : ...
        z = np.e + len(ones)
        _, keep, _, _ = run_op(dev, x, top_p=(np.e + 1.5) / z)         # mass in front of the entries: 0, e, e + 1 kept; e + 2 not
        assert list(np.nonzero(keep[0])[0]) == sorted([1] + ones[:2]), V
        assert np.array_equal(keep[0], sr.sample_row(x, top_p=(np.e + 1.5) / z)["keep"])
        check_rows(dev, np.stack([x] * 4), top_p=(np.e + 1.5) / z, seed=V)


# ------------------------------------------------------------------------------------------------------------------ 2. the draw
def draw_rows():
    rng = np.random.default_rng(79)
    g7 = load_golden("g7_generator")["fmlp_reddit_first_logits"][0].astype(np.float32)           # a trained model's logits, V 11,919
    rows = {"peaked": (rng.standard_normal(3001) * 2.5).astype(np.float32), "flat": (rng.standard_normal(50257) * 0.01).astype(np.float32),
            "trained": g7}
    bi = (rng.standard_normal(16385) * 0.5).astype(np.float32)
    bi[::2] += 6.0
    rows["bimodal"] = bi
    return rows


@pytest.mark.parametrize("name", ["peaked", "flat", "bimodal", "trained"])
@pytest.mark.parametrize("kw", [dict(), dict(top_k=50, top_p=0.95, temperature=0.8), dict(top_p=0.9), dict(temperature=1.5, repetition_penalty=1.3)],
                         ids=["plain", "k50 p.95 t.8", "p.9", "t1.5 r1.3"])
def test_the_draw_lands_in_its_interval_of_the_prefix_sums(dev, name, kw):
    x = draw_rows()[name]
    seen = (np.arange(x.size) % 5 == 0) if "repetition_penalty" in kw else None
    B = 24
    check_rows(dev, np.stack([x] * B), seen, step=np.arange(B) % 3, stream=np.arange(B) * 7 + 1, seed=0x1234567890ABCDEF, **kw)


# ------------------------------------------------------------------------------------------------------------------ 3. degenerate cases
def test_degenerate_parameters_give_the_argmax(dev):
    rng = np.random.default_rng(5)
    for V in (64, 1801, 16385):
        x = rng.standard_normal(V).astype(np.float32)
        top = int(rng.integers(V))
        x[top] = x.max() + 1.0                                         # a clear, tie-free maximum
        rows = np.stack([x] * 6)
        for kw in (dict(top_k=1), dict(top_p=1e-6), dict(temperature=1e-3), dict(do_sample=False)):
            tok, keep, _, _ = run_op(dev, rows, step=np.arange(6), **kw)
            assert list(tok) == [top] * 6, (V, kw, tok)
            if "temperature" not in kw:
                assert keep.sum() == 6 and keep[:, top].all()


def test_edge_rules(dev):
    nan, inf = float("nan"), float("inf")
    for V in (1, 5, 16500):
        for do_sample in (True, False):
            x = np.full(V, nan, np.float32)
            x[1::2] = -inf
            assert list(run_op(dev, np.stack([x] * 3), do_sample=do_sample)[0]) == [0] * 3             # nothing above -inf: id 0
            if V > 1:
                x = np.full(V, nan, np.float32)
                x[V - 2] = -7.0
                tok, keep, _, _ = run_op(dev, np.stack([x] * 3), do_sample=do_sample)                    # NaN is never chosen over a finite logit
                assert list(tok) == [V - 2] * 3
                x = np.linspace(-1, 1, V).astype(np.float32)
                x[[V - 1, V // 2]] = inf
                x[0] = nan
                tok, keep, _, _ = run_op(dev, np.stack([x] * 3), do_sample=do_sample, top_k=3, top_p=0.5)
                assert list(tok) == [V // 2] * 3 and keep.sum() == 3 and keep[:, V // 2].all()           # the lowest-indexed +inf
    tok, keep, u, _ = run_op(dev, np.zeros((4, 1), np.float32), top_k=50, top_p=0.3, temperature=0.5)   # V = 1
    assert list(tok) == [0] * 4 and keep.all() and np.array_equal(u, sr.philox_u(0, np.arange(4), 0)[0].astype(np.float32))


def test_penalty_signs_and_the_seen_bit(dev):
    # r = 4: the seen +2 becomes 0.5, the seen -1 becomes -4; unseen copies stay.  Arg-max and the kept set show both.
    x = np.array([2.0, 1.0, -1.0, -1.0, 0.75, -3.9], np.float32)
    seen = np.array([1, 0, 1, 0, 0, 0], bool)
    tok, keep, _, after = run_op(dev, x, seen, do_sample=False, repetition_penalty=4.0)
    assert tok[0] == 1 and after[0].tolist() == [True, True, True, False, False, False]                # the chosen id is now seen
    _, keep, _, _ = run_op(dev, x, seen, top_k=3, repetition_penalty=4.0)                              # 1.0, 0.75, 0.5 stay
    assert keep[0].tolist() == [True, True, False, False, True, False]
    _, keep, _, _ = run_op(dev, x, seen, top_k=5, repetition_penalty=4.0)                              # -1 (unseen) stays, -3.9 stays, -4 goes
    assert keep[0].tolist() == [True, True, False, True, True, True]
    _, keep, _, after = run_op(dev, x, None, top_k=3, repetition_penalty=4.0)                           # no bitmap: no penalty
    assert keep[0].tolist() == [True, True, False, False, True, False] and after is None
    check_rows(dev, np.stack([x] * 8), seen, repetition_penalty=4.0, temperature=0.7, seed=3)


# ------------------------------------------------------------------------------------------------------------------ 4. determinism
def test_tokens_do_not_depend_on_the_batch_or_the_place_in_it(dev):
    rng = np.random.default_rng(11)
    for V, kw in ((1801, dict(top_k=50, top_p=0.95, temperature=0.8)), (16385, dict(top_p=0.9)), (300, dict(repetition_penalty=1.2))):
        x = (rng.standard_normal((33, V)) * 3).astype(np.float32)
        seen = rng.random((33, V)) < 0.3
        steps, streams = rng.integers(0, 100, 33), rng.integers(0, 1000, 33)
        want = run_op(dev, x, seen, steps, streams, seed=42, **kw)
        for B in (1, 5, 32, 33):
            perm = rng.permutation(33)[:B]
            for _ in range(2):
                got = run_op(dev, x[perm], seen[perm], steps[perm], streams[perm], seed=42, **kw)
                assert np.array_equal(got[0], want[0][perm]) and np.array_equal(got[1], want[1][perm]), (V, B)
                assert np.array_equal(got[2], want[2][perm]) and np.array_equal(got[3], want[3][perm])


def test_another_seed_stream_or_step_is_another_draw(dev):
    x = np.zeros((4096, 64), np.float32)
    base = run_op(dev, x, step=0, stream=np.arange(4096), seed=1)[0]
    for kw in (dict(step=0, stream=np.arange(4096), seed=2), dict(step=0, stream=np.arange(4096) + 4096, seed=1),
               dict(step=1, stream=np.arange(4096), seed=1)):
        other = run_op(dev, x, **kw)[0]
        assert (other != base).mean() >= 0.9, kw
    assert np.array_equal(run_op(dev, x, step=0, stream=np.arange(4096), seed=1)[0], base)


# ------------------------------------------------------------------------------------------------------------------ 5. frequencies
def test_frequencies_of_65536_draws(dev):
    x, p, n, seed, want, near, q = sr.frequency_case()
    tok, _, u, _ = run_op(dev, np.broadcast_to(x, (n, 8)), step=0, stream=np.arange(n), seed=seed)
    assert np.array_equal(u.astype(np.float64), sr.philox_u(seed, np.arange(n), 0)[0])
    assert near.mean() <= 1e-3
    assert np.array_equal(tok[~near], want[~near])
    assert np.all(np.abs(tok[near] - want[near]) <= 1)
    counts, ref_counts = np.bincount(tok, minlength=8), np.bincount(want, minlength=8)
    assert np.abs(counts - ref_counts).sum() <= 2 * int(near.sum())
    sigma = np.sqrt(n * q * (1 - q))
    print("[sampling freq] counts", counts.tolist(), "restatement", ref_counts.tolist(), "near a boundary", int(near.sum()))
    assert np.all(np.abs(counts - n * q) <= 5 * sigma)


# ------------------------------------------------------------------------------------------------------------------ 6. the decoder
def tiny_model(dev, d, V, rag=False, seed=21):
    from oracle import gpt2_ref
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModel, GPT2LMHeadModelRAG
    sd = gpt2_ref.make_state_dict(2, d, V, n_positions=256, seed=seed, random_affine=True)
    sd["transformer.wte.weight"] *= 3.0                               # (tied: the head too) logits some 0.5 wide: every draw is open
    cls = GPT2LMHeadModelRAG if rag else GPT2LMHeadModel
    m = cls(GPT2Config(vocab_size=V, n_positions=256, n_ctx=256, n_embd=d, n_layer=2, n_head=2))
    m.load_state_dict(sd, strict=False)
    return m.to(dev).eval()


PROMPT_LENS = [9, 3, 7, 1, 9]
SAMPLING = dict(do_sample=True, temperature=0.9, top_k=20, top_p=0.9, repetition_penalty=1.3, seed=77)


def decode_once(m, dev, prompt, graph, max_gen=10, len_limit=128, eos=(), check=False, sampling=SAMPLING):
    from rag4dyg_amd.gpt2 import SamplingDecoder
    tr = m.transformer
    B, V = len(PROMPT_LENS), tr.wte.num_embeddings
    dec = SamplingDecoder(tr, B, 128)
    dec.use_graph = graph
    try:
        last = tr.prefill_last(dec.cache, PROMPT_LENS, input_ids=prompt)
        ids = [prompt[i, :n].tolist() for i, n in enumerate(PROMPT_LENS)]
        if not check:
            return dec.run(last, torch.tensor(PROMPT_LENS), max_gen, len_limit, eos, seen_ids=ids, **sampling), dec.graph_builds
        dec.begin_sampling(last, torch.tensor(PROMPT_LENS), max_gen, len_limit, eos, seen_ids=ids, **sampling)
        seen = np.zeros((B, V), bool)
        for i, row in enumerate(ids):
            seen[i, row] = True
        assert np.array_equal(sr.unpack_bits(dec.seen.cpu().numpy(), V), seen)           # the prompt is penalised from step 0
        out = [[] for _ in range(B)]
        for _ in range(max_gen + 2):                                                      # (two more: finished rows stay finished)
            active, g0 = dec.active.cpu().numpy().copy(), dec.gen_len.cpu().numpy().copy()
            dec._steps(1)
            torch.cuda.synchronize()
            logits, toks, g1 = dec.logits.cpu().numpy(), dec.out.cpu().numpy(), dec.gen_len.cpu().numpy()
            for b in range(B):
                if not active[b]:
                    assert g1[b] == g0[b] and not dec.active[b]
                    continue
                assert g1[b] == g0[b] + 1
                t = int(toks[b, g0[b]])
                ref = sr.sample_row(logits[b], seen[b], stream=b, step=int(g0[b]), **ref_kw(sampling))
                assert sr.draw_ok(t, ref), (b, g0[b], t, ref["token"])
                seen[b, t] = True
                out[b].append(t)
            assert np.array_equal(sr.unpack_bits(dec.seen.cpu().numpy(), V), seen)
        return out, dec.graph_builds
    finally:
        dec.close()


@pytest.mark.parametrize("d,V", [(64, 90), (256, 300)], ids=["d64", "d256 skinny route"])
def test_decoder_tokens_follow_the_device_logits_and_the_graph_replays_them(dev, d, V, monkeypatch):
    m = tiny_model(dev, d, V)
    prompt = torch.randint(0, V, (5, 9), generator=torch.Generator().manual_seed(4)).to(dev)
    stepped, builds = decode_once(m, dev, prompt, graph=False, check=True)
    assert builds == 0 and all(len(t) == 10 for t in stepped)
    assert len({tuple(t) for t in stepped}) > 1
    looped, _ = decode_once(m, dev, prompt, graph=False)
    replayed, builds = decode_once(m, dev, prompt, graph=True)
    assert builds == 1 and looped == stepped and replayed == stepped
    monkeypatch.setenv("R4D_DECODE_GRAPH", "0")
    from rag4dyg_amd.gpt2 import SamplingDecoder
    dec = SamplingDecoder(m.transformer, 5, 128)
    assert dec.use_graph is False
    dec.close()
    # stop rules: an eos that row 2 sampled as its 4th token stops it there (and any row at its first such token); the others run on
    eos = stepped[2][3]
    got, _ = decode_once(m, dev, prompt, graph=True, eos=(eos,))
    for b in range(5):
        cut = stepped[b].index(eos) + 1 if eos in stepped[b] else 10
        assert got[b] == stepped[b][:cut], b
    assert len(got[2]) <= 4
    assert [len(t) for t in decode_once(m, dev, prompt, graph=True, max_gen=3)[0]] == [3] * 5
    # len_limit: a row stops once its length reaches it -- prompt 9: 12 - 9 = 3 tokens, prompt 1: 10 (max_gen first)
    assert [len(t) for t in decode_once(m, dev, prompt, graph=False, len_limit=12)[0]] == [3, 9, 5, 10, 3]
    for b, t in enumerate(decode_once(m, dev, prompt, graph=False, len_limit=12)[0]):
        assert t == stepped[b][:len(t)]


def test_decoder_out_cap_stops_a_row(dev):
    from rag4dyg_amd.gpt2 import SamplingDecoder
    m = tiny_model(dev, 64, 90)
    tr = m.transformer
    prompt = torch.randint(0, 90, (5, 9), generator=torch.Generator().manual_seed(4)).to(dev)
    dec = SamplingDecoder(tr, 5, 128)
    try:
        dec.sstate.out_cap = dec.state.out_cap = 4                                        # the step now treats `out` as rows of 4 ids
        dec.use_graph = False
        last = tr.prefill_last(dec.cache, PROMPT_LENS, input_ids=prompt)
        toks = dec.run(last, torch.tensor(PROMPT_LENS), 10, 128, (), **SAMPLING)
        assert [len(t) for t in toks] == [4] * 5 and not bool(dec.active.any())
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------------------------ 7. generate
@pytest.mark.parametrize("rag", [False, True], ids=["GPT2LMHeadModel", "GPT2LMHeadModelRAG"])
def test_generate_layout_seeds_and_the_greedy_path(dev, rag):
    V, T = 90, 6
    m = tiny_model(dev, 64, V, rag=rag)
    tr = m.transformer
    prompt = torch.randint(1, V, (3, T), generator=torch.Generator().manual_seed(8)).to(dev)
    # greedy: the existing greedy step, id for id
    out = m.generate(input_ids=prompt, max_length=14, do_sample=False)
    assert out.dtype == torch.int64 and tuple(out.shape) == (3, 14) and torch.equal(out[:, :T], prompt)
    dec = tr.greedy_decoder(3, 14)
    last = tr.prefill_last(dec.cache, [T] * 3, input_ids=prompt)
    want = dec.run(last, torch.tensor([T] * 3), 8, 129, ())
    assert out[:, T:].tolist() == want
    # sampled: n rows per prompt, rows i n .. i n + n - 1 continue prompt i, stream = row number
    kw = dict(max_length=14, do_sample=True, top_k=30, top_p=0.95, temperature=1.1, repetition_penalty=1.2, num_return_sequences=4)
    a = m.generate(input_ids=prompt, seed=5, **kw)
    assert tuple(a.shape) == (12, 14) and torch.equal(a[:, :T], prompt.repeat_interleave(4, 0))
    assert torch.equal(m.generate(input_ids=prompt, seed=5, **kw), a)                      # one seed: the same call
    assert not torch.equal(m.generate(input_ids=prompt, seed=6, **kw), a)
    assert len({tuple(r) for r in a[:4].tolist()}) > 1                                     # rows of one prompt draw from their own streams
    # eos and padding: an id that some row generated mid-way ends that row; the rest is pad, L is the longest row
    eos = int(a[5, T + 2])
    b = m.generate(input_ids=prompt, seed=5, eos_token_ids=eos, pad_token_id=0, **kw)
    cuts = [(r.index(eos) + 1 if eos in r else 8) for r in a[:, T:].tolist()]
    assert cuts[5] <= 3

    def padded(pad):
        return [r[:T + c] + [pad] * (max(cuts) - c) for r, c in zip(a.tolist(), cuts)]
    assert b.tolist() == padded(0)
    c = m.generate(input_ids=prompt, seed=5, eos_token_ids=[eos], **kw)                    # no pad id: the first eos id pads
    assert c.tolist() == padded(eos)
    # the splice form: embeddings for the prompt (ids optional)
    emb = tr.wte.weight[prompt]
    e1 = m.generate(input_ids=prompt, inputs_embeds=emb, seed=5, **kw)
    assert torch.equal(e1, a)
    e2 = m.generate(inputs_embeds=emb, max_length=14, do_sample=True, top_k=30, seed=5)
    assert tuple(e2.shape) == (3, 8)
    with pytest.raises(ValueError):
        m.generate(inputs_embeds=emb, max_length=14, do_sample=True, repetition_penalty=1.2)
    # a penalised greedy call runs the sampler's arg-max (one row per prompt)
    g = m.generate(input_ids=prompt, max_length=14, do_sample=False, repetition_penalty=1.5)
    assert tuple(g.shape) == (3, 14) and torch.equal(g[:, :T], prompt) and bool(((g >= 0) & (g < V)).all())


# ------------------------------------------------------------------------------------------------------------------ 8. the buffer contract
def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _assert_same_runs(run):
    base = run(ZERO)
    for pattern in PATTERNS[1:]:
        got = run(pattern)
        assert len(got) == len(base)
        for k, (a, b) in enumerate(zip(base, got)):
            assert set(a) == set(b)
            for n in a:
                assert a[n].shape == b[n].shape and torch.equal(_bits(a[n]), _bits(b[n])), (pattern, k, n)


def test_sample_logits_does_not_read_its_outputs(dev):
    from rag4dyg_amd import ops
    rng = np.random.default_rng(3)
    cases = [(5, 300, dict(top_k=20, top_p=0.9)), (3, 16385, dict(top_p=0.8, temperature=0.7)), (4, 65, dict(do_sample=False))]

    def run(pattern):
        out = []
        for B, V, kw in cases:
            x = torch.from_numpy((np.random.default_rng(V).standard_normal((B, V)) * 4).astype(np.float32)).to(dev)
            with poisoned_allocations(pattern):                        # token, keep and u are torch.empty on the Python side
                tok, keep, u = ops.sample_logits(x, torch.zeros(B, dtype=torch.int32), torch.arange(B, dtype=torch.int32),
                                                 want_keep=True, want_u=True, seed=4, **kw)
            out.append(dict(tok=tok.clone(), keep=keep.clone(), u=u.clone()))
        return out
    _assert_same_runs(run)


@pytest.mark.parametrize("graph", [False, True], ids=["host loop", "graph"])
def test_sampled_loop_does_not_read_unwritten_memory(dev, graph):
    """``r4d_gpt2_sample_step_f32`` / ``_graph_create``: the decoder's cache, ``ws``, ``logits``, ``out`` and ``next`` poisoned
    (allocated under poison, then refilled): the ids, the last logits and the seen bitmap."""
    from rag4dyg_amd import ops
    from rag4dyg_amd.gpt2 import SamplingDecoder
    m = tiny_model(dev, 256, 300)
    tr = m.transformer
    prompt = torch.randint(0, 300, (5, 9), generator=torch.Generator().manual_seed(4)).to(dev)
    ids = [prompt[i, :n].tolist() for i, n in enumerate(PROMPT_LENS)]

    def run(pattern):
        ops._WS.clear()
        with poisoned_allocations(pattern):
            dec = SamplingDecoder(tr, 5, 128)
        dec.use_graph = graph
        out = []
        try:
            for _ in range(2):
                for b in (dec.cache, dec.ws, dec.logits):
                    poison(b, pattern)
                with poisoned_allocations(pattern):
                    last = tr.prefill_last(dec.cache, PROMPT_LENS, input_ids=prompt)
                toks = dec.run(last, torch.tensor(PROMPT_LENS), 6, 128, (), seen_ids=ids, **SAMPLING)
                assert all(len(t) == 6 for t in toks)
                out.append(dict(tokens=torch.tensor(toks), logits=dec.logits.clone(), seen=dec.seen.clone()))
            assert dec.graph_builds == (1 if graph else 0)
        finally:
            dec.close()
        return out
    _assert_same_runs(run)
