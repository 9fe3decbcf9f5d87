"""``ops.beam_select`` (``r4d_beam_select_f32``: the beam step's per-row candidates and per-prompt merge, alone) against the float64
restatement tests/_beam_ref.py.

Indices are exact.  Scores are within a bound that comes from the reference's own arithmetic: E = the largest difference between
torch's CPU fp32 ``log_softmax(x) + beam_score`` and float64 over the rows of the same call; the gate is 8 E (the factor of the
project's other float64 gates, profiles/train_stress_parity.md), and never below one fp32 ulp of the score.  E is a property of the
arithmetic, so it is taken over all rows of a call, not row by row: at V = 2 a row is two samples, torch is exact on some of them
by chance, and 8 x 0 would ask more than any fp32 chain of three roundings and two 1-ulp functions can give.  Only the rows that
start at -1e9 are measured apart from the others: fp32's unit there is 64, which says nothing about a score of magnitude 10.
The measured errors are printed (profiles/beam_search.md holds a run's).  Random rows are kept only if the restated order has a margin of 1e-4 between
neighbours -- a hundred times fp32's error on scores of magnitude 10 -- so the exact comparison of indices is sound."""
import numpy as np
import pytest
import torch

import _beam_ref as br

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 40, 257, 16384, 16385]          # below 2n, one wavefront, an odd size, the LDS limit and the first re-read row
BEAMS = [2, 3, 16]
ORDER_MARGIN = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def pack_bits(seen):
    R, V = seen.shape
    nw = (V + 31) // 32
    bits = np.zeros((R, nw), dtype=np.uint32)
    r, j = np.nonzero(seen)
    np.bitwise_or.at(bits, (r, j >> 5), np.uint32(1) << (j & 31).astype(np.uint32))
    return torch.from_numpy(bits.view(np.int32))


def run_op(dev, x, bs, n, r=1.0, seen=None, rows=False):
    from rag4dyg_amd import ops
    out = ops.beam_select(torch.from_numpy(x).to(dev), torch.from_numpy(bs).to(dev), n, r, pack_bits(seen).to(dev) if seen is not None else None,
                          want_rows=rows)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def reference_error(x, bs, seen, r):
    """Per row: max |torch fp32 log_softmax + beam score - float64| over the row's finite scores."""
    E = np.zeros(x.shape[0])
    for i in range(x.shape[0]):
        xp32 = x[i].copy()                                     # (the penalty itself in fp32, as the reference applies it)
        if seen is not None and r != 1.0:
            s = seen[i]
            xp32[s] = np.where(xp32[s] < 0, xp32[s] * np.float32(r), xp32[s] / np.float32(r))
        t = torch.log_softmax(torch.from_numpy(np.nan_to_num(xp32, nan=-np.inf)), dim=-1) + float(np.float32(bs[i]))
        ref = br.row_scores(x[i], np.float32(bs[i]), None if seen is None else seen[i], r)
        ok = np.isfinite(ref) & np.isfinite(t.numpy())
        E[i] = np.abs(t.numpy()[ok].astype(np.float64) - ref[ok]).max() if ok.any() else 0.0
    return E


def check(dev, x, bs, n, r=1.0, seen=None, round32=False, need_margin=True, what=""):
    """Every prompt of ``x`` [B0 * n, V] against the restatement; returns the op's outputs."""
    R, V = x.shape
    B0 = R // n
    got_s, got_i = run_op(dev, x, bs, n, r, seen)
    E = reference_error(x, bs, seen, r)
    start = np.abs(bs) >= 1e6                                  # the two classes of rows: E is the largest error of a row's class
    E = np.where(start, E[start].max() if start.any() else 0.0, E[~start].max() if (~start).any() else 0.0)
    worst = 0.0
    for b in range(B0):
        blk = slice(b * n, b * n + n)
        ref_s, ref_i, margin = br.select(x[blk].astype(np.float64), bs[blk].astype(np.float64), None if seen is None else seen[blk], r,
                                         round32=round32)
        if need_margin:
            assert margin >= ORDER_MARGIN, (what, b, margin)
        assert np.array_equal(got_i[b], ref_i), (what, b, got_i[b], ref_i)
        fin = np.isfinite(ref_s)
        assert np.array_equal(got_s[b][~fin], ref_s[~fin].astype(np.float32)), (what, b)
        err = np.abs(got_s[b][fin].astype(np.float64) - ref_s[fin])
        bound = np.maximum(8 * E[b * n + ref_i[fin] // V], np.spacing(np.abs(ref_s[fin]).astype(np.float32)).astype(np.float64))
        worst = max(worst, float((err / bound).max()) if err.size else 0.0)
        assert np.all(err <= bound), (what, b, err.max(), bound.min())
    print(f"beam_select {what} V={V} n={n} B0={B0}: reference fp32 error {E.max():.3e}, device error / bound {worst:.3f}")
    return got_s, got_i


def random_rows(V, n, B0, seed):
    """Rows whose restated order has the margin (seeds are walked on the CPU; the first that fits is deterministic)."""
    for s in range(seed, seed + 200):
        rng = np.random.default_rng(s)
        x = (rng.standard_normal((B0 * n, V)) * 3).astype(np.float32)
        bs = (-rng.random(B0 * n) * 4).astype(np.float32)
        if all(br.select(x[b * n:b * n + n].astype(np.float64), bs[b * n:b * n + n].astype(np.float64))[2] >= ORDER_MARGIN for b in range(B0)):
            return x, bs
    raise AssertionError("no seed with the margin")


@pytest.mark.parametrize("V", SIZES)
@pytest.mark.parametrize("n", BEAMS)
def test_random_rows_give_the_restated_candidates(dev, V, n):
    for B0 in (1, 3):
        x, bs = random_rows(V, n, B0, 1000 * n + V % 997)
        check(dev, x, bs, n, what="random")


@pytest.mark.parametrize("V", [40, 257, 16385])
@pytest.mark.parametrize("n", BEAMS)
def test_planted_winners(dev, V, n):
    rng = np.random.default_rng(V + n)
    base = (rng.standard_normal((n, V)) * 0.5).astype(np.float32)
    # all 2n winners in one beam: the others sit 50 below
    bs = np.full(n, -50.0, np.float32)
    bs[n - 1] = 0.0
    _, gi = check(dev, base, bs, n, what="one beam wins")
    assert np.all(gi[0] // V == n - 1)
    # one winner per beam: a spike of 20 in every row takes nearly all of its row's mass, the next n come from what is left
    x = base.copy()
    spikes = rng.choice(V, size=n, replace=False)
    x[np.arange(n), spikes] = 20.0
    bs = -0.125 * np.arange(n, dtype=np.float32)               # the spikes' scores: about 0, -0.125, ... -- far apart
    _, gi = check(dev, x, bs, n, need_margin=False, what="one winner per beam")
    assert sorted(gi[0][:n].tolist()) == sorted((np.arange(n) * V + spikes).tolist())
    # the start scores: one beam at 0, the others at -1e9, where fp32 holds multiples of 64 only
    bs = np.full(n, br.START, np.float32)
    bs[0] = 0.0
    gs, gi = check(dev, base, bs, n, round32=True, need_margin=False, what="start scores")
    assert np.all(gi[0][:min(2 * n, V)] // V == 0)


@pytest.mark.parametrize("V", [2, 3])
def test_start_scores_below_2n_columns_tie_by_flat_index(dev, V):
    n = 2
    x = np.asarray([[0.5, -0.25, 1.0][:V], [0.75, 2.0, -1.0][:V]], np.float32)
    bs = np.asarray([0.0, br.START], np.float32)
    gs, gi = check(dev, x, bs, n, round32=True, need_margin=False, what="start scores, V < 2n")
    assert gi[0][V:].tolist() == list(range(V, 2 * V))[:2 * n - V]             # beam 1's entries all round to -1e9: id ascending
    assert np.all(gs[0][V:] == np.float32(br.START))


@pytest.mark.parametrize("V", [40, 16385])
def test_equal_rows_with_equal_beam_scores_go_by_flat_index(dev, V):
    n = 3
    rng = np.random.default_rng(5)
    row = (rng.standard_normal(V) * 3).astype(np.float32)
    x = np.stack([row, rng.standard_normal(V).astype(np.float32), row])
    bs = np.asarray([-1.5, -40.0, -1.5], np.float32)
    gs, gi = check(dev, x, bs, n, need_margin=False, what="equal rows")
    top = np.argsort(-row.astype(np.float64), kind="stable")[:3]
    assert gi[0].tolist() == [int(f) for j in top for f in (j, 2 * V + j)]      # beam 0 before beam 2, pair by pair
    assert np.array_equal(gs[0][0::2], gs[0][1::2])                            # the same bits from either row


def test_rows_of_minus_inf_and_nan_with_fewer_than_2n_finite_entries(dev):
    n, V = 16, 40
    x = np.full((n, V), -np.inf, np.float32)
    x[:, 1::2] = np.nan
    x[3, [7, 9, 30]] = [1.0, 0.5, np.nan]
    x[10, [0, 39]] = [0.25, 2.0]
    bs = np.zeros(n, np.float32)
    gs, gi, cs, ci = run_op(dev, x, bs, n, rows=True)
    ref_s, ref_i, _ = br.select(x.astype(np.float64), bs.astype(np.float64))
    assert np.array_equal(gi[0], ref_i)
    assert gi[0][:4].tolist() == [10 * V + 39, 3 * V + 7, 3 * V + 9, 10 * V + 0]
    assert gi[0][4:].tolist() == list(range(28)) and np.all(np.isneginf(gs[0][4:]))     # nothing finite left: the flat index orders
    assert np.allclose(gs[0][:4], ref_s[:4], rtol=0, atol=1e-6)
    # a row's own list: its finite entries, then ids ascending at -inf
    assert ci[3].tolist()[:2] == [7, 9] and ci[3].tolist()[2:] == [j for j in range(V) if j not in (7, 9)][:30]
    assert ci[0].tolist() == list(range(32)) and np.all(np.isneginf(cs[0]))


@pytest.mark.parametrize("V", [40, 16385])
def test_a_seen_bit_on_the_would_be_winner_under_a_penalty(dev, V):
    n = 2
    rng = np.random.default_rng(V)
    x = (rng.standard_normal((n, V)) * 0.5).astype(np.float32)
    x[0, 11] = 6.0                                             # the winner without the penalty
    x[1, 5] = -0.1
    seen = np.zeros((n, V), bool)
    seen[0, 11] = True                                         # 6 / 8 = 0.75 falls behind
    seen[1, 5] = True                                          # a negative logit is multiplied
    x[0, 20] = 3.0
    bs = np.zeros(n, np.float32)
    _, plain = check(dev, x, bs, n, need_margin=False, what="no penalty")
    _, pen = check(dev, x, bs, n, r=8.0, seen=seen, need_margin=False, what="penalty 8")
    assert plain[0][0] == 11 and pen[0][0] == 20 and pen[0][1] != 11          # 0.75 is behind other rows' best as well
    _, off = check(dev, x, bs, n, r=1.0, seen=seen, need_margin=False, what="penalty 1")
    assert np.array_equal(off, plain)


@pytest.mark.parametrize("V", [257, 16385])
def test_a_prompt_alone_and_inside_a_batch_of_three_give_the_same_bits(dev, V):
    n = 3
    x, bs = random_rows(V, n, 3, 77)
    s3, i3, cs3, ci3 = run_op(dev, x, bs, n, rows=True)
    for b in range(3):
        blk = slice(b * n, b * n + n)
        s1, i1, cs1, ci1 = run_op(dev, x[blk], bs[blk], n, rows=True)
        assert np.array_equal(s1[0].view(np.uint32), s3[b].view(np.uint32)) and np.array_equal(i1[0], i3[b])
        assert np.array_equal(cs1.view(np.uint32), cs3[blk].view(np.uint32)) and np.array_equal(ci1, ci3[blk])


def test_arguments_are_checked(dev):
    from rag4dyg_amd import ops
    x = torch.zeros(4, 8, device=dev)
    bs = torch.zeros(4, device=dev)
    for bad in (dict(num_beams=1), dict(num_beams=17), dict(num_beams=3), dict(num_beams=2, repetition_penalty=0.5)):
        with pytest.raises(ValueError):
            ops.beam_select(x, bs, **bad)
    with pytest.raises(ValueError):
        ops.beam_select(torch.zeros(4, 1, device=dev), bs, 2)                   # n * V < 2n
