"""Float64 restatement of the reference's greedy beam search (``models/modeling_utils.py:929-1153``, ``BeamHypotheses``
``:1205-1252``) for the beam tests: the single selection (``select``), the hypothesis list (``Hyps``), the search loop over any
source of next-token logits (``beam_search``) and the last step (``finalize``).  Every decision records its MARGIN in
log-probability, so that a fixture can demand that no decision is close enough for fp32 to turn it.

The tie rule is the library's (include/r4d.h, "Beam search"): candidates in the order (score descending, flat index
``beam * V + id`` ascending); among hypotheses of equal score the earliest arrival leaves first and the latest is returned first.
"""
import numpy as np

START = -1e9                      # beams 1 .. n-1 of a prompt start here (:956-959)
MARGIN = 1e-3                     # what the fixture demands of every decision


def penalise(x, seen, r):
    """The repetition penalty (``enforce_repetition_penalty_``): seen ids are multiplied (negative) or divided (positive) by r."""
    x = np.array(x, dtype=np.float64)
    if seen is not None and r != 1.0:
        s = np.asarray(seen, dtype=bool)
        x[s] = np.where(x[s] < 0, x[s] * r, x[s] / r)
    return x


def row_scores(x, beam_score, seen=None, r=1.0):
    """log_softmax of the penalised row + the beam score; NaN counts as -inf, going in and coming out."""
    x = penalise(x, seen, r)
    x[np.isnan(x)] = -np.inf
    m = x.max()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = ((x - m) - np.log(np.exp(x - m).sum())) + np.float64(beam_score)
    s[np.isnan(s)] = -np.inf
    return s


def select(logits, beam_scores, seen=None, r=1.0, k=None, round32=False):
    """One prompt: ``logits`` [n, V], ``beam_scores`` [n].  Returns (scores [k], flat indices [k], margin): the k = 2n best in the
    order (score descending, flat index ascending); margin = the smallest gap between neighbours among the best k + 1, gaps of
    exactly 0 (equal scores, which the flat index orders) left out.  ``round32``: the scores are rounded to fp32 before they are
    ordered -- for planted rows whose fp32 scores are known to coincide, such as the rows that start at -1e9."""
    n, V = logits.shape
    k = 2 * n if k is None else k
    s = np.concatenate([row_scores(logits[i], beam_scores[i], None if seen is None else seen[i], r) for i in range(n)])
    if round32:
        s = s.astype(np.float32).astype(np.float64)
    order = np.lexsort((np.arange(s.size), -s))[:k + 1]
    top = s[order]
    with np.errstate(invalid="ignore"):
        gaps = top[:-1] - top[1:]
    gaps = gaps[np.isfinite(gaps) & (gaps > 0)]
    return top[:k], order[:k].astype(np.int64), (float(gaps.min()) if gaps.size else np.inf)


class Hyps:
    """The n-best list of one prompt.  ``beams``: [score, ids] in order of arrival; ``margin``: the closest ``score > worst`` /
    ``worst >= cur`` decision so far; ``displaced``: entries that had to leave."""

    def __init__(self, n, max_length, length_penalty):
        self.n, self.limit, self.lp = n, max_length - 1, float(length_penalty)
        self.beams, self.worst, self.margin, self.displaced = [], 1e9, np.inf, 0

    def add(self, ids, sum_logprobs):
        score = float(sum_logprobs) / len(ids) ** self.lp
        if len(self.beams) < self.n:
            self.beams.append((score, list(ids)))
            self.worst = min(self.worst, score)
            return
        self.margin = min(self.margin, abs(score - self.worst))
        if score > self.worst:
            self.beams.append((score, list(ids)))
            out = min(range(len(self.beams)), key=lambda i: (self.beams[i][0], i))
            del self.beams[out]
            self.displaced += 1
            self.worst = min(sc for sc, _ in self.beams)

    def is_done(self, best_sum_logprobs):
        if len(self.beams) < self.n:
            return False
        cur = float(best_sum_logprobs) / self.limit ** self.lp
        self.margin = min(self.margin, abs(self.worst - cur))
        return self.worst >= cur

    def best(self, k):
        ranked = sorted(self.beams, key=lambda h: h[0])
        sc = np.asarray([h[0] for h in ranked][-(k + 1):])                     # the sort decides among the best k + 1 only
        if sc.size > 1 and np.all(np.isfinite(sc)):
            self.margin = min(self.margin, float(np.min(np.diff(sc))))
        return [ranked.pop()[1] for _ in range(k)]


def finalize(hyps, n_ret, max_length, pad, eos):
    """:1120-1153.  Returns int64 [len(hyps) * n_ret, L]."""
    rows = [ids for h in hyps for ids in h.best(n_ret)]
    lens = [len(r) for r in rows]
    if min(lens) == max(lens):
        return np.asarray(rows, dtype=np.int64).reshape(len(rows), lens[0])
    assert pad is not None
    out = np.full((len(rows), min(max(lens) + 1, max_length)), pad, dtype=np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
        if len(r) < max_length:
            out[i, len(r)] = eos[0]
    return out


def beam_search(step_logits, prompts, n, max_length, eos=None, length_penalty=1.0, repetition_penalty=1.0, pad=None, n_ret=1):
    """``step_logits(rows)``: next-token logits [len(rows), V] (any float dtype) for a list of equally long id lists.  ``prompts``
    [B0, T].  Returns dict(ids int64 [B0 * n_ret, L], margin, stats) -- stats: prompts done early, hypotheses displaced, whether the
    output pads, prompts that end without a finished hypothesis."""
    prompts = [list(map(int, p)) for p in prompts]
    B0, T = len(prompts), len(prompts[0])
    eos = list(eos) if eos is not None else None
    if pad is None and eos is not None:
        pad = eos[0]
    rows = [list(p) for p in prompts for _ in range(n)]
    scores = np.tile(np.asarray([0.0] + [START] * (n - 1)), B0)
    hyps = [Hyps(n, max_length, length_penalty) for _ in range(B0)]
    done = [False] * B0
    margin, cur = np.inf, T
    while cur < max_length:
        logits = np.asarray(step_logits(rows), dtype=np.float64)
        V = logits.shape[1]
        new_rows, new_scores = [], []
        for b in range(B0):
            blk = slice(b * n, b * n + n)
            if done[b]:
                new_rows += [rows[b * n + i] + [pad if pad is not None else 0] for i in range(n)]
                new_scores += [0.0] * n
                continue
            seen = None
            if repetition_penalty != 1.0:
                seen = np.zeros((n, V), dtype=bool)
                for i in range(n):
                    seen[i, rows[b * n + i]] = True
            top, flat, gap = select(logits[blk], scores[blk], seen, repetition_penalty)
            if hyps[b].is_done(top[0]):
                done[b] = True
                new_rows += [rows[b * n + i] + [pad if pad is not None else 0] for i in range(n)]
                new_scores += [0.0] * n
                continue
            margin = min(margin, gap)
            took = 0
            for sc, f in zip(top, flat):
                beam, tok = int(f) // V, int(f) % V
                if eos is not None and tok in eos:
                    hyps[b].add(rows[b * n + beam], sc)
                else:
                    new_rows.append(rows[b * n + beam] + [tok])
                    new_scores.append(float(sc))
                    took += 1
                if took == n:
                    break
            assert took == n, "Beam should always be full"
        rows, scores = new_rows, np.asarray(new_scores)
        if all(done):
            break
        cur += 1
    unfinished = 0
    for b in range(B0):
        if not done[b]:
            unfinished += 0 if hyps[b].beams else 1
            for i in range(n):
                hyps[b].add(rows[b * n + i], scores[b * n + i])
    ids = finalize(hyps, n_ret, max_length, pad, eos)
    margin = min([margin] + [h.margin for h in hyps])
    lens = [len(r) for h in hyps for r in h.best(n_ret)]
    stats = dict(done_early=sum(done), displaced=sum(h.displaced for h in hyps), pads=bool(ids.shape[1] and (min(lens) != max(lens))),
                 unfinished=unfinished)
    return dict(ids=ids, margin=float(margin), stats=stats)


# ------------------------------------------------------------------------------------------------ the fixture's model and cases
N_LAYER, N_HEAD, N_EMBD, VOCAB, N_POSITIONS = 2, 2, 64, 40, 32
EOS = (5, 17, 29)                 # the boosted ids
WEIGHT_SEED, SCALE, BOOST = 16, 4.0, 2.0
FIXTURE = "g16_beam_search"


def make_weights():
    """The tiny model's state dict (fp32, reference layout, tied head): embeddings scaled so that the logits spread over a few
    units, and the rows of ``EOS`` moved along ln_f's shift -- hidden . row grows by about BOOST -- so that an eos is often among
    the best 2n."""
    from oracle import gpt2_ref
    sd = gpt2_ref.make_state_dict(N_LAYER, N_EMBD, VOCAB, n_positions=N_POSITIONS, seed=WEIGHT_SEED, random_affine=True)
    wte = sd["transformer.wte.weight"]
    wte *= SCALE
    b = sd["transformer.ln_f.bias"]
    for e in EOS:
        wte[e] += BOOST * b / float(b @ b)
    sd["lm_head.weight"] = wte
    return sd


def weights_from(g):
    """The state dict out of the fixture ``g`` (``np.load``), head tied."""
    import torch
    sd = {k[len("weights/"):]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith("weights/")}
    sd["lm_head.weight"] = sd["transformer.wte.weight"]
    return sd


def logits_fn(sd, n_head=N_HEAD):
    """``step_logits`` of ``beam_search`` from the float64 forward of oracle/gpt2_ref.py over the whole rows (no cache)."""
    import torch
    from oracle import gpt2_ref
    sd64 = {k: v.double() for k, v in sd.items()}

    def step(rows):
        return gpt2_ref.gpt2_forward(sd64, torch.tensor(rows, dtype=torch.long), n_head)["logits"][:, -1].numpy()
    return step


# name -> (prompt seed, B0, T, generate's arguments)
CASES = {
    "n2_one_eos":        (8, 3, 5, dict(num_beams=2, max_length=14, eos_token_ids=[5])),
    "n3_three_eos_lp06": (5, 2, 4, dict(num_beams=3, max_length=16, eos_token_ids=[5, 17, 29], length_penalty=0.6)),
    "n4_lp2_return_all": (347, 2, 6, dict(num_beams=4, max_length=12, eos_token_ids=[5], length_penalty=2.0, num_return_sequences=4)),
    "n16_single_prompt": (4, 1, 3, dict(num_beams=16, max_length=7, eos_token_ids=[5])),
    "n3_no_eos":         (5, 2, 4, dict(num_beams=3, max_length=10)),
    "n4_penalty_13":     (6, 2, 5, dict(num_beams=4, max_length=14, eos_token_ids=[5], repetition_penalty=1.3, num_return_sequences=2)),
    "n2_one_token":      (7, 2, 1, dict(num_beams=2, max_length=8, eos_token_ids=[17], pad_token_id=0)),
    "n3_one_step":       (8, 2, 6, dict(num_beams=3, max_length=7, eos_token_ids=[5])),
}


def case_inputs(case):
    """(prompts as lists [B0][T], generate's keyword arguments) of a ``CASES`` entry: ids drawn below the vocabulary, no eos among them."""
    seed, B0, T, kw = case
    rng = np.random.default_rng(seed)
    free = np.asarray([i for i in range(VOCAB) if i not in EOS])
    return rng.choice(free, size=(B0, T)).tolist(), dict(kw)


# ------------------------------------------------------------------------------------------------ a second shape, no fixture
# (tests/test_gpu_beam_generate.py: the restatement driven by the project's own forward.)  The seeds are those whose margin under
# the float64 forward of oracle/gpt2_ref.py is at least 3e-3: under the device's fp32 logits nearly all keep 1e-3.
INDEPENDENT = dict(n_layer=2, n_head=4, d=256, V=1000, n_positions=32, T=5, max_length=24, n=4, eos=[7], length_penalty=0.8,
                   weight_seed=31, seeds=(10, 81, 111, 126, 150, 152, 163, 166, 218, 221))


def independent_weights():
    from oracle import gpt2_ref
    I = INDEPENDENT
    sd = gpt2_ref.make_state_dict(I["n_layer"], I["d"], I["V"], n_positions=I["n_positions"], seed=I["weight_seed"], random_affine=True)
    wte = sd["transformer.wte.weight"]
    wte *= 3.0
    b = sd["transformer.ln_f.bias"]
    for e in I["eos"]:
        wte[e] += 3.0 * b / float(b @ b)
    sd["lm_head.weight"] = wte
    return sd


def independent_prompts(seed):
    I = INDEPENDENT
    rng = np.random.default_rng(seed)
    free = np.asarray([i for i in range(I["V"]) if i not in I["eos"]])
    return rng.choice(free, size=(2, I["T"])).tolist()
