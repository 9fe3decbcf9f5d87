"""The sampler of include/r4d.h ("Sampled decoding") restated in numpy, for tests/test_host_sampling.py,
tests/test_gpu_sampling.py and tools/gen_sampling_fixture.py.

Steps 1-3 (repetition penalty, temperature) are single IEEE fp32 operations and are done in fp32 here, as the header defines them;
everything after them -- thresholds, weights, cumulative masses, the draw -- is float64.  ``philox_u`` is Philox-4x32-10 with the
kernel's counter and key layout.
"""
import numpy as np

SITE = 0x53414D50
GRID = [(k, p, t, r) for k in (0, 1, 5, 50) for p in (1.0, 0.9, 0.5) for t in (0.7, 1.0, 1.5) for r in (1.0, 1.3)]
FIXTURE_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 16384)
ALL_SIZES = FIXTURE_SIZES + (16385, 50257)
P_MARGIN, K_MARGIN = 1e-4, 1e-5


def philox4x32_10(c, k):
    """Philox-4x32-10 (Salmon et al., SC'11): ``c`` four and ``k`` two uint64 arrays holding 32-bit words -> four output words."""
    m32 = np.uint64(0xFFFFFFFF)
    c = [np.asarray(v, dtype=np.uint64) & m32 for v in c]
    k0, k1 = (np.asarray(v, dtype=np.uint64) & m32 for v in k)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c


def philox_u(seed, stream, step):
    """(u as float64 = (word >> 8) * 2^-24, the 32-bit word) for arrays (or scalars) of stream and step numbers."""
    stream, step = np.broadcast_arrays(np.asarray(stream, dtype=np.int64), np.asarray(step, dtype=np.int64))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10([step.astype(np.uint64), stream.astype(np.uint64), np.zeros(step.shape, np.uint64), np.full(step.shape, SITE, np.uint64)],
                      [np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)])[0]
    return (w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24, w


def make_logits(V, seed):
    """Tie-free seeded logits and a seen mask for one vocabulary size: normal draws, wide enough that the top-p cuts of the
    grid fall between well separated masses also at the large sizes."""
    rng = np.random.default_rng(seed)
    scale = 3.0 if V <= 300 else 10.0
    x = (rng.standard_normal(V) * scale).astype(np.float32)
    while True:                                                      # fp32 normals repeat among 50,257 draws: redraw the repeats
        first = np.unique(x, return_index=True)[1]
        if first.size == V:
            break
        dup = np.setdiff1d(np.arange(V), first)
        x[dup] = (rng.standard_normal(dup.size) * scale).astype(np.float32)
    seen = rng.random(V) < 0.2
    return x, seen


def pack_bits(mask):
    """bool [.., V] -> uint32 words [.., ceil(V/32)], bit j % 32 of word j / 32."""
    mask = np.asarray(mask, dtype=bool)
    V = mask.shape[-1]
    pad = (-V) % 32
    m = np.concatenate([mask, np.zeros(mask.shape[:-1] + (pad,), bool)], -1)
    return np.packbits(m.reshape(mask.shape[:-1] + (-1, 32)), axis=-1, bitorder="little").view(np.uint32)[..., 0]


def unpack_bits(words, V):
    words = np.ascontiguousarray(np.asarray(words).view(np.uint32))
    return np.unpackbits(words.view(np.uint8), axis=-1, bitorder="little").reshape(words.shape[:-1] + (-1,))[..., :V].astype(bool)


def transform(x, seen, do_sample, tau, r):
    """Steps 1 and 3 in fp32, NaN as -inf."""
    x = np.asarray(x, dtype=np.float32).copy()
    if seen is not None and r != 1:
        s = np.asarray(seen, dtype=bool)
        with np.errstate(all="ignore"):
            x[s] = np.where(x[s] < 0, x[s] * np.float32(r), x[s] / np.float32(r))
    if do_sample and tau != 1:
        with np.errstate(all="ignore"):
            x = x / np.float32(tau)
    return np.where(np.isnan(x), -np.inf, x).astype(np.float32)


def sample_row(x, seen=None, do_sample=True, tau=1.0, top_k=0, top_p=1.0, r=1.0, seed=0, stream=0, step=0):
    """One row.  Returns dict(keep bool [V], token, u, w float64 [V] (weights of the kept set, 0 elsewhere), C (their inclusive
    prefix sums in index order), Z, p_margin / k_margin (how far the nearest cumulative mass / logit is from its cut))."""
    y = transform(x, seen, do_sample, tau, r).astype(np.float64)
    V = y.size
    u, _ = philox_u(seed, stream, step)
    u = float(u)
    ymax = y.max()
    first_max = int(np.argmax(y))
    out = dict(u=u, p_margin=np.inf, k_margin=np.inf)
    if not do_sample or not np.isfinite(ymax):
        keep = np.zeros(V, bool)
        keep[first_max] = True
        w = keep.astype(np.float64)
        out.update(keep=keep, token=first_max, w=w, C=np.cumsum(w), Z=1.0)
        return out
    keep = np.ones(V, bool)
    if top_k > 0:
        kk = min(max(int(top_k), 1), V)
        thr = np.sort(y)[V - kk]
        keep &= y >= thr
        off = y[(y != thr) & np.isfinite(y)]
        if off.size:
            out["k_margin"] = float(np.min(np.abs(off - thr)) / max(abs(thr), 1e-30))
    w = np.exp(y - ymax)
    if top_p < 1:
        tp = float(np.float32(top_p))
        idx = np.nonzero(keep)[0]
        order = idx[np.lexsort((idx, -y[idx]))]                      # value descending, index ascending
        ws = w[order]
        cum = np.cumsum(ws)
        before = cum - ws                                            # the mass of the i entries in front of the i-th
        k2 = before <= tp * cum[-1]
        k2[0] = True
        keep = np.zeros(V, bool)
        keep[order[k2]] = True
        if order.size > 1:
            out["p_margin"] = float(np.min(np.abs(before[1:] / cum[-1] - tp)))
    w = np.where(keep, w, 0.0)
    C = np.cumsum(w)
    Z = float(C[-1])
    hit = np.nonzero(keep & (C > u * Z))[0]
    token = int(hit[0]) if hit.size else int(np.nonzero(keep)[0][-1])
    out.update(keep=keep, token=token, w=w, C=C, Z=Z)
    return out


def eps_of(V):
    """The draw's tolerance (the issue's): (V / 64 + 256) * 2^-24."""
    return (V / 64 + 256) * 2.0 ** -24


def draw_ok(token, ref):
    """The chosen id is kept and u * Z lies in its interval of the index-order prefix sums, widened by eps * Z on both sides."""
    V = ref["keep"].size
    e = eps_of(V) * ref["Z"]
    t = int(token)
    if not (0 <= t < V) or not ref["keep"][t]:
        return False
    uz = ref["u"] * ref["Z"]
    return ref["C"][t] - ref["w"][t] - e <= uz < ref["C"][t] + e


def near_boundary(ref):
    """True when u * Z is within eps * Z of a boundary between two kept ids (the restatement cannot name the token alone)."""
    e = eps_of(ref["keep"].size) * ref["Z"]
    return bool(np.any(np.abs(ref["C"][ref["keep"]] - ref["u"] * ref["Z"]) <= e))


def grid_margins_ok(x, seen):
    for k, p, t, r in GRID:
        res = sample_row(x, seen, True, t, k, p, r)
        if res["p_margin"] <= P_MARGIN or res["k_margin"] <= K_MARGIN:
            return False
    return True


def frequency_case():
    """The 8-token distribution, seed and uniforms of the frequency test (GPU test 5), with the restatement's own tokens."""
    p = np.array([0.30, 0.22, 0.16, 0.12, 0.08, 0.06, 0.04, 0.02])
    x = np.log(p).astype(np.float32)
    n, seed = 65536, 20240
    u, _ = philox_u(seed, np.arange(n), 0)
    base = sample_row(x)
    C, Z = base["C"], base["Z"]
    tok = np.searchsorted(C, u * Z, side="right")                      # the lowest index whose prefix exceeds u Z
    near = np.min(np.abs(C[None, :] - (u * Z)[:, None]), axis=1) <= eps_of(8) * Z
    return x, p, n, seed, tok, near, base["w"] / Z


# the first seed of make_logits, per size, whose row passes grid_margins_ok (found by tools/gen_sampling_fixture.py, which asserts it)
SEEDS = {1: 0, 2: 0, 63: 0, 64: 0, 65: 0, 255: 0, 256: 1, 257: 0, 16384: 2, 16385: 2, 50257: 0}
