"""Shared reference, input generator, case table and yardstick of the loss-head edge tests (``test_host_loss_head.py`` on the CPU,
``test_gpu_loss_head.py`` on the device, ``oracle/gen_golden.py g14`` for the reference-pinned fixture).  Nothing here touches
the GPU.

``loss_head`` restates ``CLtime_loss`` + ``alpha * info_nce`` (``oracle/train_ref.py``) with three [B, B] matrix products in place
of the oracle's [3B, 3B, d] cosine tensor (0.9 GB in float64 at B = 129, d = 768) and accepts B = 1, where the oracle -- like
the reference -- raises (its ``.squeeze()`` leaves a 0-d decay "matrix").  The host file pins it to the oracle at 1e-12."""
import functools
from collections import namedtuple

import numpy as np
import torch

EPS = 1e-8                                                        # F.cosine_similarity's clamp on each norm


def loss_head(tau, lam, alpha, emb, ta, tp, tn):
    """(CLtime, alpha * info_nce) of ``emb`` [5, B, d] (anchors, positives, hard negatives, two views) in ``emb``'s dtype;
    the times are [B] or [B, 1]."""
    a, p, n, s1, s2 = emb
    B = a.shape[0]
    ta, tp, tn = (t.reshape(-1).to(emb.dtype) for t in (ta, tp, tn))

    def unit(x):
        return x / x.norm(dim=1, keepdim=True).clamp_min(EPS)

    def decay(t):
        return torch.exp(-lam * torch.abs(ta[:, None] - t[None, :]))
    ua = unit(a)
    d_neg = decay(ta) * (1.0 - torch.eye(B, dtype=emb.dtype))     # the zeroed logit stays in the softmax
    logits = torch.cat([ua @ unit(p).T * decay(tp), ua @ ua.T * d_neg, ua @ unit(n).T * decay(tn)], dim=1) / tau
    cl = torch.nn.functional.cross_entropy(logits, torch.arange(B))
    z = torch.cat([s1, s2], dim=0)
    sim = (z @ z.T / tau).masked_fill(torch.eye(2 * B, dtype=torch.bool), float("-inf"))
    partner = torch.cat([torch.arange(B) + B, torch.arange(B)])
    return cl, alpha * torch.nn.functional.cross_entropy(sim, partner)


# ---------------------------------------------------------------------------------------------------------------- inputs
REGIMES = ("unit", "gauss", "pooled", "dups", "zero", "tgap", "tsame")
SCALES = (1.0, 7.0, 0.2)                                           # anchors, positives, hard negatives: a wrong norm index shows
DUPS_COMMON = 3.0
T_OFFSETS = (0.0, 3.0, 11.0)                                       # ta, tp, tn: a wrong time vector shows


SEED = 3                                                           # chosen once on the CPU: of seeds 0..9 the one at which the float32
#                                                                    reference leaves the unit / dups / zero cases the widest margin
#                                                                    under the caps (worst K * element-wise ratio 0.60; the tiny shapes
#                                                                    scatter up to 1.8 with the draw) -- before any device run


def make_inputs(regime, B, d, seed=SEED):
    """(emb [5, B, d] float32, ta, tp, tn [B, 1] float32) of one regime, deterministic in (regime, B, d, seed)."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * B + d + 101 * REGIMES.index(regime))
    blocks = [torch.randn(B, d, generator=g) for _ in range(5)]
    times = [torch.rand(B, 1, generator=g) * 30 + off for off in T_OFFSETS]
    if regime == "pooled":                                         # what mean-pooling a trained encoder gives: near-collinear rows
        common = torch.randn(1, d, generator=g) * 3
        blocks = [common + 0.05 * x for x in blocks]
    if regime == "dups":                                           # correlated rows (cosines near 0.9): with independent rows an exact
        common = torch.randn(1, d, generator=g) * DUPS_COMMON      # duplicate saturates both softmaxes and leaves rounding noise
        blocks = [common + x for x in blocks]
    if regime in ("unit", "dups"):
        blocks[3:] = [torch.nn.functional.normalize(x, dim=1) for x in blocks[3:]]
    blocks[:3] = [x * s for x, s in zip(blocks[:3], SCALES)]
    if regime == "dups":
        if B > 1:
            blocks[0][1] = blocks[0][0]
        blocks[1] = blocks[0].clone()                              # p == a (and with it the positives' scale)
        blocks[4] = blocks[3].clone()
        times[1] = times[0].clone()
    if regime == "zero":
        for k, r in ((0, 0), (1, 1 % B), (2, 2 % B), (3, 0)):
            blocks[k][r] = 0
    if regime == "tgap":
        times = [t * 1e5 for t in times]
    if regime == "tsame":
        times = [torch.full((B, 1), 12.5) for _ in times]
    return (torch.stack(blocks).contiguous(),) + tuple(times)


# ---------------------------------------------------------------------------------------------------------------- cases
# (B, d): 2B and B against the 16 waves of the softmax kernel, 3B and 2B against 64 lanes, d against 64 lanes and 256 threads,
# d up to the accepted maximum.
SHAPES = ((1, 7), (1, 64), (2, 3), (3, 65), (8, 64), (9, 64), (16, 256), (17, 63), (21, 65), (22, 130), (32, 255), (33, 1),
          (63, 257), (64, 256), (65, 257), (129, 768), (257, 64), (5, 1024), (3, 8192))
TAUS, LAMS, ALPHA_SCALES = (0.07, 1.0, 0.01), (0.05, 0.0, 5.0), ((1.0, 1.0), (0.3, 0.25), (0.0, 1.0))
CROSS_SHAPES = ((2, 3), (9, 64), (17, 63), (21, 65))               # the full hyper-parameter cross runs on these
Case = namedtuple("Case", "regime B d tau lam alpha gscale")
# beside the rotation: the training scripts' own hyper-parameters on what mean-pooling gives at the wikiv2 width.  (``dups`` stays
# at B <= 21: at B = 65 and 257 the float32 reference's element-wise ratio is 0.10 - 0.13, no longer K below the cap.)
EXTRA = (Case("pooled", 129, 768, 0.07, 0.05, 1.0, 1.0), Case("gauss", 129, 768, 0.07, 0.05, 0.3, 0.25))


def _regime(i, tau, lam):
    """The i-th regime of the rotation.  ``dups`` is not paired with tau = 0.01 or lam = 5: the duplicate's logit then stands alone,
    both softmaxes saturate and the float64 gradient is itself ~1e-5 of its terms -- float32 rounding noise, no yardstick."""
    r = REGIMES[i % 7]
    return "zero" if r == "dups" and (tau == 0.01 or lam == 5.0) else r


def _cases():
    out = []
    for k, (B, d) in enumerate(SHAPES):                            # every shape: unit + two rotating regimes, rotating hypers
        for j, r in enumerate(dict.fromkeys((0, k % 7, (k + 2) % 7))):
            i = k + j
            alpha, gs = ALPHA_SCALES[i % 3]
            tau, lam = TAUS[(i // 3) % 3] if j else 0.07, LAMS[i % 3]
            regime = _regime(r, tau, lam)
            if d == 1:
                # Every cosine is +-1 at d = 1: the float64 CLtime gradient is identically zero, and what a float32 evaluation
                # returns is cancellation residue, ~eps32 x its terms (~1 / (B tau |x|), |x| as small as a Gaussian draw gets).
                # torch's autograd projects with u = +-1 and cancels EXACTLY, so e_ref does not price that residue: with all
                # decays at 1 (tsame, tau 1) the device's is 6e-7 absolute = 2.2e-5 of the views' gradient against e_ref 3e-7.
                # d = 1 therefore runs where the decays suppress the CLtime terms (lam = 5, times apart) and the views'
                # gradient sets the scale: the case checks the d = 1 trip of every loop, the views and the three losses.
                alpha, gs = ALPHA_SCALES[0]
                lam = 5.0
                regime = "tgap" if regime == "tsame" else regime
            c = Case(regime, B, d, tau, lam, alpha, gs)
            if c not in out:
                out.append(c)
    for c in EXTRA:
        if c not in out:
            out.append(c)
    i = 0
    for B, d in CROSS_SHAPES:                                      # the full cross, the regime rotating through it
        for tau in TAUS:
            for lam in LAMS:
                for alpha, gs in ALPHA_SCALES:
                    c = Case(_regime(i, tau, lam), B, d, tau, lam, alpha, gs)
                    i += 1
                    if c not in out:
                        out.append(c)
    return out


CASES = _cases()


def case_id(c):
    return f"{c.regime}-B{c.B}-d{c.d}-tau{c.tau:g}-lam{c.lam:g}-a{c.alpha:g}-s{c.gscale:g}"


CASE_IDS = [case_id(c) for c in CASES]


def evaluate(c, dtype, inputs=None):
    """``loss_head`` and autograd of ``gscale * (cl + alpha * nce)`` in ``dtype``: (losses [3] float64 numpy, grad [5, B, d] float64
    numpy).  The float32 inputs are the same in both dtypes."""
    emb, ta, tp, tn = inputs if inputs is not None else make_inputs(c.regime, c.B, c.d)
    leaf = emb.to(dtype).requires_grad_(True)
    cl, au = loss_head(c.tau, c.lam, c.alpha, leaf, ta, tp, tn)
    tot = cl + au
    (tot * c.gscale).backward()
    return np.array([cl.item(), au.item(), tot.item()], np.float64), leaf.grad.double().numpy()


def loss_err(got, ref):
    """max over the three losses of |got - ref| / max(1, |ref|)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


Yardstick = namedtuple("Yardstick", "losses64 grad64 e_ref lerr_ref ew_ref caps")


@functools.lru_cache(maxsize=None)
def yardstick(c):
    """The float64 truth of a case and the float32 reference's own errors against it: ``e_ref`` (max-norm gradient error),
    ``lerr_ref`` (loss error over max(1, |loss|)), ``ew_ref`` (``conftest.elementwise_err``), and ``caps``: whether the case also
    carries the fixed caps (element-wise ratio < 1, loss error < 1e-5) -- only where the float32 reference meets them with K to
    spare.  Computed from the reference alone."""
    from _training_stress_cases import K
    from conftest import elementwise_err, rel_err
    l64, g64 = evaluate(c, torch.float64)
    l32, g32 = evaluate(c, torch.float32)
    ew = elementwise_err(g32, g64)
    lerr = loss_err(l32, l64)
    caps = bool(K * ew < 1 and K * lerr < 1e-5)
    return Yardstick(l64, g64, rel_err(g32, g64), lerr, ew, caps)


def bounds(c):
    """(gradient max-norm bound, loss bound) of the yardstick form  e_dev <= K * max(e_ref, E_FLOOR)."""
    from _training_stress_cases import E_FLOOR, K
    y = yardstick(c)
    return K * max(y.e_ref, E_FLOOR), K * max(y.lerr_ref, E_FLOOR)


# ---------------------------------------------------------------------------------------------------------------- g14 fixture
G14_SHAPES = ((2, 3), (3, 65), (17, 63))                           # every regime; plus (65, 80) for ``unit`` only
G14_HYPERS = ((0.07, 0.05), (1.0, 0.0), (0.01, 5.0))               # (tau, lam), rotating
# A float32 value pins another float32 implementation at 1e-5 only where float32 resolves it.  The raw info_nce logits of ``pooled``
# views are ~9 d / tau: at d = 65, tau = 0.07 one ulp of a logit is 1e-3 and the reference's own value lies 1.0e-5 from float64 (5.5e-6
# at B = 17, d = 63 and 1.6e-6 at B = 3, d = 65 with tau = 1).  ``pooled`` is therefore pinned at tau = 1 and d <= 9; ``gen_golden.py g14`` refuses
# any entry whose reference value is not within 1e-5 / 4 of float64 (near-collinear views leave 1.5e-6 even there).
G14_POOLED = {(2, 3): (2, 3, 1.0, 0.05), (3, 65): (3, 9, 1.0, 0.0), (17, 63): (17, 7, 1.0, 5.0)}


def g14_entries():
    """[(tag, regime, B, d, tau, lam)] of ``tests/golden/g14_loss_head_edges.npz``."""
    out, i = [], 0
    for B, d in G14_SHAPES:
        for regime in REGIMES:
            tau, lam = G14_HYPERS[i % 3]
            i += 1
            if regime == "pooled":
                B_, d_, tau, lam = G14_POOLED[(B, d)]
                out.append((f"{regime}_B{B_}_d{d_}", regime, B_, d_, tau, lam))
            else:
                out.append((f"{regime}_B{B}_d{d}", regime, B, d, tau, lam))
    out.append(("unit_B65_d80", "unit", 65, 80, 0.07, 0.05))
    return out
