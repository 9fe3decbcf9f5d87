"""Planted inputs, references and a structural emulation for the encoder attention kernels (test infra only, CPU torch).

``plant`` builds a packed c_attn output ``qkv`` [B, T, 3 H hd] whose attention LOGITS are chosen, not drawn.  The logits are low
rank, so that every query of a sequence sees the chosen profile at once: ``q[..., 0] = sqrt(hd)`` and ``k[..., 0] = c_j`` give
key j the logit c_j for every query, ``q[..., 1] = sqrt(hd) a_i`` and ``k[..., 1] = b_j`` add ``a_i b_j``; the other head
columns of q and k hold 0.05 * randn (logit noise of about 0.0025 sqrt(hd)) and v is randn.  Everything is generated in float64
and rounded to float32 once: every reference reads the rounded values, so the planting need not be exact.

``attn_ref`` is the dense reference built on ``oracle/gpt2_ref.attn_core`` (float64: the bar; float32: the yardstick for what
fp32 itself costs).  ``attn_tiled`` restates the STRUCTURE of the fused kernels in float64 -- 32-query tiles, a per-query online
softmax over 32-key tiles, the four key-split states and their merge, or 128-key super-tiles on one state -- and can switch on
one seeded mistake (``DEFECTS``): tests/test_host_attention_planted.py shows with it, without a GPU, that each such mistake moves
a planted case by 10x or more of the bound tests/test_gpu_attention_planted.py holds the device to."""
import math

import numpy as np
import torch

from conftest import elementwise_err, rel_err
from oracle import gpt2_ref

PATTERNS = ("flat", "up", "steep", "down", "spike", "wide", "dead", "zigzag")
STEEP_MAX_T = 160                                   # c_j = 0.5 j: logits of 80 at T = 160, beyond that fp32 exp runs out of range
FORMS = ("keysplit", "colsplit")
DEFECTS = ("drop_tile_last", "double_tile_first", "no_rescale", "mask_lt", "merge_unweighted", "leak_next")
SPIKE_KEYS = (31, 32, 127, 128, -1, 0, 33, 129, 255, 256)      # -1: the last key, T - 1
# `up`: every key of an early query has a logit near -UP_AMP, a raw dot product of sqrt(hd) * UP_AMP; a 256-term fp32 sum rounds
# each addition at that magnitude.  At 30 (raw 480, ulp 3e-5) the float32 CPU evaluation ALONE reaches elementwise_err 1.1 - 1.4 at
# head_dim 256 (measured over six seeds; 0.63 at 16, the next binade down), so the amplitude is 15 and the bound stays.
UP_AMP = 15.0
DEAD_TILES = ((0, 32), (64, 96))
DEAD_SUPER_TILES = ((128, 256), (256, 384))
REL_BOUND, ELT_BOUND, YARDSTICK_FACTOR = 2e-5, 1.0, 4.0        # the device's bound: max(project bound, 4 x the float32 yardstick)


def patterns_for(T):
    return tuple(p for p in PATTERNS if p != "steep" or T <= STEEP_MAX_T)


def spike_key(b, h, H, T):
    """The key of (sequence b, head h) that ``spike`` gives the logit 12: the last key of a 32-key tile or of a 128-key
    super-tile, the first key of the next one, the last key, key 0 -- cyclically, clipped to T - 1."""
    s = SPIKE_KEYS[(b * H + h) % len(SPIKE_KEYS)]
    return T - 1 if s < 0 else min(s, T - 1)


def dead_ranges(b, h, T):
    """Key ranges of (sequence b, head h) whose K rows ``dead`` makes identical, with the logit -200: two whole 32-key tiles
    and one whole 128-key super-tile, clipped to T."""
    rs = DEAD_TILES + (DEAD_SUPER_TILES[(b + h) % 2],)
    return [(lo, min(hi, T)) for lo, hi in rs if lo < T]


@torch.no_grad()
def plant(B, T, H, hd, pattern, generator):
    """``qkv`` float32 [B, T, 3 H hd] with the logits of ``pattern``:

        flat    q = 0, v[..., 0] = 1, v[..., 1] = j     output row i is the plain mean over keys 0..i: column 0 = 1, column 1 = i / 2
        up      c_j = -15 + 15 j / T                    every tile raises the running maximum (-30 + 30 j / T put the fp32
                                                        yardstick itself over elementwise_err 1 at head_dim 256: see UP_AMP)
        steep   c_j = 0.5 j  (T <= 160)                 earlier tiles shrink by e^-16 per tile: a rescale factor far from 1
        down    c_j = -30 j / T                         the maximum is in the first tile, later rescales are almost 1
        spike   c_j = 0.5 randn, one key (``spike_key``) at 12 with its v slice x 4
        wide    c_j = -100 rand                         whole groups of keys underflow to weight 0
        dead    c_j = 0.5 randn, but K = (-200, 0, 0, ...) exactly on ``dead_ranges``: a first tile later rescaled by exactly 0,
                whole key-split states and a whole super-tile of weight 0; queries inside the first tile see identical keys
        zigzag  a_i = +1 / -1 for even / odd i, b_j = 20 (j / T - 0.5): neighbouring queries have their maximum on the diagonal
                key and on key 0 in turn"""
    assert pattern in PATTERNS, pattern
    assert pattern != "steep" or T <= STEEP_MAX_T, (pattern, T)
    assert hd >= 2
    f64 = dict(dtype=torch.float64, generator=generator)
    q = 0.05 * torch.randn(B, T, H, hd, **f64)
    k = 0.05 * torch.randn(B, T, H, hd, **f64)
    v = torch.randn(B, T, H, hd, **f64)
    j = torch.arange(T, dtype=torch.float64)
    c = torch.zeros(B, T, H, dtype=torch.float64)
    a = torch.zeros(T, dtype=torch.float64)
    b = torch.zeros(T, dtype=torch.float64)
    if pattern == "up":
        c += (-UP_AMP + UP_AMP * j / T).view(1, T, 1)
    elif pattern == "steep":
        c += (0.5 * j).view(1, T, 1)
    elif pattern == "down":
        c += (-30.0 * j / T).view(1, T, 1)
    elif pattern == "spike":
        c = 0.5 * torch.randn(B, T, H, **f64)
        for s in range(B):
            for h in range(H):
                ts = spike_key(s, h, H, T)
                c[s, ts, h] = 12.0
                v[s, ts, h] *= 4.0
    elif pattern == "wide":
        c = -100.0 * torch.rand(B, T, H, **f64)
    elif pattern == "dead":
        c = 0.5 * torch.randn(B, T, H, **f64)
    elif pattern == "zigzag":
        a = 1.0 - 2.0 * (torch.arange(T) % 2).double()
        b = 20.0 * (j / T - 0.5)
    q[..., 0] = math.sqrt(hd)
    q[..., 1] = math.sqrt(hd) * a.view(1, T, 1)
    k[..., 0] = c
    k[..., 1] = b.view(1, T, 1)
    if pattern == "flat":
        q.zero_()
        v[..., 0] = 1.0
        v[..., 1] = j.view(1, T, 1)
    elif pattern == "dead":
        for s in range(B):
            for h in range(H):
                for lo, hi in dead_ranges(s, h, T):
                    k[s, lo:hi, h] = 0.0
                    k[s, lo:hi, h, 0] = -200.0
    return torch.cat([x.reshape(B, T, H * hd) for x in (q, k, v)], dim=2).float()


def _heads(qkv, H, dtype):
    B, T, d3 = qkv.shape
    d = d3 // 3
    return tuple(x.to(dtype).view(B, T, H, d // H).permute(0, 2, 1, 3) for x in qkv.split(d, dim=2))      # [B, H, T, hd]


@torch.no_grad()
def attn_ref(qkv, H, dtype):
    """Dense causal attention [B, T, d] of ``qkv`` evaluated in ``dtype``: ``gpt2_ref.attn_core``, which carries the reference's
    -1e4 masked bias (every planted logit stays above -9896, where skipping the masked keys equals that formula: DESIGN.md 7)."""
    B, T, d3 = qkv.shape
    q, k, v = _heads(qkv, H, dtype)
    return gpt2_ref.attn_core(q, k.transpose(2, 3), v).permute(0, 2, 1, 3).reshape(B, T, d3 // 3)


class _State:
    """One online-softmax state of 32 queries per (sequence, head): running maximum m, sum l, accumulator O."""

    def __init__(self, B, H, hd):
        self.m = torch.full((B, H, 32), -math.inf, dtype=torch.float64)
        self.l = torch.zeros(B, H, 32, dtype=torch.float64)
        self.O = torch.zeros(B, H, 32, hd, dtype=torch.float64)

    def step(self, S, V, w, no_rescale):
        """Keys with logits S [B, H, 32, n] (-inf = masked), values V [B, H, n, hd] and multiplicities w [n]."""
        m_new = torch.maximum(self.m, S.max(dim=-1).values)
        fin = torch.isfinite(m_new)
        m_safe = torch.where(fin, m_new, torch.zeros_like(m_new))
        alpha = torch.where(torch.isfinite(self.m), torch.exp(self.m - m_safe), torch.zeros_like(m_new))
        p = torch.where(fin.unsqueeze(-1), torch.exp(S - m_safe.unsqueeze(-1)), torch.zeros_like(S)) * w
        self.l = self.l * alpha + p.sum(dim=-1)
        self.O = self.O * (1.0 if no_rescale else alpha.unsqueeze(-1)) + p @ V
        self.m = m_new

    def merge(self, other, unweighted):
        """``ATTN_MERGE4``'s step: fa = exp(m - m_new) (0 for an empty state), fb likewise for the second state."""
        m_new = torch.maximum(self.m, other.m)
        m_safe = torch.where(torch.isfinite(m_new), m_new, torch.zeros_like(m_new))
        fa = torch.where(torch.isfinite(self.m), torch.exp(self.m - m_safe), torch.zeros_like(m_new))
        fb = torch.where(torch.isfinite(other.m), torch.exp(other.m - m_safe), torch.zeros_like(m_new))
        if unweighted:
            fb = torch.ones_like(fb)
        self.O = self.O * fa.unsqueeze(-1) + other.O * fb.unsqueeze(-1)
        self.l = self.l * fa + other.l * fb
        self.m = m_new


@torch.no_grad()
def attn_tiled(qkv, H, form, defect=None):
    """float64 emulation of the fused kernels' STRUCTURE (not of their arithmetic): one 32-query tile at a time, a per-query
    online softmax over 32-key tiles up to the diagonal.

        keysplit   wave w takes the tiles w, w + 4, ... on a state of its own; the four states are merged (2, 3) -> (0, 1), then
                   1 -> 0 (``ATTN_MERGE4``)
        colsplit   128-key super-tiles (four tiles at once) on one state

    ``defect`` switches on ONE seeded mistake:

        drop_tile_last      the last key of every full tile (key0 + 31 < T) is lost
        double_tile_first   the first key of every tile after the first is counted twice
        no_rescale          the accumulator is not multiplied by alpha when the maximum rises (the sum is)
        mask_lt             the mask is key < query (row 0 keeps its own key)
        merge_unweighted    the second state of a merge enters with weight 1 (keysplit only: colsplit has no merge)
        leak_next           the keys of the last, partial tile that lie past T are the next sequence's rows (zeros after the last
                            sequence) and are not masked"""
    assert form in FORMS, form
    assert defect is None or defect in DEFECTS, defect
    B, T, d3 = qkv.shape
    d = d3 // 3
    hd = d // H
    q, k, v = _heads(qkv, H, torch.float64)
    ntile = (T + 31) // 32
    Tp = ntile * 32
    pad = lambda x: torch.cat([x, torch.zeros(B, H, Tp - T, hd, dtype=torch.float64)], dim=2)
    qp, kp, vp = pad(q), pad(k), pad(v)
    if defect == "leak_next" and Tp > T:
        for s in range(B - 1):
            n = min(Tp - T, T)
            kp[s, :, T:T + n] = k[s + 1, :, :n]
            vp[s, :, T:T + n] = v[s + 1, :, :n]
    out = torch.zeros(B, H, Tp, hd, dtype=torch.float64)
    ar = torch.arange(32)

    def tile(qt, kt):
        """Masked logits [B, H, 32, 32], values [B, H, 32, hd] and multiplicities [32] of key tile kt for query tile qt."""
        qi, kj = (qt * 32 + ar).view(32, 1), (kt * 32 + ar).view(1, 32)
        S = qp[:, :, qt * 32:qt * 32 + 32] @ kp[:, :, kt * 32:kt * 32 + 32].transpose(2, 3) / math.sqrt(hd)
        seen = (kj < qi) | ((kj == 0) & (qi == 0)) if defect == "mask_lt" else kj <= qi
        if defect == "leak_next" and kt == ntile - 1:
            seen = seen | (kj >= T)
        if defect == "drop_tile_last" and kt * 32 + 31 < T:
            seen = seen & (kj != kt * 32 + 31)
        w = torch.ones(32, dtype=torch.float64)
        if defect == "double_tile_first" and kt >= 1:
            w[0] = 2.0
        return S.masked_fill(~seen, -math.inf), vp[:, :, kt * 32:kt * 32 + 32], w

    for qt in range(ntile):
        if form == "keysplit":
            st = [_State(B, H, hd) for _ in range(4)]
            for w_ in range(4):
                for kt in range(w_, qt + 1, 4):
                    st[w_].step(*tile(qt, kt), no_rescale=defect == "no_rescale")
            st[0].merge(st[2], defect == "merge_unweighted")
            st[1].merge(st[3], defect == "merge_unweighted")
            st[0].merge(st[1], defect == "merge_unweighted")
            s0 = st[0]
        else:
            s0 = _State(B, H, hd)
            for kt0 in range(0, qt + 1, 4):
                parts = [tile(qt, kt) for kt in range(kt0, min(kt0 + 4, qt + 1))]
                s0.step(torch.cat([p[0] for p in parts], dim=-1), torch.cat([p[1] for p in parts], dim=2),
                        torch.cat([p[2] for p in parts]), no_rescale=defect == "no_rescale")
        out[:, :, qt * 32:qt * 32 + 32] = s0.O / s0.l.unsqueeze(-1)
    return out[:, :, :T].permute(0, 2, 1, 3).reshape(B, T, d)


def slice_errs(got, want, H):
    """(worst ``rel_err``, worst ``elementwise_err``) over the B * H (sequence, head) slices [T, hd] of two [B, T, d] tensors:
    a wrong head with small values cannot hide behind another head or sequence."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    B, T, d = want.shape
    hd = d // H
    e = w = 0.0
    for b in range(B):
        for h in range(H):
            g_, r_ = got[b, :, h * hd:(h + 1) * hd], want[b, :, h * hd:(h + 1) * hd]
            e, w = max(e, rel_err(g_, r_)), max(w, elementwise_err(g_, r_))
    return e, w


def device_bound(f32_rel, f32_elt):
    """The bound a device result is held to, from the float32 CPU yardstick of the SAME case: the project's numbers for this
    operation (rel_err 2e-5, elementwise_err 1) or 4 x the yardstick, whichever is larger.  The factor 4 covers another
    summation order over up to 1024 keys and the rounded reciprocal of sqrt(hd) at head dims 32, 96 and 128."""
    return max(REL_BOUND, YARDSTICK_FACTOR * f32_rel), max(ELT_BOUND, YARDSTICK_FACTOR * f32_elt)


_CASES = {}
_CASES_HD = [None]


def case(B, T, H, hd, pattern):
    """(qkv float32, float64 reference, (float32 yardstick rel_err, elementwise_err)) of one planted case: built once, shared
    by every test that asks for it and never modified.  Only the cases of the head_dim last asked for are kept."""
    if _CASES_HD[0] != hd:
        _CASES.clear()
        _CASES_HD[0] = hd
    key = (B, T, H, hd, pattern)
    if key not in _CASES:
        g = torch.Generator().manual_seed(((B * 7 + H) * 1031 + T) * 257 + hd * 11 + PATTERNS.index(pattern))
        qkv = plant(B, T, H, hd, pattern, g)
        want = attn_ref(qkv, H, torch.float64)
        _CASES[key] = (qkv, want, slice_errs(attn_ref(qkv, H, torch.float32).numpy(), want.numpy(), H))
    return _CASES[key]


def forget_cases():
    """Drop the cached cases (half a gigabyte at head_dim 256): the test modules call it when they are done."""
    _CASES.clear()
    _CASES_HD[0] = None
