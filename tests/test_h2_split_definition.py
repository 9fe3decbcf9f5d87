"""The two-term fp16 split of ``csrc/h2.h`` against a NumPy statement of its definition.

    v = x * PRE (PRE = 1/4 for activations, 1 for weights; exact),  hi = RN16(v),  lo' = RN16((v - hi) * 2^11)

``np.float16`` conversion is round-to-nearest-even, ``v - hi`` and its product with 2^11 are exact in float32 (hi is the nearest
of the 11-bit neighbours of the 24-bit v), so the statement below is the definition itself, and the three kernels that hand the
split out -- ``r4d_pack_h2_words_f32`` (h2 words), ``r4d_split2_lines_f16`` (activation lines), ``r4d_split2_planes_f16`` (weight
planes) -- must give its BITS for every finite input whose hi is finite.  Where hi overflows (|v| >= 65520) or the input is not
finite, the definition gives a non-finite lo' and the kernel's single fused rounding may give another non-finite one (inf where
the definition has NaN or the other way round: NaN payloads and that choice are not part of the contract): there only "finite or
not" is compared per position."""
import numpy as np
import pytest

F16_MAX = 65504.0


def split_ref(x, pre):
    """(hi, lo') as uint16 bit patterns; float32 arithmetic throughout."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = x.astype(np.float32) * np.float32(pre)
        hi = v.astype(np.float16)
        lo = ((v - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def _inputs():
    """(finite values whose hi is finite at PRE = 1/4 and at PRE = 1 after the division below, the rest): float32 arrays."""
    rng = np.random.default_rng(11)
    parts = [rng.standard_normal(1400)]
    # hi halfway: v exactly between two neighbouring fp16 values (ties to even), and one float32 step to either side
    h = rng.standard_normal(200).astype(np.float16)
    mid = (h.astype(np.float64) + np.nextafter(h, np.float16(np.inf)).astype(np.float64)) / 2
    mid32 = mid.astype(np.float32)
    assert np.array_equal(mid32.astype(np.float64), mid)
    parts += [mid32, np.nextafter(mid32, np.float32(np.inf)), np.nextafter(mid32, np.float32(-np.inf))]
    # lo' halfway: (v - hi) 2^11 between two neighbouring fp16 values.  With u = ulp16(hi) the scaled rest is a multiple of u/4
    # below 1024 u; fp16 holds it exactly below 512 u and in steps of u/2 from there on: the ties are 512 u + (2k + 1) u/4
    h = (rng.standard_normal(300) * 3).astype(np.float16)
    h = h[np.abs(h) >= 2.0 ** -10]
    u = np.spacing(np.abs(h)).astype(np.float64)
    k = rng.integers(0, 1023, h.size)
    rest = (512 * u + (2 * k + 1) * u / 4) * rng.choice([-1.0, 1.0], h.size)
    v = h.astype(np.float64) + rest / 2048
    v32 = v.astype(np.float32)
    keep = (v32.astype(np.float64) == v) & (v32.astype(np.float16) == h)
    assert keep.sum() > 200
    parts += [v32[keep]]
    # hi subnormal or zero; lo' subnormal or zero (v an fp16 value, or one a few float32 steps away from it)
    parts += [rng.standard_normal(300) * 2.0 ** rng.integers(-30, -13, 300)]
    h = rng.standard_normal(200).astype(np.float16).astype(np.float32)
    parts += [h, np.nextafter(h, np.float32(np.inf)), np.nextafter(np.nextafter(h, np.float32(-np.inf)), np.float32(-np.inf))]
    parts += [np.array([0.0, -0.0, 2.0 ** -149, -2.0 ** -149, 2.0 ** -126, 2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 3 * 2.0 ** -26])]
    # magnitudes 1e-8 .. 2^15 (times four below for the prescaled kernels: .. 2^17), random mantissas and signs
    mag = np.exp(rng.uniform(np.log(1e-8), np.log(2.0 ** 15), 600))
    parts += [mag * rng.choice([-1.0, 1.0], 600)]
    # the largest finite hi, from both sides of its rounding interval
    parts += [np.array([F16_MAX, -F16_MAX, 65519.0, -65519.0, np.nextafter(np.float32(65520.0), np.float32(0)), 65503.99, 65488.0, 65472.0])]
    fin = np.concatenate([np.asarray(p, np.float32) for p in parts])
    fin = np.resize(fin, 4096 - 64).astype(np.float32)                 # (repeats the head to fill whole lines)
    rest = np.array([np.inf, -np.inf, np.nan, 65520.0, -65520.0, 1e5, 2.0 ** 18, -3e5, 1e30, -1e30, 3e38, -3e38, 2.0 ** 120, 2.0 ** 127,
                     -2.0 ** 117, 7e4], np.float32)
    return fin, np.resize(rest, 64).astype(np.float32)


FIN, REST = _inputs()


def test_the_numpy_statement_reconstructs_x():
    """Host only: hi + 2^-11 lo' is within 2^-22 |v| of v wherever hi is an fp16 NORMAL number and lo' has not fallen into the
    fp16 subnormals (the range the GEMMs promise, gemm_h2.hip), and the inputs hold what the module says."""
    for pre in (0.25, 1.0):
        x = FIN if pre == 1.0 else FIN * np.float32(4.0)
        hi, lo = split_ref(x, pre)
        assert np.isfinite(hi.view(np.float16)).all() and np.isfinite(lo.view(np.float16)).all()
        v = x.astype(np.float64) * pre
        back = hi.view(np.float16).astype(np.float64) + lo.view(np.float16).astype(np.float64) / 2048
        inside = np.abs(v) >= 2.0 ** -3                                 # lo' >= 2^-3 2^-11 2^11 ... well inside the normals
        assert inside.sum() > 2000
        assert (np.abs(back - v)[inside] <= 2.0 ** -22 * np.abs(v)[inside]).all()
        hf = hi.view(np.float16)
        assert (hf == 0).any() and ((np.abs(hf) < 2.0 ** -14) & (hf != 0)).any() and (np.abs(hf) == F16_MAX).any()
        lf = lo.view(np.float16)
        assert (lf == 0).sum() > 100 and ((np.abs(lf) < 2.0 ** -14) & (lf != 0)).any()
    hi, lo = split_ref(REST, 1.0)
    assert not np.isfinite(lo.view(np.float16)).any()


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _check(got_hi, got_lo, x, pre, n_fin):
    hi, lo = split_ref(x, pre)
    assert np.array_equal(got_hi[:n_fin], hi[:n_fin]), np.flatnonzero(got_hi[:n_fin] != hi[:n_fin])[:8]
    assert np.array_equal(got_lo[:n_fin], lo[:n_fin]), np.flatnonzero(got_lo[:n_fin] != lo[:n_fin])[:8]
    for got, ref in ((got_hi, hi), (got_lo, lo)):
        assert np.array_equal(np.isfinite(got[n_fin:].view(np.float16)), np.isfinite(ref[n_fin:].view(np.float16)))


@pytest.mark.gpu
def test_h2_words_lines_and_planes_are_the_definition_bit_for_bit(dev):
    import torch
    from rag4dyg_amd import _lib, ops
    n_fin = FIN.size
    with np.errstate(over="ignore"):
        x4 = np.concatenate([FIN, REST]) * np.float32(4.0)             # the prescaled kernels: v = x / 4 runs over FIN (4 * 3e38 = inf: as good)
    xd = torch.from_numpy(x4).to(dev)
    w = ops.pack_h2_words(xd).cpu().numpy().view(np.uint32)
    _check((w & 0xffff).astype(np.uint16), (w >> 16).astype(np.uint16), x4, 0.25, n_fin)
    # an odd count: the last word's partner is the kernel's own zero
    w3 = ops.pack_h2_words(xd[:3]).cpu().numpy().view(np.uint32)
    assert np.array_equal(w3, w[:3])
    lines = ops.split2_lines(xd.view(-1, 64)).cpu().numpy().view(np.uint16)          # [rows, 2, 2, 32]
    _check(lines[:, :, 0].reshape(-1), lines[:, :, 1].reshape(-1), x4, 0.25, n_fin)
    # weight planes (no prescale), both source layouts; the entry point itself: ops.split2_planes declines weights beyond 6e4
    x1 = np.concatenate([FIN, REST])
    for transposed in (0, 1):
        N, K = 64, 64
        wt = torch.from_numpy(x1.reshape(N, K) if transposed else np.ascontiguousarray(x1.reshape(N, K).T)).to(dev)
        planes = torch.empty(N, K // 32, 2, 32, dtype=torch.int16, device=dev)
        _lib.check(_lib.load().r4d_split2_planes_f16(wt.data_ptr(), K, N, transposed, planes.data_ptr(), ops._stream()), "split2_planes")
        p = planes.cpu().numpy().view(np.uint16)
        _check(p[:, :, 0].reshape(-1), p[:, :, 1].reshape(-1), x1, 1.0, n_fin)
