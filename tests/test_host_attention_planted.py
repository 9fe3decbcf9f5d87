"""The planted attention cases (tests/_attention_ref.py) pinned to the oracle, and the proof that the GPU test built on them
(tests/test_gpu_attention_planted.py) has teeth: no GPU needed.

  * the float64 emulation of the kernels' structure -- 32-key tiles, an online softmax, four key-split states and their merge, or
    128-key super-tiles -- equals the dense float64 ``attn_core`` on every planted case, so the patterns do reach nothing that
    the structure itself gets wrong;
  * a float32 evaluation of the dense reference stays inside the project's bounds for this operation (rel_err 2e-5,
    elementwise_err 1) on every pattern but ``steep``, whose logits approach 80 (there the device's bound is 4 x this yardstick);
  * each seeded structural mistake moves at least one planted case by 10x or more of the bound the device is held to on that
    case.  What the i.i.d. N(0,1) input of the older value tests gives for the same mistakes is printed beside it."""
import pytest
import torch

from conftest import rel_err
from _attention_ref import (DEFECTS, FORMS, PATTERNS, REL_BOUND, ELT_BOUND, attn_ref, attn_tiled, case, device_bound, forget_cases, patterns_for,
                            slice_errs)

TS = (1, 31, 32, 33, 127, 128, 129, 160, 257, 1024)
HDS = (32, 64, 96, 128, 256)
B, H = 3, 2
DETECT_TS = tuple(T for T in TS if 33 <= T <= 257)
DETECT_HD = 32


@pytest.fixture(scope="module", autouse=True)
def _cases_forgotten():
    yield
    forget_cases()


@pytest.mark.parametrize("hd", [32, 256])
@pytest.mark.parametrize("form", FORMS)
def test_tiled_emulation_equals_the_dense_reference(form, hd):
    """float64, no defect: the tiling, the online softmax, the key split and its merge are the dense ``attn_core`` to 1e-12 per
    (sequence, head) slice on every pattern and T -- dead first tiles, empty key-split states and partial last tiles included."""
    worst = 0.0
    for T in TS:
        for pattern in patterns_for(T):
            qkv, want, _ = case(B, T, H, hd, pattern)
            e, _ = slice_errs(attn_tiled(qkv, H, form).numpy(), want.numpy(), H)
            worst = max(worst, e)
            assert e < 1e-12, (form, hd, pattern, T, e)
    print(f"[attn-planted tiled] {form} hd {hd}: worst slice rel_err {worst:.2e}")


@pytest.mark.parametrize("hd", HDS)
def test_float32_yardstick_is_inside_the_project_bounds(hd):
    """What plain fp32 costs on the planted inputs, per (sequence, head) slice.  ``steep`` is reported only: its logits approach
    80, where the resolution of an fp32 logit (2^-17 at 64) alone costs more than 2e-5."""
    for pattern in PATTERNS:
        worst = (0.0, 0.0)
        for T in TS:
            if pattern not in patterns_for(T):
                continue
            e, w = case(B, T, H, hd, pattern)[2]
            print(f"[attn-planted f32] hd {hd} {pattern} T {T}: rel_err {e:.2e} elementwise_err {w:.3f}")
            worst = (max(worst[0], e), max(worst[1], w))
            if pattern != "steep":
                assert e < REL_BOUND and w < ELT_BOUND, (hd, pattern, T, e, w)
        print(f"[attn-planted f32] hd {hd} {pattern}: worst rel_err {worst[0]:.2e} elementwise_err {worst[1]:.3f}")


def test_every_seeded_defect_moves_a_planted_case():
    """The detection matrix (defect x pattern: the largest slice rel_err over both forms and T in 33 .. 257) and, per defect, the
    best ratio of that error to the device's rel_err bound of the same case: at least 10."""
    g = torch.Generator().manual_seed(5)
    gauss = {T: torch.randn(B, T, 3 * H * DETECT_HD, generator=g) for T in DETECT_TS}
    gauss_ref = {T: attn_ref(x, H, torch.float64).numpy() for T, x in gauss.items()}
    print("[attn-planted detect] defect: " + " ".join(f"{p:>8s}" for p in PATTERNS + ("N(0,1)",)) + "   best ratio to the bound")
    for defect in DEFECTS:
        row, best = [], (0.0, None)
        for pattern in PATTERNS:
            worst = 0.0
            for T in DETECT_TS:
                if pattern not in patterns_for(T):
                    continue
                qkv, want, f32 = case(B, T, H, DETECT_HD, pattern)
                for form in FORMS:
                    e, _ = slice_errs(attn_tiled(qkv, H, form, defect).numpy(), want.numpy(), H)
                    worst = max(worst, e)
                    ratio = e / device_bound(*f32)[0]
                    if ratio > best[0]:
                        best = (ratio, (pattern, T, form))
            row.append(worst)
        # for information only: the i.i.d. input of the older value tests, in the max-norm over the whole tensor they use
        row.append(max(rel_err(attn_tiled(gauss[T], H, form, defect).numpy(), gauss_ref[T]) for T in DETECT_TS for form in FORMS))
        print(f"[attn-planted detect] {defect:>17s}: " + " ".join(f"{e:8.1e}" for e in row) + f"   {best[0]:.1e} at {best[1]}")
        assert best[0] >= 10.0, (defect, best)
