"""CPU side of the training stress tests (``test_gpu_training_stress.py``): the case table of ``_training_stress_cases.py`` is
ADMISSIBLE -- the float32 reference alone, with the whole summation-order allowance K on top, stays inside every absolute cap an
entry carries --, K covers the spread of the reference's own error over the CPU's summation orders with a factor two to spare, the
float64 gradients are finite and none is identically zero, and the inputs are what their tags say: peaked softmax rows, saturated
GELU pre-activations, an activation beyond the fp16 range."""
import numpy as np
import pytest

import _training_stress_cases as C

pytestmark = pytest.mark.slow


@pytest.mark.parametrize("e", C.ENTRIES, ids=C.ENTRY_IDS)
def test_entry_is_admissible_and_K_covers_the_reference_spread(e):
    p = C.reference_profile(e)
    spread, name = C.order_spread(p)
    worst_e = max(p.e_ref.values())
    print(f"{C.entry_id(e)}: spread {spread:.2f} ({name}); reference max-norm {worst_e:.2e}, element-wise {p.ew_ref:.3f}, loss {p.loss_ref:.1e}, "
          f"emb/hidden {p.hidden_ref:.1e}")
    # the float64 gradients: finite, no tensor identically zero
    for n, g in p.ref64["grads"].items():
        assert np.isfinite(g).all(), n
        assert np.abs(g).max() > 0, f"{n}: gradient identically zero"
    assert np.isfinite(p.ref64["loss"])
    # K itself: the reference's spread over the CPU orders is at most K / 2 (a larger one names its tensor)
    assert spread <= C.K / 2, f"{name}: float32 reference spread {spread:.2f} over the CPU orders exceeds K / 2 = {C.K / 2}"
    # admissibility of every cap the entry carries
    assert C.K * p.loss_ref <= C.LOSS_CAP, p.loss_ref
    assert C.K * worst_e <= C.NORM_CAP, {n: v for n, v in p.e_ref.items() if C.K * v > C.NORM_CAP}
    if "h" in e.caps:
        assert C.K * p.hidden_ref <= C.HIDDEN_CAP, p.hidden_ref
    if "e" in e.caps:
        assert C.K * p.ew_ref <= C.EW_CAP, p.ew_ref


def test_K_is_within_its_limits():
    assert 1.5 <= C.K <= 10.0


def test_every_required_length_and_shape_is_in_the_table():
    peaked_weights = {e.weights for e in C.ENTRIES if e.peaked}
    lengths = {t for e in C.ENTRIES if e.weights in peaked_weights for t in e.Ts}
    assert {2, 127, 128, 129, 255, 256, 257, 509, 1024} <= lengths, lengths
    assert any(e.kind == "enc" and e.Ts == (1,) for e in C.ENTRIES)
    assert any(e.kind == "enc" and e.Ts == (129, 37, 256) for e in C.ENTRIES)
    assert {e.weights for e in C.ENTRIES} >= set(C.G13_CASES)
    assert {"enc", "lm", "gen", "gen_tied"} == {e.kind for e in C.ENTRIES}
    assert all(1 <= b <= 4 for e in C.ENTRIES for b in e.Bs)
    shapes = {C.SEEDED[e.weights][:3] + (C.SEEDED[e.weights][5],) for e in C.ENTRIES if e.weights in C.SEEDED}
    assert {(2, 8, 512, 4.0), (2, 2, 512, 6.0), (2, 6, 768, 6.0), (1, 2, 256, 6.0)} <= shapes
    # the element-wise cap: at least every sharpen-4 entry and the two unsharpened G13 sets
    for e in C.ENTRIES:
        if e.weights in ("hd128_plain", "hd128_stress") or (e.weights in C.SEEDED and C.SEEDED[e.weights][5] == 4.0):
            assert "e" in e.caps, C.entry_id(e)


_PEAKS = {}


@pytest.mark.parametrize("e", [e for e in C.ENTRIES if e.peaked], ids=[C.entry_id(e) for e in C.ENTRIES if e.peaked])
def test_peaked_entries_have_peaked_softmax_rows(e):
    med, _pre = C.attention_and_gelu_statistics(e)
    print(f"{C.entry_id(e)}: row-max median per layer {med}")
    _PEAKS[C.entry_id(e)] = max(m for m in med if m is not None)
    assert _PEAKS[C.entry_id(e)] >= 0.3, med


def test_some_entry_reaches_a_row_max_median_of_09():
    for e in C.ENTRIES:
        if e.peaked and C.entry_id(e) not in _PEAKS:
            med, _pre = C.attention_and_gelu_statistics(e)
            _PEAKS[C.entry_id(e)] = max(m for m in med if m is not None)
    assert max(_PEAKS.values()) >= 0.9, _PEAKS


@pytest.mark.parametrize("e", [e for e in C.ENTRIES if e.weights.startswith("gelusat") and e.Ts[0] > 1],
                         ids=[C.entry_id(e) for e in C.ENTRIES if e.weights.startswith("gelusat") and e.Ts[0] > 1])
def test_gelu_saturation_entries_are_saturated(e):
    _med, pre = C.attention_and_gelu_statistics(e)
    a = np.abs(pre)
    share = float(((a > 4) & (a < 8)).mean())
    print(f"{C.entry_id(e)}: max |c_fc pre-activation| {a.max():.1f}, {100 * share:.1f} % in 4 < |x| < 8")
    assert a.max() >= 10 and share >= 0.01


def test_f16_range_weights_exceed_the_fp16_range_in_the_oracle():
    """One GELU output of the float64 oracle beyond 2^18 (the f16x2 A operand's limit); the float64 gradients stay finite."""
    _sd, _H, top = C.f16_range_weights()
    assert top > C.F16_RANGE_LIMIT, top
    p = C.reference_profile(C.f16_range_entry())
    assert all(np.isfinite(g).all() and np.abs(g).max() > 0 for g in p.ref64["grads"].values())
    spread, name = C.order_spread(p)
    print(f"f16 range case: largest GELU output {top:.3e}; reference max-norm {max(p.e_ref.values()):.2e}, spread {spread:.2f} ({name})")
    assert spread <= C.K / 2, name
    assert C.K * max(p.e_ref.values()) <= C.NORM_CAP and C.K * p.loss_ref <= C.LOSS_CAP
