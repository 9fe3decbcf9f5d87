"""CPU half of the optimizer-kernel tests: the states and bounds of ``_optimizer_ref.py`` hold for a float32 torch restatement of
the same update at every case, so ``test_gpu_optimizer_kernels.py`` asks of the device only what float32 can give."""
import math

import numpy as np
import pytest
import torch

import _optimizer_ref as opt


def test_ulp32_is_the_float32_spacing():
    assert opt.ulp32(1.0) == 2.0 ** -23 and opt.ulp32(-3.0) == 2.0 ** -22 and opt.ulp32(0.75) == 2.0 ** -24
    assert opt.ulp32(0.0) == 2.0 ** -149


@pytest.mark.parametrize("n", opt.ADAMW_NS)
def test_states_span_what_they_claim(n):
    p, g, m, v = opt.adamw_state(n)
    assert all(x.dtype == torch.float32 and x.shape == (n,) and torch.isfinite(x).all() for x in (p, g, m, v))
    assert (v >= 0).all() and torch.equal(g == 0, v == 0) and not m[g == 0].any()
    if n >= 255:
        a = g[g != 0].abs()
        assert a.min() < 1e-10 and a.max() > 1e2 and (g > 0).any() and (g < 0).any() and (g == 0).sum() >= n // 9


@pytest.mark.parametrize("n", opt.ADAMW_NS)
def test_float32_restatement_meets_every_bound(n):
    """Every (t, wd, lr, eps, betas) on every n: float32 arithmetic itself stays inside the three bounds (m, v: 1e-5 max-norm;
    p: 1e-4 of the largest update + 2 ulp), with the worst ratio printed."""
    p, g, m, v = opt.adamw_state(n)
    worst = np.zeros(3)
    for t, wd, (lr, eps), betas in opt.ADAMW_HYPERS:
        for coef in (1.0, 0.37):
            ref = opt.adamw_oracle(p, g, m, v, t, lr, betas, eps, wd, coef)
            got = opt.adamw_float32(p, g, m, v, t, lr, betas, eps, wd, coef)
            r = np.array(opt.adamw_ratios(got, ref, p))
            assert (r[:2] < 1).all() and r[2] <= 1, (t, wd, lr, eps, betas, coef, r)
            assert float((ref[0] - p.double()).abs().max()) > 0
            worst = np.maximum(worst, r)
    print(f"[adamw float32 restatement] n {n}: worst error / bound  m {worst[0]:.3f}  v {worst[1]:.3f}  p {worst[2]:.3f}")


def test_bias_correction_saturates_over_the_step_counts():
    bc2 = [1 - 0.999 ** t for t in opt.ADAMW_TS]
    assert bc2[0] < 1.1e-3 and bc2[-1] == 1.0 and sorted(bc2) == bc2


@pytest.mark.parametrize("n", opt.SUMSQ_NS)
def test_float32_norm_meets_the_bound(n):
    x = opt.sumsq_input(n)
    assert abs(math.sqrt(float(x.square().sum())) / opt.norm64(x) - 1) < opt.NORM_BOUND
    assert abs(math.sqrt(float((x * x).cumsum(0)[-1])) / opt.norm64(x) - 1) < opt.NORM_BOUND     # even summed one after the other


def test_sumsq_data_cases():
    n = 1000
    spike = opt.sumsq_input(n, "spike")
    assert abs(math.sqrt(float(spike.square().sum())) / opt.norm64(spike) - 1) < opt.NORM_BOUND and opt.norm64(spike) > 9e17
    assert math.isnan(float(opt.sumsq_input(n, "nan").square().sum()))
    over = opt.sumsq_input(n, "overflow")
    assert torch.isfinite(over).all() and math.isinf(float(over.square().sum()))
    from oracle import train_ref
    coef, total = train_ref.clip_coefficient([opt.sumsq_input(n)], 1.0)
    assert abs(total - opt.norm64(opt.sumsq_input(n))) < 1e-9 and coef == min(1.0, 1.0 / (total + 1e-6)) and coef < 1
