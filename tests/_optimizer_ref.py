"""Shared states, cases and bounds of the optimizer-kernel tests (``test_host_optimizer_kernels.py`` on the CPU,
``test_gpu_optimizer_kernels.py`` on the device): ``r4d_sumsq_accumulate_f32`` and ``r4d_adamw_step_f32`` on their own, from a
GIVEN state, against ``oracle/train_ref.py`` (``adamw_step`` / ``clip_coefficient``) in float64.  Nothing here touches the GPU."""
import functools
import itertools
import math

import numpy as np
import torch

# ---------------------------------------------------------------------------------------------------------------- sumsq
# 256 threads a workgroup, at most 1024 workgroups: the grid-stride loop takes its second trip beyond 262144 elements
SUMSQ_NS = (1, 63, 64, 65, 255, 256, 257, 262143, 262144, 262145, 1000003)
SUMSQ_FLOATS = 1025                                                 # [0] the running total (caller state), [1:] scratch partials
NORM_BOUND = 1e-5                                                   # test_training_step_parameter_update_equals_oracle_adamw's on grad_norm()


def sumsq_input(n, kind="gauss"):
    g = torch.Generator().manual_seed(n)
    if kind == "gauss":
        return torch.randn(n, generator=g)
    x = torch.full((n,), 1e-3)
    x[n // 3] = {"spike": 1e18, "nan": float("nan"), "overflow": 1e20}[kind]      # (1e20)^2 is beyond float32
    return x


def norm64(*xs):
    return math.sqrt(sum(float(x.double().square().sum()) for x in xs))


# ---------------------------------------------------------------------------------------------------------------- AdamW
ADAMW_NS = (1, 255, 256, 257, 100003)
ADAMW_TS = (1, 2, 10, 1000, 100000)                                 # 1 - b2^t from 1e-3 to 1: the bias correction saturates
ADAMW_WDS = (0.0, 0.01)
ADAMW_LR_EPS = ((1e-3, 1e-8), (5e-5, 1e-6))
ADAMW_BETAS = ((0.9, 0.999), (0.8, 0.9))
# beside the cross: a decay strong enough to show WHICH p it multiplies -- decaying the old p instead of the updated one moves the
# result by lr * wd = 5 % of the update here, by 1e-5 of it (inside every bound) at the cross's lr * wd
ADAMW_STRONG_DECAY = ((10, 0.5, (0.1, 1e-8), (0.9, 0.999)), (1, 0.5, (0.1, 1e-8), (0.8, 0.9)))
ADAMW_HYPERS = tuple(itertools.product(ADAMW_TS, ADAMW_WDS, ADAMW_LR_EPS, ADAMW_BETAS)) + ADAMW_STRONG_DECAY
MOMENT_BOUND, UPDATE_BOUND, P_ULPS = 1e-5, 1e-4, 2.0


@functools.lru_cache(maxsize=None)
def adamw_state(n):
    """(p, g, m, v) float32 of n elements: gradients from 1e-12 to 1e3 in magnitude with both signs, one in eight exactly zero
    and there m = v = 0 as well (a parameter no batch has touched yet); m of the gradients' magnitude, v >= 0 near m^2;
    parameters around 1 with a few large and a few tiny ones."""
    gen = torch.Generator().manual_seed(77 * n + 5)
    mag = 10.0 ** (torch.rand(n, generator=gen) * 15 - 12)
    g = mag * torch.sign(torch.randn(n, generator=gen))
    m = mag * torch.randn(n, generator=gen) * 0.5
    v = (mag * (0.3 + torch.rand(n, generator=gen))) ** 2
    p = torch.randn(n, generator=gen)
    p[::7] *= 100
    p[3::11] *= 1e-4
    zero = torch.arange(n) % 8 == (0 if n > 1 else 1)
    g[zero] = 0; m[zero] = 0; v[zero] = 0
    return p, g, m, v


def adamw_oracle(p, g, m, v, t, lr, betas, eps, wd, coef=1.0):
    """``train_ref.adamw_step`` in float64 on the float32 state (gradient scaled by the clip coefficient first)."""
    from oracle import train_ref
    return train_ref.adamw_step(p.double(), g.double() * coef, m.double(), v.double(), t, lr, betas=betas, eps=eps, weight_decay=wd)


def adamw_float32(p, g, m, v, t, lr, betas, eps, wd, coef=1.0):
    """The same update in float32 torch arithmetic, scalars formed in double and rounded once: what ``transformers.AdamW`` does."""
    b1, b2 = betas
    g = g * np.float32(coef)
    m = m * np.float32(b1) + g * np.float32(1.0 - b1)
    v = v * np.float32(b2) + g * g * np.float32(1.0 - b2)
    step = np.float32(lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))
    p = p - step * (m / (v.sqrt() + np.float32(eps)))
    if wd > 0.0:
        p = p - np.float32(lr * wd) * p
    return p, m, v


def ulp32(x):
    """Spacing of float32 at |x| (float64 array in, float64 out)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def adamw_ratios(got, ref, p0):
    """Each measured error over its bound (pass: all < 1 -- <= 1 for p): (m, v, p).
    m, v: max-norm relative error against MOMENT_BOUND.  p, per element: |p - p_ref| against
    UPDATE_BOUND * max |p_ref - p0| + P_ULPS * ulp_f32(|p_ref|) -- the first term is the bound of the whole-step tests, the second the
    float32 roundings on the way to p (update, subtraction, decay), without which a small lr on parameters near 1 fails by
    rounding alone."""
    from conftest import rel_err
    (p, m, v), (pr, mr, vr) = got, ref
    pr64, p64 = pr.double().numpy(), p.double().numpy()
    bound = UPDATE_BOUND * np.abs(pr64 - p0.double().numpy()).max() + P_ULPS * ulp32(pr64)
    return (rel_err(m.numpy(), mr.numpy()) / MOMENT_BOUND, rel_err(v.numpy(), vr.numpy()) / MOMENT_BOUND,
            float((np.abs(p64 - pr64) / bound).max()))
