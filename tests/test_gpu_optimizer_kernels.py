"""GPU tests of the two optimizer kernels on their own (``csrc/train_ops.hip``): ``r4d_sumsq_accumulate_f32`` next to its
workgroup and grid-stride boundaries and on data that overflows, ``r4d_adamw_step_f32`` for one step from a GIVEN state over
step counts, decays, learning rates and betas, and the three clip modes -- against ``oracle/train_ref.py`` in float64 under
the bounds ``test_host_optimizer_kernels.py`` shows float32 arithmetic itself to meet."""
import math

import numpy as np
import pytest
import torch

import _optimizer_ref as opt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sumsq(x, accum):
    from rag4dyg_amd import _lib
    return _lib.load().r4d_sumsq_accumulate_f32(x.data_ptr(), x.numel(), accum.data_ptr(), _stream())


def _adamw(dev, state, t, lr, betas, eps, wd, sumsq=None, max_norm=0.0, n=None):
    """One launch on device copies of the state; returns (rc, (p, m, v) on the CPU)."""
    from rag4dyg_amd import _lib
    p, g, m, v = (x.to(dev).clone() for x in state)
    rc = _lib.load().r4d_adamw_step_f32(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel() if n is None else n, lr,
                                        betas[0], betas[1], eps, wd, t, sumsq.data_ptr() if sumsq is not None else None,
                                        max_norm, _stream())
    return rc, (p.cpu(), m.cpu(), v.cpu())


# ================================================================================================ sumsq
@pytest.mark.parametrize("n", opt.SUMSQ_NS)
def test_sumsq_norm_accumulation_and_determinism(dev, n):
    x = opt.sumsq_input(n).to(dev)
    accum = torch.zeros(opt.SUMSQ_FLOATS, dtype=torch.float32, device=dev)
    assert _sumsq(x, accum) == 0
    first = accum[:1].clone()
    err = abs(math.sqrt(first.item()) / opt.norm64(x.cpu()) - 1)
    print(f"[sumsq] n {n}: norm error {err:.2e} (bound {opt.NORM_BOUND:g})")
    assert err < opt.NORM_BOUND
    accum.zero_()
    assert _sumsq(x, accum) == 0 and torch.equal(accum[:1], first)                 # same bits on a second run
    # three tensors into one total, on top of a value that is already there
    others = [opt.sumsq_input(k).to(dev) * s for k, s in ((257, 3.0), (1000, 0.5))]
    accum.zero_()
    accum[0] = 5.0
    for t in (x, *others):
        assert _sumsq(t, accum) == 0
    want = math.sqrt(5.0 + opt.norm64(x.cpu(), *(o.cpu() for o in others)) ** 2)
    assert abs(math.sqrt(accum[0].item()) / want - 1) < opt.NORM_BOUND
    before = accum.clone()
    from rag4dyg_amd import _lib
    assert _lib.load().r4d_sumsq_accumulate_f32(x.data_ptr(), 0, accum.data_ptr(), _stream()) == 0      # n = 0 changes nothing
    assert torch.equal(accum.view(torch.int32), before.view(torch.int32))


@pytest.mark.parametrize("n", [257, 262145])
def test_sumsq_on_a_spike_a_nan_and_an_overflow(dev, n):
    accum = torch.zeros(opt.SUMSQ_FLOATS, dtype=torch.float32, device=dev)
    spike = opt.sumsq_input(n, "spike")
    assert _sumsq(spike.to(dev), accum) == 0
    assert abs(math.sqrt(accum[0].item()) / opt.norm64(spike) - 1) < opt.NORM_BOUND
    accum.zero_()
    assert _sumsq(opt.sumsq_input(n, "nan").to(dev), accum) == 0 and math.isnan(accum[0].item())
    accum.zero_()
    assert _sumsq(opt.sumsq_input(n, "overflow").to(dev), accum) == 0 and accum[0].item() == math.inf


# ================================================================================================ AdamW
@pytest.mark.parametrize("n", opt.ADAMW_NS)
def test_adamw_step_from_a_given_state_equals_the_oracle(dev, n):
    state = opt.adamw_state(n)
    worst = np.zeros(3)
    for t, wd, (lr, eps), betas in opt.ADAMW_HYPERS:
        rc, got = _adamw(dev, state, t, lr, betas, eps, wd)
        assert rc == 0
        ref = opt.adamw_oracle(*state, t, lr, betas, eps, wd)
        r = np.array(opt.adamw_ratios(got, ref, state[0]))
        worst = np.maximum(worst, r)
        assert (r[:2] < 1).all() and r[2] <= 1, (t, wd, lr, eps, betas, r)
        zero = state[1] == 0                                       # untouched elements: moments stay zero, only the decay moves p
        assert not got[1][zero].any() and not got[2][zero].any()
        if wd == 0:
            assert torch.equal(got[0][zero], state[0][zero])
    print(f"[adamw] n {n}: worst error / bound  m {worst[0]:.3f}  v {worst[1]:.3f}  p {worst[2]:.3f}")


HYPER = dict(t=3, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.01)


def _bits(x):
    return [t.view(torch.int32) for t in x]


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(_bits(a), _bits(b)))


@pytest.mark.parametrize("n", [257, 100003])
def test_clip_modes(dev, n):
    from oracle import train_ref
    state = opt.adamw_state(n)
    g = state[1]
    sumsq = torch.zeros(opt.SUMSQ_FLOATS, dtype=torch.float32, device=dev)
    assert _sumsq(g.to(dev), sumsq) == 0
    norm = opt.norm64(g)
    assert abs(math.sqrt(sumsq[0].item()) / norm - 1) < opt.NORM_BOUND
    rc0, none = _adamw(dev, state, **HYPER)                                        # no pointer
    rc1, off = _adamw(dev, state, **HYPER, sumsq=sumsq, max_norm=0.0)              # pointer, max_norm = 0
    rc2, idle = _adamw(dev, state, **HYPER, sumsq=sumsq, max_norm=float(np.float32(norm * 1.5)))   # norm < max_norm: coef == 1 exactly
    assert rc0 == rc1 == rc2 == 0
    assert _same_bits(none, off) and _same_bits(none, idle)
    max_norm = float(np.float32(norm * 0.01))                                      # an active clip
    coef, total = train_ref.clip_coefficient([g], max_norm)
    assert coef < 0.011 and abs(total - norm) < 1e-9 * norm
    rc, got = _adamw(dev, state, **HYPER, sumsq=sumsq, max_norm=max_norm)
    ref = opt.adamw_oracle(*state, HYPER["t"], HYPER["lr"], HYPER["betas"], HYPER["eps"], HYPER["wd"], coef)
    r = opt.adamw_ratios(got, ref, state[0])
    print(f"[adamw clip] n {n}: coefficient {coef:.4e}; error / bound  m {r[0]:.3f}  v {r[1]:.3f}  p {r[2]:.3f}")
    assert rc == 0 and r[0] < 1 and r[1] < 1 and r[2] <= 1
    assert not _same_bits(none, got)


def test_clip_with_a_non_finite_norm(dev):
    """An infinite norm with finite gradients clips them to nothing (coefficient max_norm / inf = 0): the moments only decay.  A NaN
    norm poisons the whole update, as ``clip_grad_norm_`` does (NaN coefficient times every gradient)."""
    n = 1000
    state = opt.adamw_state(n)
    p0, _g, m0, v0 = state
    sumsq = torch.zeros(opt.SUMSQ_FLOATS, dtype=torch.float32, device=dev)
    sumsq[0] = math.inf
    rc, (p, m, v) = _adamw(dev, state, **HYPER, sumsq=sumsq, max_norm=1.0)
    assert rc == 0
    assert torch.equal(m, m0 * np.float32(0.9)) and torch.equal(v, v0 * np.float32(0.999))
    ref = opt.adamw_oracle(*state, HYPER["t"], HYPER["lr"], HYPER["betas"], HYPER["eps"], HYPER["wd"], 0.0)
    r = opt.adamw_ratios((p, m, v), ref, p0)
    assert r[0] < 1 and r[1] < 1 and r[2] <= 1, r
    sumsq[0] = math.nan
    rc, (p, m, v) = _adamw(dev, state, **HYPER, sumsq=sumsq, max_norm=1.0)
    assert rc == 0 and torch.isnan(p).all() and torch.isnan(m).all() and torch.isnan(v).all()
    rc, clean = _adamw(dev, state, **HYPER, sumsq=sumsq, max_norm=0.0)             # clipping off: the NaN is not read into the update
    assert rc == 0 and all(torch.isfinite(x).all() for x in clean)


def test_adamw_empty_tensor_and_step_zero(dev):
    from rag4dyg_amd import _lib
    state = opt.adamw_state(257)
    rc, got = _adamw(dev, state, **HYPER, n=0)
    assert rc == 0 and _same_bits(got, (state[0], state[2], state[3]))             # n = 0: OK, nothing written
    rc, got = _adamw(dev, state, **dict(HYPER, t=0))
    assert rc != 0 and _lib.load().r4d_last_error()
    assert _same_bits(got, (state[0], state[2], state[3]))
