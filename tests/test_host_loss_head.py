"""CPU half of the loss-head edge tests: ``_loss_head_ref.loss_head`` is pinned to the oracle (``oracle/train_ref.py``) in float64
and to the reference's own float32 values (``tests/golden/g14_loss_head_edges.npz``), and every bound and cap that
``test_gpu_loss_head.py`` puts on the device is established here from the reference alone."""
import numpy as np
import pytest
import torch

import _loss_head_ref as lh
from _training_stress_cases import E_FLOOR, K
from conftest import elementwise_err, load_golden, rel_err

ORACLE_CASES = [c for c in lh.CASES if 2 <= c.B <= 33]


def test_case_table_keeps_every_shape_every_regime_and_the_full_cross():
    assert {(c.B, c.d) for c in lh.CASES} == set(lh.SHAPES)
    assert {c.regime for c in lh.CASES} == set(lh.REGIMES)
    for B, d in lh.CROSS_SHAPES:
        got = {(c.tau, c.lam, c.alpha, c.gscale) for c in lh.CASES if (c.B, c.d) == (B, d)}
        assert got >= {(tau, lam, a, s) for tau in lh.TAUS for lam in lh.LAMS for a, s in lh.ALPHA_SCALES}
    for regime in lh.REGIMES:                                      # every regime also beyond one wave / one 256-thread trip
        assert any(c.regime == regime and c.d > 256 for c in lh.CASES)
        assert regime == "dups" or any(c.regime == regime and c.B > 21 for c in lh.CASES)
    assert len(set(lh.CASE_IDS)) == len(lh.CASES)


def test_generator_regimes_hold_what_they_claim():
    for B, d in ((1, 7), (5, 64), (17, 63)):
        for regime in lh.REGIMES:
            emb, ta, tp, tn = lh.make_inputs(regime, B, d)
            assert emb.shape == (5, B, d) and emb.dtype == torch.float32 and all(t.shape == (B, 1) for t in (ta, tp, tn))
            assert torch.equal(emb, lh.make_inputs(regime, B, d)[0])
            nrm = emb.norm(dim=2)
            if regime == "unit":
                assert (nrm[3:] - 1).abs().max() < 1e-6
            if regime == "dups":
                assert torch.equal(emb[1], emb[0]) and torch.equal(emb[4], emb[3]) and torch.equal(tp, ta)
                assert B == 1 or torch.equal(emb[0, 1], emb[0, 0])
            else:                                                  # the three blocks at three scales
                live = nrm[:3].median(dim=1).values
                assert regime == "zero" and B < 3 or (live[1] > 3 * live[0] and live[0] > 2 * live[2])
            if regime == "zero":
                assert all(bool((emb[k] == 0).all(dim=1).any()) for k in range(4))
            if regime == "pooled":
                u = torch.nn.functional.normalize(emb.reshape(-1, d), dim=1)
                assert d < 8 or (u @ u.T).min() > 0.99
            if regime == "tgap" and B > 1:
                off = torch.exp(-0.05 * (ta - ta.T).abs())[~torch.eye(B, dtype=torch.bool)]
                assert off.max() == 0 and torch.exp(-0.05 * (ta - tp.T).abs()).max() == 0
            if regime == "tsame":
                assert len({float(x) for t in (ta, tp, tn) for x in t.reshape(-1)}) == 1
            elif regime != "dups" and B >= 17:
                assert (tp - ta).mean() > 1 and (tn - tp).mean() > 1


@pytest.mark.parametrize("c", ORACLE_CASES, ids=[lh.case_id(c) for c in ORACLE_CASES])
def test_loss_head_float64_equals_the_oracle_in_value_and_gradient(c):
    from oracle import train_ref
    emb, ta, tp, tn = lh.make_inputs(c.regime, c.B, c.d)
    leaf = emb.double().requires_grad_(True)
    cl = train_ref.cltime_loss(c.tau, c.lam, leaf[0], leaf[1], leaf[2], ta.double(), tp.double(), tn.double())
    au = c.alpha * train_ref.info_nce(leaf[3], leaf[4], c.tau, c.B)
    ((cl + au) * c.gscale).backward()
    y = lh.yardstick(c)
    assert lh.loss_err([cl.item(), au.item(), (cl + au).item()], y.losses64) < 1e-12
    assert rel_err(leaf.grad.numpy(), y.grad64) < 1e-12
    flat, _ = lh.evaluate(c, torch.float64, (emb, ta.reshape(-1), tp.reshape(-1), tn.reshape(-1)))      # [B] times
    assert np.array_equal(flat, y.losses64)


def test_oracle_raises_at_batch_one_and_loss_head_does_not():
    from oracle import train_ref
    g = load_golden("g14_loss_head_edges")
    assert bool(g["b1_raises"])                                    # the reference's own CLtime_loss
    emb, ta, tp, tn = lh.make_inputs("gauss", 1, 7)
    with pytest.raises(RuntimeError):
        train_ref.cltime_loss(0.07, 0.05, emb[0], emb[1], emb[2], ta, tp, tn)
    for dtype in (torch.float32, torch.float64):
        cl, au = lh.loss_head(0.07, 0.05, 1.0, emb.to(dtype), ta, tp, tn)
        assert torch.isfinite(cl) and cl.dtype == dtype and au.item() == 0.0
    # one row: logits [cos(a, p) dec | 0 | cos(a, n) dec] / tau with label 0
    a, p, n = (x[0].double() for x in emb[:3])
    cos = lambda x, y: float(x @ y / (x.norm() * y.norm()))
    lg = np.array([cos(a, p) * np.exp(-0.05 * abs(float(ta) - float(tp))), 0.0, cos(a, n) * np.exp(-0.05 * abs(float(ta) - float(tn)))]) / 0.07
    want = np.log(np.exp(lg - lg.max()).sum()) + lg.max() - lg[0]
    assert abs(lh.loss_head(0.07, 0.05, 1.0, emb.double(), ta, tp, tn)[0].item() - want) < 1e-12


def test_loss_head_float32_reproduces_the_reference_values():
    g = load_golden("g14_loss_head_edges")
    assert [str(t) for t in g["tags"]] == [e[0] for e in lh.g14_entries()]
    for tag, regime, B, d, tau, lam in lh.g14_entries():
        emb, ta, tp, tn = lh.make_inputs(regime, B, d)
        assert np.array_equal(emb.numpy(), g[tag + ":emb"]) and np.array_equal(torch.stack([ta, tp, tn]).numpy(), g[tag + ":time"])
        assert tuple(g[tag + ":hyper"]) == (tau, lam)
        cl, au = lh.loss_head(tau, lam, 1.0, emb, ta, tp, tn)
        want = g[tag + ":losses"]
        assert want[1] == want[2]                                  # rebuilt mask == passed mask
        err = lh.loss_err([cl.item(), au.item()], want[:2])
        assert err < 1e-5, (tag, cl.item(), au.item(), want)


def test_yardstick_and_caps_come_from_the_reference_alone():
    """Which cases carry the fixed caps (element-wise ratio < 1, loss error < 1e-5) is computed: only where the float32 reference
    meets them with K to spare.  No case is degenerate (a float64 gradient that is itself rounding noise is no yardstick)."""
    ys = {c: lh.yardstick(c) for c in lh.CASES}
    for c, y in ys.items():
        assert y.caps == (K * y.ew_ref < 1 and K * y.lerr_ref < 1e-5)
        assert np.isfinite(y.grad64).all() and np.isfinite(y.losses64).all()
        assert np.abs(y.grad64).max() > 0 or y.e_ref == 0           # all decays underflow at tgap with alpha = 0: exactly zero in both
        assert y.e_ref < 1e-3, (lh.case_id(c), y.e_ref)
        gb, lb = lh.bounds(c)
        assert gb == K * max(y.e_ref, E_FLOOR) and lb == K * max(y.lerr_ref, E_FLOOR)
        if c.alpha == 0:
            assert y.losses64[1] == 0 and not y.grad64[3:].any()
    capped = [c for c in lh.CASES if ys[c].caps]
    assert 3 * len(capped) >= 2 * len(lh.CASES), (len(capped), len(lh.CASES))
    for c in lh.CASES:
        if c.regime in ("unit", "dups", "zero"):
            assert ys[c].caps, (lh.case_id(c), ys[c].ew_ref, ys[c].lerr_ref)
    c = max(capped, key=lambda c: ys[c].ew_ref)
    print(f"{len(capped)} of {len(lh.CASES)} cases carry the caps; worst capped reference ratio {ys[c].ew_ref:.3f} ({lh.case_id(c)})")
    assert elementwise_err(ys[c].grad64, ys[c].grad64) == 0
