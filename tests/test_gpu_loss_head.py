"""GPU tests of the retriever loss head (``csrc/losses.hip``, ``r4d_retriever_losses_f32``) at its own edges: every loop of its three
kernels at zero, one and several trips and next to its strides, the input regimes of ``_loss_head_ref.py``, the hyper-parameter
cross -- against float64 autograd of ``_loss_head_ref.loss_head`` (pinned to the oracle and to the reference's values by
``test_host_loss_head.py``, which also establishes every bound used here from the float32 reference alone)."""
import types

import pytest
import torch

import _loss_head_ref as lh
from conftest import elementwise_err, load_golden, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _args(c):
    return types.SimpleNamespace(temperature=c.tau, lambda_decay=c.lam, alpha=c.alpha, per_gpu_train_batch_size=c.B + 1)


def _run(c, dev, inputs, want_grad=True):
    from rag4dyg_amd import training
    emb, ta, tp, tn = inputs
    losses, demb = training.retriever_losses(_args(c), emb.to(dev), ta, tp, tn, grad_scale=c.gscale, want_grad=want_grad)
    return losses.cpu(), (demb.cpu() if want_grad else None)


def _check(c, losses, demb, y, what=""):
    """The yardstick bound always, the fixed caps where the case carries them; every figure printed before it is asserted."""
    gb, lb = lh.bounds(c)
    e_dev, l_dev = rel_err(demb.numpy(), y.grad64), lh.loss_err(losses.numpy(), y.losses64)
    ew = elementwise_err(demb.numpy(), y.grad64)
    print(f"[loss head] {lh.case_id(c)}{what}: e_dev {e_dev:.2e} (e_ref {y.e_ref:.2e}, bound {gb:.2e})  loss {l_dev:.2e} "
          f"(ref {y.lerr_ref:.2e}, bound {lb:.2e})  element-wise {ew:.3f} (ref {y.ew_ref:.3f}) caps {int(y.caps)}")
    assert torch.isfinite(losses).all() and torch.isfinite(demb).all()
    assert e_dev <= gb and l_dev <= lb
    if y.caps:
        assert ew < 1 and l_dev < 1e-5


@pytest.mark.parametrize("c", lh.CASES, ids=lh.CASE_IDS)
def test_losses_and_gradient_equal_float64_autograd(dev, c):
    inputs = lh.make_inputs(c.regime, c.B, c.d)
    y = lh.yardstick(c)
    losses, demb = _run(c, dev, inputs)
    assert demb.shape == (5, c.B, c.d)
    _check(c, losses, demb, y)
    assert losses[2].item() == (losses[0] + losses[1]).item()                      # float32 sum of the two
    again, demb2 = _run(c, dev, inputs)
    assert torch.equal(again, losses) and torch.equal(demb2, demb)                 # same bits on a second launch
    only, none = _run(c, dev, inputs, want_grad=False)
    assert none is None and torch.equal(only, losses)
    if c.alpha == 0:
        assert losses[1].item() == 0 and not demb[3:].any()
    if c.B == 1:
        assert losses[1].item() == 0


def test_times_as_vectors_and_as_columns_give_the_same_bits(dev):
    c = lh.Case("gauss", 9, 64, 0.07, 0.05, 1.0, 1.0)
    emb, ta, tp, tn = lh.make_inputs(c.regime, c.B, c.d)
    l1, g1 = _run(c, dev, (emb, ta, tp, tn))
    l2, g2 = _run(c, dev, (emb, ta.reshape(-1), tp.reshape(-1).double(), tn.reshape(-1)))
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_reference_values_of_the_edge_fixture(dev):
    """tests/golden/g14_loss_head_edges.npz: the reference's own CLtime_loss / info_nce in float32, within 1e-5 relative."""
    g = load_golden("g14_loss_head_edges")
    for tag, regime, B, d, tau, lam in lh.g14_entries():
        c = lh.Case(regime, B, d, tau, lam, 1.0, 1.0)
        emb, t = torch.from_numpy(g[tag + ":emb"]), torch.from_numpy(g[tag + ":time"])
        losses, _ = _run(c, dev, (emb, t[0], t[1], t[2]), want_grad=False)
        want = g[tag + ":losses"]
        err = lh.loss_err(losses.numpy()[:2], want[:2])
        print(f"[g14] {tag}: device {losses.numpy()[:2]} reference {want[:2]} error {err:.2e}")
        assert err < 1e-5, tag


PROPERTY_CASES = [lh.Case("gauss", 9, 64, 0.07, 0.05, 1.0, 1.0), lh.Case("unit", 17, 63, 0.07, 0.05, 0.3, 0.25),
                  lh.Case("zero", 21, 65, 1.0, 0.0, 1.0, 1.0)]


@pytest.mark.parametrize("c", PROPERTY_CASES, ids=[lh.case_id(c) for c in PROPERTY_CASES])
def test_permuting_the_batch_permutes_the_gradient(dev, c):
    """One permutation of the batch rows of all five blocks and the three time vectors: the same sums in another order."""
    emb, ta, tp, tn = lh.make_inputs(c.regime, c.B, c.d)
    perm = torch.randperm(c.B, generator=torch.Generator().manual_seed(c.B))
    assert not torch.equal(perm, torch.arange(c.B))
    y = lh.yardstick(c)
    losses, demb = _run(c, dev, (emb[:, perm].contiguous(), ta[perm], tp[perm], tn[perm]))
    yp = y._replace(grad64=y.grad64[:, perm.numpy()])
    _check(c, losses, demb, yp, " permuted")
    base_l, base_g = _run(c, dev, (emb, ta, tp, tn))
    gb, lb = lh.bounds(c)
    assert lh.loss_err(losses.numpy(), base_l.numpy()) <= 2 * lb
    assert rel_err(demb.numpy(), base_g[:, perm].numpy()) <= 2 * gb


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("where", [(0, 1, 2), (3, 0, 5)], ids=["anchor", "view"])
@pytest.mark.parametrize("c", PROPERTY_CASES[:2], ids=[lh.case_id(c) for c in PROPERTY_CASES[:2]])
def test_non_finite_inputs_stay_loud(dev, c, where, bad):
    emb, ta, tp, tn = lh.make_inputs(c.regime, c.B, c.d)
    emb = emb.clone()
    emb[where] = bad
    cl, au = lh.loss_head(c.tau, c.lam, c.alpha, emb.double(), ta, tp, tn)
    assert not torch.isfinite(cl + au)                             # the float64 truth is non-finite here
    losses, _ = _run(c, dev, (emb, ta, tp, tn))
    assert not torch.isfinite(losses[2])
    for k, ref in ((0, cl), (1, au)):
        if not torch.isfinite(ref):
            assert not torch.isfinite(losses[k])


def test_bad_arguments_are_errors_and_leave_the_losses_untouched(dev):
    from rag4dyg_amd import _lib, training
    lib = _lib.load()
    B, d = 4, 16
    emb, ta, tp, tn = (x.to(dev) for x in lh.make_inputs("gauss", B, d))
    ts = [t.reshape(-1).contiguous() for t in (ta, tp, tn)]
    need = lib.r4d_retriever_losses_workspace_bytes(4097)          # large enough for every B tried below
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(B_, d_, tau, nbytes):
        losses = torch.full((3,), -7.25, dtype=torch.float32, device=dev)
        demb = torch.full_like(emb, -7.25)
        rc = lib.r4d_retriever_losses_f32(emb.data_ptr(), ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), B_, d_, tau, 0.05, 1.0,
                                          1.0, losses.data_ptr(), demb.data_ptr(), ws.data_ptr(), nbytes, stream)
        torch.cuda.synchronize()
        return rc, losses.cpu(), demb.cpu()
    exact = lib.r4d_retriever_losses_workspace_bytes(B)
    rc, losses, demb = call(B, d, 0.07, exact)
    assert rc == 0 and (losses != -7.25).all() and (demb != -7.25).all()             # the good call, at exactly the bytes asked for
    for what, a in (("B = 0", (0, d, 0.07, need)), ("B = 4097", (4097, d, 0.07, need)), ("d = 0", (B, 0, 0.07, need)),
                    ("d = 8193", (B, 8193, 0.07, need)), ("temperature = 0", (B, d, 0.0, need)),
                    ("workspace one byte short", (B, d, 0.07, exact - 1))):
        rc, losses, demb = call(*a)
        assert rc != 0, what
        assert (losses == -7.25).all() and (demb == -7.25).all(), what
        assert lib.r4d_last_error()
    args = types.SimpleNamespace(temperature=0.07, lambda_decay=0.05, alpha=1.0)
    for bad in (ta[:3], torch.cat([ta, ta])):
        with pytest.raises(_lib.R4DError):
            training.retriever_losses(args, emb, bad, tp, tn)
        with pytest.raises(_lib.R4DError):
            training.retriever_losses(args, emb, ta, tp, bad)
