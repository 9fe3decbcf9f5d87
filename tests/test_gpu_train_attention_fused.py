"""The opt-in fused training attention on the GPU (``attention_kernel="fused"``, ``r4d_set_train_attention_fused``,
csrc/attention_train_fused.hip): the kernels alone through the single-op entries -- against float64 attention and its autograd on the
bf16-rounded q, k, v, dO, gated at 2 x the error of the unfused chain of the ``+attn`` products on the same inputs; planted logits
across key tiles; the dropout mask bit for bit; isolation and determinism; refusals -- and the three training steps under it.

The step helpers are those of tests/test_gpu_train_bf16.py, the gates' tables those of tests/_train_bf16_attn_ref.py.  Every test
restores the switches it found."""
import ctypes
import math
import statistics

import pytest
import torch

import _train_modes
import _attention_ref as AR
import _train_bf16_attn_ref as A
import _train_bf16_ref as R
import test_gpu_train_bf16 as TB
from _poison import HUGE, NAN, ONE, ZERO, poison

pytestmark = pytest.mark.gpu

FUSED_PREFIX = "tuning:train_attn_fused:"
ATTN_PREFIX = "tuning:train_bf16_attn:"
LM, ENC, GEN = TB.LM, TB.ENC, TB.GEN
SENTINEL = -7777.25
GUARD = 64
DROP = (0.1, 0.1, 0.1)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


restore_switches = _train_modes.switches_restored(ops_too=True)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------- the kernels alone
# (B, H, T, hd): every T of {1, 4, 17, 63, 64, 65, 127, 128, 129, 257} and every hd of {16, 48, 64, 96, 128, 256}, crossed sparsely: T
# below / at / above the 32-key tile, the 64- and 128-key dK/dV workgroups and the 128-query workgroup; one and several sequences
SHAPES = [(1, 1, 1, 16), (2, 2, 4, 16), (2, 3, 17, 48), (1, 2, 63, 64), (1, 2, 64, 96), (1, 2, 65, 128), (1, 1, 127, 256),
          (1, 2, 128, 64), (3, 2, 129, 96), (1, 2, 257, 128), (1, 1, 129, 256), (2, 1, 257, 48), (1, 1, 1024, 64)]


def heads(x, H):
    """[B, T, H hd] -> [B, H, T, hd]"""
    B, T, d = x.shape
    return x.view(B, T, H, d // H).permute(0, 2, 1, 3)


def merged(x):
    """[B, H, T, hd] -> [B, T, H hd]"""
    B, H, T, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, T, H * hd)


def make_inputs(dev, B, H, T, hd, seed=0):
    g = torch.Generator().manual_seed(1000 * T + 10 * hd + B + H + 100000 * seed)
    qkv = torch.randn(B, T, 3 * H * hd, generator=g).to(dev)
    dao = (torch.randn(B, T, H * hd, generator=g) * 1e-3).to(dev)            # a gradient's scale
    return qkv, dao


def keep_mask(dev, B, H, T, p, seed, step, site, base):
    """[B, H, T, T] of {0, 1}: r4d_dropout_f32 of a ones block at index_base + (bh T + i) ld + j"""
    from rag4dyg_amd import _lib, ops
    ld = ops.train_attn_probs_ld(T)
    ones = torch.ones(B * H * T * ld, dtype=torch.float32, device=dev)
    out = torch.empty_like(ones)
    _lib.check(_lib.load().r4d_dropout_f32(ones.data_ptr(), None, ones.numel(), out.data_ptr(), p, seed, step, site, base, _stream()), "dropout")
    return (out.view(B, H, T, ld)[..., :T] != 0).double()


def reference64(qkv, dao, H, keep=None, p=0.0):
    """float64 causal attention and its autograd on the bf16-rounded q, k, v, dO -> dict(O, lse, dq, dk, dv, floors): floors are the
    (K + 2) 2^-24 sum |a| |b| terms of the four outputs' products, ABSOLUTE (max-norm)"""
    B, T, d3 = qkv.shape
    d, hd = d3 // 3, d3 // 3 // H
    q, k, v = (heads(x.bfloat16().double(), H).detach().requires_grad_(True) for x in qkv.split(d, dim=2))
    go = heads(dao.bfloat16().double(), H)
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(hd)
    causal = torch.tril(torch.ones(T, T, dtype=torch.bool, device=qkv.device))
    s = s.masked_fill(~causal, float("-inf"))
    P = torch.softmax(s, dim=-1)
    Pd = P if keep is None else P * keep / (1.0 - p)
    O = torch.matmul(Pd, v)
    O.backward(go)
    with torch.no_grad():
        scale = 1.0 if keep is None else keep / (1.0 - p)
        gP = torch.matmul(go, v.transpose(-1, -2)) * scale
        dS = (P * (gP - (P * gP).sum(-1, keepdim=True)) / math.sqrt(hd)).abs()
        eps = 2.0 ** -24
        # dS = P (g - D) cancels g = dO . V^T against D = rowsum(P o g), both built on fp32 sums of hd terms of |dO| |V| size (D's terms
        # reach |dO| |O| through P . V): their accumulation floors, times P / sqrt(hd), pass through the dQ and dK products
        ddS = P * (hd + 2) * eps * (torch.matmul(go.abs(), v.abs().transpose(-1, -2)) * scale + (go.abs() * O.detach().abs()).sum(-1, keepdim=True)) / math.sqrt(hd)
        floors = {"O": (T + 2) * eps * float(torch.matmul(Pd.abs(), v.abs()).max()),
                  "dq": (T + 2) * eps * float(torch.matmul(dS, k.abs()).max()) + float(torch.matmul(ddS, k.abs()).max()),
                  "dk": (T + 2) * eps * float(torch.matmul(dS.transpose(-1, -2), q.abs()).max()) + float(torch.matmul(ddS.transpose(-1, -2), q.abs()).max()),
                  "dv": (T + 2) * eps * float(torch.matmul(Pd.abs().transpose(-1, -2), go.abs()).max())}
        sqk = float(torch.matmul(q.abs(), k.abs().transpose(-1, -2)).max()) / math.sqrt(hd)
    return dict(O=O.detach(), lse=torch.logsumexp(s, dim=-1).detach(), dq=q.grad, dk=k.grad, dv=v.grad, floors=floors,
                s_floor=(hd + 2) * 2.0 ** -24 * sqk)


def run_fused(dev, qkv, dao, H, dropout=None, site=0, base=0):
    """-> dict(O, lse, dq, dk, dv) as [B, H, T, ...] float64 views of the fused single ops' outputs"""
    from rag4dyg_amd import ops
    B, T, d3 = qkv.shape
    d = d3 // 3
    att, lse = ops.train_attn_fused_fwd(qkv, B, T, H, d, dropout=dropout, site=site, index_base=base)
    dqkv = ops.train_attn_fused_bwd(qkv, att, lse, dao, B, T, H, d, dropout=dropout, site=site, index_base=base)
    torch.cuda.synchronize()
    dq, dk, dv = (heads(x, H).double() for x in dqkv.split(d, dim=2))
    return dict(O=heads(att, H).double(), lse=lse.view(B, H, T).double(), dq=dq, dk=dk, dv=dv, raw=(att, lse, dqkv))


def run_unfused(dev, qkv, dao, H, dropout=None, site=0, base=0):
    """The parent's chain on the same inputs: the six ``ops.train_attn_product_bf16`` products around an fp32 causal softmax (torch, on
    the device), ``r4d_dropout_f32`` and the recompute mode's two backward row kernels -> dict(O, dq, dk, dv)"""
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    B, T, d3 = qkv.shape
    d, hd = d3 // 3, d3 // 3 // H
    ld = ops.train_attn_probs_ld(T)
    p, seed, step = dropout if dropout is not None else (0.0, 0, 0)
    S = torch.zeros(B * H, T, ld, dtype=torch.float32, device=dev)
    ops.train_attn_product_bf16("s", qkv, qkv[0, 0, d:], S, B, T, H, d)
    causal = torch.tril(torch.ones(T, T, dtype=torch.bool, device=dev))
    P = torch.zeros_like(S)
    P[..., :T] = torch.softmax(S[..., :T].masked_fill(~causal, float("-inf")), dim=-1)
    Pd = P
    if p > 0:
        Pd = torch.empty_like(P)
        _lib.check(lib.r4d_dropout_f32(P.data_ptr(), None, P.numel(), Pd.data_ptr(), p, seed, step, site, base, _stream()), "dropout")
    att = torch.empty(B, T, d, dtype=torch.float32, device=dev)
    ops.train_attn_product_bf16("pv", Pd, qkv[0, 0, 2 * d:], att, B, T, H, d)
    dP = torch.zeros_like(S)
    ops.train_attn_product_bf16("dp", dao, qkv[0, 0, 2 * d:], dP, B, T, H, d)
    dST, PdT = torch.zeros_like(S), torch.zeros_like(S)
    _lib.check(lib.r4d_softmax_dropout_bwd_transpose_f32(P.data_ptr(), dP.data_ptr(), dST.data_ptr(), B * H, T, ld, math.sqrt(hd), p, seed, step,
                                                         site, base, _stream()), "softmax_bwd_t")
    dqkv = torch.empty(B, T, 3 * d, dtype=torch.float32, device=dev)
    ops.train_attn_product_bf16("dq", dP, qkv[0, 0, d:], dqkv, B, T, H, d)
    ops.train_attn_product_bf16("dk", dST, qkv, dqkv[0, 0, d:], B, T, H, d)
    _lib.check(lib.r4d_dropout_transpose_f32(P.data_ptr(), PdT.data_ptr(), B * H, T, ld, p, seed, step, site, base, _stream()), "dropout_t")
    ops.train_attn_product_bf16("dv", PdT, dao, dqkv[0, 0, 2 * d:], B, T, H, d)
    torch.cuda.synchronize()
    dq, dk, dv = (heads(x, H).double() for x in dqkv.split(d, dim=2))
    return dict(O=heads(att, H).double(), dq=dq, dk=dk, dv=dv)


def two_x_gate(tag, fused, unfused, ref):
    """e_fused <= 2 e_unfused + floor for each of O, dQ, dK, dV: max-norm errors, printed relative to the tensor's max-abs and compared as
    absolute numbers (the same inequality; dQ and dK ARE zero at T = 1, where only the floor is left)"""
    bad = {}
    for n in ("O", "dq", "dk", "dv"):
        ef, eu, fl = float((fused[n] - ref[n]).abs().max()), float((unfused[n] - ref[n]).abs().max()), ref["floors"][n]
        m = max(float(ref[n].abs().max()), 1e-300)
        print(f"[train_attn_fused] {tag} {n}: e_fused {ef / m:.3e} e_unfused {eu / m:.3e} floor {fl / m:.1e} (relative to max-abs {m:.2e}) "
              f"ratio {ef / max(eu, 1e-300):.3f}")
        assert math.isfinite(ef)
        if not ef <= 2.0 * eu + fl:
            bad[n] = (ef, eu, fl)
    assert not bad, f"{tag}: (e_fused, e_unfused, floor) outside e_fused <= 2 e_unfused + floor: {bad}"


def lse_tolerance(ref):
    """|lse - lse64|: the logits' fp32 accumulation ((hd + 2) 2^-24 sum |q| |k| / sqrt(hd), as the product test's floor), the fast
    exponential's argument rounding (|x| 2^-24 at |x| <= ~100: 2^-17 relative per term) and the fp32 sum over up to 1024 terms
    (2^-14 relative at worst) -- together below 2^-13 on log(l) -- and the final fp32 rounding of m + log(l) (2^-23 |lse|)"""
    return ref["s_floor"] + 2.0 ** -13 + 2.0 ** -22 * float(ref["lse"].abs().max())


@pytest.mark.parametrize("shape", SHAPES, ids=["B{}H{}T{}hd{}".format(*s) for s in SHAPES])
def test_01_fused_against_float64_at_twice_the_unfused_chains_error(dev, shape):
    B, H, T, hd = shape
    qkv, dao = make_inputs(dev, B, H, T, hd)
    ref = reference64(qkv, dao, H)
    fused, unfused = run_fused(dev, qkv, dao, H), run_unfused(dev, qkv, dao, H)
    two_x_gate("B{}H{}T{}hd{}".format(*shape), fused, unfused, ref)
    e = float((fused["lse"] - ref["lse"]).abs().max())
    print(f"[train_attn_fused] lse: largest |error| {e:.2e}, tolerance {lse_tolerance(ref):.2e}")
    assert e <= lse_tolerance(ref)


def plant_swing(B, T, H, hd, g):
    """Maxima rising and falling by more than 80 from one 32-key tile to the next: key j has the logit 85 ((j // 32) % 3) for every
    query -- tiles at 0, 85, 170, 0, 85, ... -- on the low-rank frame of ``_attention_ref.plant`` (q[..., 0] = sqrt(hd), k[..., 0] = c_j)"""
    qkv = AR.plant(B, T, H, hd, "flat", g).view(B, T, 3, H, hd)
    qkv[:, :, 0] = 0.05 * torch.randn(B, T, H, hd, generator=g)
    qkv[:, :, 0, :, 0] = math.sqrt(hd)
    qkv[:, :, 1] = 0.05 * torch.randn(B, T, H, hd, generator=g)
    qkv[:, :, 1, :, 0] = (85.0 * ((torch.arange(T) // 32) % 3)).view(1, T, 1)
    qkv[:, :, 2] = torch.randn(B, T, H, hd, generator=g)
    return qkv.view(B, T, 3 * H * hd)


PLANTED = [("spike", 2, 3, 200, 64), ("swing", 1, 2, 257, 128), ("swing", 1, 2, 200, 64), ("wide", 1, 2, 200, 64), ("dead", 2, 2, 300, 64),
           ("flat", 1, 2, 130, 64)]


@pytest.mark.parametrize("case", PLANTED, ids=["{}-B{}H{}T{}hd{}".format(*c) for c in PLANTED])
def test_02_planted_logits_across_key_tiles(dev, case):
    """A dominating key on a tile boundary (spike: keys 31, 32, 127, 128, T - 1, 0 by (sequence, head)), maxima rising and falling by
    85 / 170 from tile to tile (swing), groups that underflow (wide, dead) and all-equal logits (flat: a plain mean).  O and lse
    against float64 of the bf16-rounded inputs.  O's bound per element: the probabilities are rounded to bf16 once (2^-9 relative
    each, 2^-8 granted for the rounding before the normalisation), the logits carry their fp32 accumulation error s_floor, which
    moves a probability by at most 2 s_floor relative, plus the exponential's and the sum's 2^-13 (``lse_tolerance``): all times
    sum_j P_ij |v_j|.  A missing rescale, a wrong mask or a dropped tile moves these cases by orders of magnitude more."""
    pattern, B, H, T, hd = case
    g = torch.Generator().manual_seed(7 * T + hd)
    qkv = (plant_swing(B, T, H, hd, g) if pattern == "swing" else AR.plant(B, T, H, hd, pattern, g)).to(dev)
    dao = torch.zeros(B, T, H * hd, device=dev)
    ref = reference64(qkv, dao + 1e-3, H)
    got = run_fused(dev, qkv, dao + 1e-3, H)
    assert torch.isfinite(got["O"]).all() and torch.isfinite(got["lse"]).all()
    d = H * hd
    v = heads(qkv[..., 2 * d:].bfloat16().double(), H)
    q, k = (heads(x.bfloat16().double(), H) for x in (qkv[..., :d], qkv[..., d:2 * d]))
    s = (torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(hd)).masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool, device=dev)), float("-inf"))
    bound = (2.0 ** -8 + 2.0 * ref["s_floor"] + 2.0 ** -13) * torch.matmul(torch.softmax(s, -1), v.abs())
    worst = float(((got["O"] - ref["O"]).abs() / bound.clamp_min(1e-300)).max())
    e = float((got["lse"] - ref["lse"]).abs().max())
    print(f"[train_attn_fused] planted {pattern} T{T} hd{hd}: O largest |error| / bound {worst:.3f}; lse |error| {e:.2e} (tolerance {lse_tolerance(ref):.2e})")
    assert worst <= 1.0 and e <= lse_tolerance(ref)
    if pattern == "flat":                                                      # the plain mean: column 0 = 1, column 1 = i / 2
        i = torch.arange(T, dtype=torch.float64, device=dev)
        assert float((got["O"][..., 0] - 1.0).abs().max()) <= 2.0 ** -8
        assert float(((got["O"][..., 1] - i / 2).abs() / (i / 2 + 1)).max()) <= 2.0 ** -8
        assert float((got["lse"] - torch.log(i + 1)).abs().max()) <= 2.0 ** -13 + 2.0 ** -20


@pytest.mark.parametrize("shape", [(1, 2, 33, 64), (1, 1, 130, 256)], ids=("B1H2T33hd64", "B1H1T130hd256"))
def test_03_dropout_mask_bit_for_bit(dev, shape):
    """q = k = 0 (every probability of row i is 1 / (i + 1)) and V rows one-hot (T <= hd): O[i, j] (i + 1) (1 - p) is the mask of element
    (i, j) -- 1 / (i + 1) rounds to bf16 relative 2^-9, far from the 0 / 1 decision at 0.5 -- and must equal r4d_dropout_f32 of a ones
    block at the same site, seed, step and index_base + (bh T + i) ld + j, with a non-zero index_base."""
    B, H, T, hd = shape
    d = H * hd
    p, seed, step, site, base = 0.1, 1234567, 9, 5, 4 * 1031
    qkv = torch.zeros(B, T, 3, H, hd, device=dev)
    qkv[:, :, 2] = torch.eye(T, hd, device=dev).view(1, T, 1, hd)
    qkv = qkv.view(B, T, 3 * d)
    got = run_fused(dev, qkv, torch.zeros(B, T, d, device=dev), H, dropout=(p, seed, step), site=site, base=base)
    i = torch.arange(T, dtype=torch.float64, device=dev).view(1, 1, T, 1)
    rec = got["O"][..., :T] * (i + 1) * (1 - p)
    keep = keep_mask(dev, B, H, T, p, seed, step, site, base)
    tril = torch.tril(torch.ones(T, T, dtype=torch.bool, device=dev))
    assert float((rec - rec.round()).abs().max()) < 0.01
    assert torch.equal(rec.round()[..., tril], keep[..., tril])
    assert 0.02 < 1.0 - float(keep[..., tril].mean()) < 0.25                   # something was dropped, about p of it
    assert bool((rec.round()[..., ~tril] == 0).all())


@pytest.mark.parametrize("shape", [(2, 2, 129, 64), (1, 2, 65, 128), (1, 1, 257, 256), (2, 3, 17, 48)], ids=lambda s: "B{}H{}T{}hd{}".format(*s))
def test_03b_dropout_forward_and_backward_at_the_two_x_gate(dev, shape):
    """Random inputs, p = 0.1: the forward and both backward kernels regenerate the mask the unfused chain draws under the same
    struct, so both sit at their rounding error from the float64 reference with that mask."""
    B, H, T, hd = shape
    p, seed, step, site, base = 0.1, 99, 3, 8, 4 * 77
    qkv, dao = make_inputs(dev, B, H, T, hd, seed=1)
    ref = reference64(qkv, dao, H, keep=keep_mask(dev, B, H, T, p, seed, step, site, base), p=p)
    drop = (p, seed, step)
    two_x_gate("dropout B{}H{}T{}hd{}".format(*shape), run_fused(dev, qkv, dao, H, drop, site, base), run_unfused(dev, qkv, dao, H, drop, site, base), ref)


def guarded(dev, n, fill):
    raw = torch.full((GUARD + n + GUARD,), fill, dtype=torch.float32, device=dev)
    return raw, raw[GUARD:GUARD + n]


def test_04_isolation_and_determinism(dev):
    """One sequence computed in the middle of buffers whose neighbouring sequences' rows and guards hold NaN (inputs) or a sentinel
    (outputs): the same bits as inside the full batch, nothing else written; two runs and a poisoned workspace give the same bits;
    NaN in another head's columns of qkv / dao reaches only that head's outputs."""
    from rag4dyg_amd import ops
    drop, site, base = (0.1, 5, 2), 4, 0
    for B, H, T, hd in ((3, 2, 65, 64), (3, 1, 129, 256), (3, 3, 33, 48)):
        d = H * hd
        ld = ops.train_attn_probs_ld(T)
        qkv, dao = make_inputs(dev, B, H, T, hd, seed=2)
        full = run_fused(dev, qkv, dao, H, drop, site, base)
        again = run_fused(dev, qkv, dao, H, drop, site, base)
        for n in ("O", "lse", "dq", "dk", "dv"):
            assert torch.equal(full[n], again[n]), (n, "two runs")
        # sequence 1 alone: NaN rows around it, sentinel-filled guarded outputs; its dropout indices are those of bh = H .. 2H - 1
        nq, nd = qkv.clone(), dao.clone()
        nq[0] = nq[2] = float("nan")
        nd[0] = nd[2] = float("nan")
        att_raw, att = guarded(dev, 3 * T * d, SENTINEL)
        lse_raw, lse = guarded(dev, 3 * H * T, SENTINEL)
        dq_raw, dqkv = guarded(dev, 3 * T * 3 * d, SENTINEL)
        att, lse, dqkv = att.view(3, T, d), lse.view(3 * H, T), dqkv.view(3, T, 3 * d)
        b1 = base + H * T * ld
        ops.train_attn_fused_fwd(nq[1], 1, T, H, d, att=att[1], lse=lse[H], dropout=drop, site=site, index_base=b1)
        nbytes = int(ops._lib.load().r4d_train_attn_fused_bwd_workspace_bytes(1, T, H, d))
        outs = []
        for pattern in (ZERO, NAN, HUGE, ONE):
            ws = poison(torch.empty(nbytes, dtype=torch.uint8, device=dev), pattern)
            dqkv[1] = SENTINEL
            ops.train_attn_fused_bwd(nq[1], att[1], lse[H], nd[1], 1, T, H, d, dqkv=dqkv[1], dropout=drop, site=site, index_base=b1, workspace=ws)
            torch.cuda.synchronize()
            outs.append(dqkv[1].clone())
        for o in outs[1:]:
            assert torch.equal(outs[0], o), "the workspace's content reached the result"
        assert torch.equal(heads(att[1:2], H).double(), full["O"][1:2]) and torch.equal(lse[H:2 * H].double(), full["lse"][1])
        for n, x in zip(("dq", "dk", "dv"), dqkv[1:2].split(d, dim=2)):
            assert torch.equal(heads(x, H).double(), full[n][1:2]), (n, "bits depend on the batch")
        for raw, body, own in ((att_raw, att, att[1]), (lse_raw, lse, lse[H:2 * H]), (dq_raw, dqkv, dqkv[1])):
            own.fill_(SENTINEL)
            assert bool((raw == SENTINEL).all()), "wrote outside its own rows"
        if H > 1:                                                              # NaN in head 1's columns: head 0 keeps its bits
            hq, hdao = qkv.clone(), dao.clone()
            hq.view(B, T, 3, H, hd)[:, :, :, 1] = float("nan")
            hdao.view(B, T, H, hd)[:, :, 1] = float("nan")
            hn = run_fused(dev, hq, hdao, H, drop, site, base)
            for n in ("O", "lse", "dq", "dk", "dv"):
                assert torch.equal(hn[n][:, 0], full[n][:, 0]), (n, "another head's NaN leaked")
                if H > 2:
                    assert torch.equal(hn[n][:, 2], full[n][:, 2]), n


def test_05_refusals_before_any_launch(dev):
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    before = TB.hits(FUSED_PREFIX)
    x = torch.zeros(1 << 16, device=dev)
    for B, T, H, d in ((1, 8, 1, 24), (1, 8, 1, 272), (1, 0, 1, 64), (1, 1025, 1, 64), (65536, 1, 1, 16), (1, 8, 3, 64)):
        with pytest.raises(_lib.R4DError, match="bad shape"):
            ops.train_attn_fused_fwd(x, B, T, H, d, att=x, lse=x)
        with pytest.raises(_lib.R4DError, match="bad shape"):
            ops.train_attn_fused_bwd(x, x, x, x, B, T, H, d, dqkv=x)
    stream = _stream()
    assert lib.r4d_train_attn_fused_fwd_f32(None, 1, 8, 1, 64, x.data_ptr(), x.data_ptr(), None, 0, 0, stream) != 0
    assert lib.r4d_train_attn_fused_fwd_f32(x.data_ptr(), 1, 8, 1, 64, x.data_ptr(), None, None, 0, 0, stream) != 0
    ws = torch.empty(4096, dtype=torch.uint8, device=dev)
    assert lib.r4d_train_attn_fused_bwd_f32(x.data_ptr(), x.data_ptr(), None, x.data_ptr(), 1, 8, 1, 64, x.data_ptr(), None, 0, 0, ws.data_ptr(), 4096, stream) != 0
    need = int(lib.r4d_train_attn_fused_bwd_workspace_bytes(2, 100, 2, 128))
    assert need >= 4 * 2 * 2 * 100
    with pytest.raises(_lib.R4DError, match="workspace"):
        ops.train_attn_fused_bwd(x, x, x, x, 2, 100, 2, 128, dqkv=x, workspace=torch.empty(need - 4, dtype=torch.uint8, device=dev))
    with pytest.raises(_lib.R4DError):                                          # an index base that splits a Philox block
        ops.train_attn_fused_fwd(x, 1, 8, 1, 64, att=x, lse=x, dropout=(0.1, 1, 1), index_base=2)
    torch.cuda.synchronize()
    assert TB.hits(FUSED_PREFIX) == before, "a refused call launched"


# ------------------------------------------------------------------------------------------------------------------ the steps
def fused_stepper(monkeypatch, dev, c, precision, **kw):
    """TB.stepper with attention_kernel="fused": the trainers read R4D_TRAIN_ATTENTION_KERNEL where the keyword is None"""
    monkeypatch.setenv("R4D_TRAIN_ATTENTION_KERNEL", "fused")
    tr, step = TB.stepper(dev, c, precision, **kw)
    monkeypatch.delenv("R4D_TRAIN_ATTENTION_KERNEL")
    assert (tr.enc if hasattr(tr, "enc") else tr).attention_kernel == "fused"
    return tr, step


def step_errors(out, exact):
    got = {"loss": float(out["loss"]), "grads": {n: t.detach().cpu().double().numpy() for n, t in out["grads"].items()}}
    for k in ("emb", "hidden"):
        if out.get(k) is not None:
            got[k] = out[k].detach().cpu().double().numpy()
    assert set(got["grads"]) == set(exact["grads"])
    return R.errors(got, exact)


def upper_gate(c, mode, e, e_unfused):
    """Every gated quantity of the case inside the project's own upper gate e_gpu <= K max(e_emu32, e_emu64) against the exact float64
    step, K and the tables from the emulations of tests/_train_bf16_attn_ref.py alone; -> the gated e_fused / e_unfused ratios"""
    K, tab = A.margin(mode), A.error_table(c, mode)
    assert set(e) == set(tab)
    bad, ratios = {}, []
    for n, t in tab.items():
        if t["emu64"] < R.GATE_FLOOR:
            continue
        ratios.append(e[n] / max(e_unfused[n], 1e-300))
        if not e[n] <= K * max(t["emu32"], t["emu64"]):
            bad[n] = (e[n], K * max(t["emu32"], t["emu64"]))
    assert len(ratios) >= A.MIN_GATED, (mode, R.case_id(c), len(ratios))
    print(f"[train_attn_fused] {mode} {R.case_id(c)}: K {K:.2f}, {len(ratios)} gated, e_fused / e_unfused median {statistics.median(ratios):.3f} "
          f"extremes {min(ratios):.3f} .. {max(ratios):.3f}")
    assert not bad, f"{mode} {R.case_id(c)}: (e_gpu, K max(e_emu32, e_emu64)) outside the gate: {bad}"


@pytest.mark.parametrize("c", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_06_step_against_the_exact_oracle_inside_the_projects_gate(dev, monkeypatch, c):
    """"bf16+attn" with the fused kernels: retriever, LM, frozen and unfrozen generator steps of every weight set."""
    _tr, unfused = TB.stepper(dev, c, "bf16+attn")
    eu = step_errors(unfused(), R.references(c)[0])
    _tr, step = fused_stepper(monkeypatch, dev, c, "bf16+attn")
    b0, b1 = TB.hits(FUSED_PREFIX), TB.hits(ATTN_PREFIX)
    out = step()
    assert TB.hits(ATTN_PREFIX) == b1 and all(v > b0[n] for n, v in TB.hits(FUSED_PREFIX).items())
    upper_gate(c, "bf16+attn", step_errors(out, R.references(c)[0]), eu)


ATTN_ONLY = [R.case("L2_d256_T130", k) for k in R.KINDS] + [R.case("g10_trained", "lm")]


@pytest.mark.parametrize("c", ATTN_ONLY, ids=[R.case_id(c) for c in ATTN_ONLY])
def test_06b_attention_alone_under_gemm_mode_f32(dev, monkeypatch, c):
    """"fp32+attn" under gemm mode f32 (every other GEMM exact): the attention-only emulation's tables and K."""
    from rag4dyg_amd import ops
    ops.set_gemm_mode("f32")
    _tr, unfused = TB.stepper(dev, c, "fp32+attn")
    eu = step_errors(unfused(), R.references(c)[0])
    _tr, step = fused_stepper(monkeypatch, dev, c, "fp32+attn")
    upper_gate(c, "fp32+attn", step_errors(step(), R.references(c)[0]), eu)


def profile_counts(step):
    from rag4dyg_amd import _lib
    lib = _lib.load()
    _lib.check(lib.r4d_profile_enable(1), "profile_enable")
    try:
        step()
        torch.cuda.synchronize()
        out = {}
        for cls in range(lib.r4d_profile_num_classes()):
            ms, n, wk = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
            _lib.check(lib.r4d_profile_read(cls, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(wk)), "profile_read")
            if n.value:
                out[lib.r4d_profile_class_name(cls).decode()] = n.value
    finally:
        _lib.check(lib.r4d_profile_enable(0), "profile_enable")
    return out


def test_07_launch_accounting(dev, monkeypatch):
    """A fused step: per layer and batch one forward launch and the backward's three (row sums, dK / dV, dQ); none of the six bf16
    products, no softmax launch; the layer axis counts what "bf16" counts.  Activations recompute runs the forward launch again for
    every layer but the last.  With the switch off the parent's counts are unchanged."""
    L, G = 2, len(ENC.Bs)

    def delta(before, prefix):
        return {n: v - before[n] for n, v in TB.hits(prefix).items()}
    _t, step = TB.stepper(dev, LM, "bf16+attn")
    b0, b1, b2 = TB.hits(ATTN_PREFIX), TB.hits(FUSED_PREFIX), TB.hits(); step()
    assert delta(b0, ATTN_PREFIX) == {"nt": 2 * L, "nn": 4 * L} and delta(b1, FUSED_PREFIX) == {"fwd": 0, "rowsum": 0, "dkv": 0, "dq": 0}
    layer_axis = TB.delta(b2)
    for c, groups in ((LM, 1), (ENC, G), (GEN, 1)):
        for attention in ("stored", "recompute"):
            _t, step = fused_stepper(monkeypatch, dev, c, "bf16+attn", attention=attention)
            b0, b1, b2 = TB.hits(ATTN_PREFIX), TB.hits(FUSED_PREFIX), TB.hits(); step()
            n = L * groups
            assert delta(b0, ATTN_PREFIX) == {"nt": 0, "nn": 0}
            assert delta(b1, FUSED_PREFIX) == {"fwd": n, "rowsum": n, "dkv": n, "dq": n}, (R.case_id(c), attention)
            if c is LM:
                assert TB.delta(b2) == layer_axis
    _t, step = fused_stepper(monkeypatch, dev, LM, "bf16+attn", activations="recompute")
    b1 = TB.hits(FUSED_PREFIX); step()
    assert delta(b1, FUSED_PREFIX) == {"fwd": L + (L - 1), "rowsum": L, "dkv": L, "dq": L}
    step()
    counts = profile_counts(step)
    print(f"[train_attn_fused] profile classes of a fused LM step: {counts}")
    assert counts.get("attn_train_fused_fwd") == L + (L - 1) and counts.get("attn_train_fused_dkv") == L and counts.get("attn_train_fused_dq") == L
    assert "causal_softmax" not in counts and "gemm_bf16h_nt" not in counts and "gemm_bf16h_nn" not in counts


@pytest.mark.parametrize("c", (ENC, LM, GEN), ids=("enc", "lm", "gen"))
def test_08_combinations_give_the_same_bits(dev, monkeypatch, c):
    """Activations stored / recompute and the (ineffective) attention word: one set of bits; a repeated step and a step on a poisoned
    workspace under the same dropout struct: the same bits; and they are not the unfused step's."""
    base = None
    for attention, activations in (("stored", "stored"), ("recompute", "stored"), ("stored", "recompute"), ("recompute", "recompute")):
        tr, step = fused_stepper(monkeypatch, dev, c, "bf16+attn", dropout=DROP, attention=attention, activations=activations, seed=5)
        s = TB.snapshot(step())
        if base is None:
            base = s
        else:
            TB.assert_same_bits(base, s, (attention, activations))
    _t, unfused = TB.stepper(dev, c, "bf16+attn", dropout=DROP, seed=5)
    u = TB.snapshot(unfused())
    assert any(not torch.equal(u[n], base[n]) for n in u), "the fused step gave the unfused step's bits"
    tr, step = fused_stepper(monkeypatch, dev, c, "bf16+attn")
    first = TB.snapshot(step())
    TB.assert_same_bits(first, TB.snapshot(step()), "a repeated step")
    for pattern in (NAN, HUGE, ONE):
        ws = tr._ws
        assert ws is not None
        poison(ws, pattern)
        TB.assert_same_bits(first, TB.snapshot(step()), ("workspace", pattern))


def test_08b_frozen_generator_step_equals_the_unfrozen_fused_steps_bits(dev, monkeypatch):
    m = TB.model_of(dev, GEN)
    _t, frozen = fused_stepper(monkeypatch, dev, GEN, "bf16+attn", dropout=DROP, freeze=True, seed=5, model=m)
    f = TB.snapshot(frozen())
    _t, free = fused_stepper(monkeypatch, dev, GEN, "bf16+attn", dropout=DROP, freeze=False, seed=5, model=m)
    u = TB.snapshot(free())
    assert {"loss", "hidden", "grads:lm_head.weight", "grads:gnn_fusion.convs.0.lin.weight", "grads:gnn_fusion.convs.0.bias"} <= set(f)
    for n in f:
        assert torch.equal(f[n], u[n]), n


def test_09_refusals_of_the_steps(dev):
    from rag4dyg_amd import _lib, training
    from rag4dyg_amd.lm_training import LMTrainer
    x = R.inputs(ENC)
    ids, G = [t.to(dev) for t in x["ids"]], x["G"].to(dev)
    for first, second in (("fused", "products"), ("products", "fused")):
        tr = training.EncoderTrainer(TB.model_of(dev, ENC), precision="bf16+attn", attention_kernel=first)
        tr.forward(ids)
        tr.attention_kernel = second
        with pytest.raises(_lib.R4DError, match="train-attention-fused"):
            tr.backward(G)
        tr.attention_kernel = first
        tr.forward(ids)
        tr.backward(G)                                                     # the matching pair goes through
    # the library's own refusal of the switch without the bf16 attention products (the trainers raise before they get there)
    tr = training.EncoderTrainer(TB.model_of(dev, ENC), precision="bf16+attn", attention_kernel="fused")
    tr.precision = "bf16"
    with pytest.raises(_lib.R4DError):                                     # the size query answers 0
        tr.forward(ids)
    m = TB.model_of(dev, LM)
    for precision in ("fp32", "bf16"):
        with pytest.raises(ValueError, match="fused"):
            LMTrainer(m, precision=precision, attention_kernel="fused")


def test_10_a_short_training_run(dev):
    """30 AdamW steps of LMTrainer on L2 d256, B 8, T 40 (the run of test_gpu_train_bf16_attn.py::test_09) in "bf16", "bf16+attn" and
    "bf16+attn" with the fused kernels: every loss finite, the loss falls, and the fused run ends within the spread the first two
    show -- no further from their interval than their own distance |bf16 - bf16+attn| of this very run."""
    from rag4dyg_amd import training
    from rag4dyg_amd.lm_training import LMTrainer
    c = R.case("L2_d256_T130", "lm")
    V = R.weights(c.weights)[0]["transformer.wte.weight"].shape[0]
    ids = torch.randint(0, V - 2, (8, 40), generator=torch.Generator().manual_seed(77)).to(dev)
    losses = {}
    for name, precision, kernel in (("bf16", "bf16", "products"), ("bf16+attn", "bf16+attn", "products"), ("fused", "bf16+attn", "fused")):
        tr = LMTrainer(TB.model_of(dev, c).train(), dropout=DROP, seed=3, precision=precision, attention_kernel=kernel)
        opt = training.AdamW(tr.params, tr.grads, lr=1e-3, weight_decay=0.01, flat_grads=tr.flat_grads)
        ls = []
        for _ in range(30):
            ls.append(tr.step(ids))
            opt.step(max_grad_norm=1.0)
        losses[name] = [float(v) for v in torch.stack(ls).cpu()]
    a, b, f = losses["bf16"], losses["bf16+attn"], losses["fused"]
    print("[train_attn_fused] 30 steps, loss at steps 1, 10, 20, 30: " +
          "; ".join(f"{n} {ls[0]:.4f} {ls[9]:.4f} {ls[19]:.4f} {ls[29]:.4f}" for n, ls in losses.items()))
    spread = abs(a[-1] - b[-1])
    print(f"[train_attn_fused] final losses bf16 {a[-1]:.5f} bf16+attn {b[-1]:.5f} fused {f[-1]:.5f}; spread |bf16 - bf16+attn| {spread:.2e}, "
          f"|fused - bf16+attn| {abs(f[-1] - b[-1]):.2e}")
    for ls in (a, b, f):
        assert all(math.isfinite(v) for v in ls) and ls[-1] < ls[0], ls
    assert min(a[-1], b[-1]) - spread <= f[-1] <= max(a[-1], b[-1]) + spread
