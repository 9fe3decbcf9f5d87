"""Float64 reference, error scale, precision reference and planted defects for the decode step's weight-stream GEMM
(``csrc/gemm_skinny.hip`` through ``ops.conv1d_skinny``); numpy only, runs on the CPU.  Shared by tests/test_host_skinny_gemm.py,
tests/test_gpu_skinny_gemm.py and tests/_skinny8_child.py.

The operation: y[M,N] = epilogue(x' . wT^T + bias), x' = x or LayerNorm(x).  Notation below: ``ln`` is None or (gain, shift, eps).

The error measure.  ``denom`` is, per output element, the sum of the magnitudes of the terms of the formula the kernel evaluates;
one rounding of one term moves the result by at most 2^-24 of it.  ``rho`` = max |got - ref| / (2^-24 denom) is therefore the error
in units of the worst-case rounding of one term, and a chain of D dependent fp32 additions is bounded by about D of those units:
the HARD gate is ``chain_depth + 16`` (the 16: the products' own roundings, the LayerNorm statistics, v_rsq_f32).  The MEASURED
gate is 8 x the rho of ``seq32`` -- the same formula in float32 with k accumulated strictly in order, the longest chain any kernel
form could have -- on the same inputs; the margin of 8 stands for another summation order, for the maximum over up to 32 N
elements, and for the final bias / residual / GELU roundings.  Neither gate comes from what the GPU gives.

For the GELU epilogue the comparison is with ``gelu_new64(ref_pre)`` and the budget is 1.13 x (pre-activation budget) + 3e-7
|ref_pre|: 1.13 bounds |gelu_new'|, 3e-7 |x| is the error documented at gelu_new1 (csrc/gemm_common.h).  ``rho`` folds that in -- it
is max (|got - ref| - 3e-7 |ref_pre|)+ / (1.13 x 2^-24 denom) -- so that both gates read the same for every epilogue, and the
measured gate takes seq32's PRE-activation rho (its own GELU error would vanish inside the 3e-7 allowance)."""
import math

import numpy as np

U = 2.0 ** -24
GELU_SLOPE, GELU_ERR = 1.13, 3e-7
EPILOGUES = ("none", "gelu", "residual")
DEFECTS = ("drop_k", "swap_rows_15_16", "bias_missing_on_ragged_tile", "residual_from_row_above", "stale_column_tile")
LN_EPS = 1e-5


def cdiv(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------------------------- what the dispatcher picks
def form(K, N, skinny16=True):
    """(kernel, ng, KS) that launch_gemm_skinny chooses: "skinny16" / "skinny8" (8 waves, slices of 256 ng) or "plain" (slices of
    256).  ``skinny16`` False: the process runs under R4D_SKINNY16=0."""
    ng = 3 if K % 768 == 0 else (2 if K % 512 == 0 else 0)
    if not ng:
        return "plain", 0, K // 256
    KS = K // (256 * ng)
    if skinny16 and (KS == 1 or cdiv(N, 16) <= 256):
        return "skinny16", ng, KS
    return "skinny8", ng, KS


def chain_depth(M, K, N, skinny16=True):
    """Longest dependent chain of fp32 additions behind one output, read off the kernels: the plain kernel's one accumulator takes
    256 products per slice, a wave of the 8-wave kernels K / (8 KS); then 8 for the waves that meet in LDS, KS for the slices and
    3 for bias, residual and GELU."""
    kind, _ng, KS = form(K, N, skinny16)
    return (256 if kind == "plain" else K // (8 * KS)) + 8 + KS + 3


def hard_gate(M, K, N, skinny16=True):
    return chain_depth(M, K, N, skinny16) + 16


def expected_branches(K, N, ln=None, skinny16=True):
    """Dispatch counter names one launch of the entry increments (each by one).  ``ln``: None, "launch" or "fold"."""
    kind, ng, KS = form(K, N, skinny16)
    if kind == "plain":
        return {"skinny:plain + epilogue launch": 1}
    if kind == "skinny16":
        out = {"skinny16:LayerNorm pre-folded into the weight" if ln == "fold" else f"skinny16:ng{ng}" + ("+layernorm" if ln else ""): 1}
        if KS > 1:
            out["skinny16:split-K last-arriver"] = 1
        return out
    out = {f"skinny8:ng{ng}": 1}
    if ln:
        out["tuning:skinny8:+layernorm"] = 1
    if KS > 1:
        out["skinny8:split-K + epilogue launch"] = 1
    return out


def workspace_bytes(K, N):
    return 4 * (cdiv(K, 256) * 32 * N + 256)


# ----------------------------------------------------------------------------------------------- data
# (M, K, N, seed, ln) -> draw number.  Under draw 0 of these shapes one planted defect was invisible to the gates in one of the
# cases that share the data -- the dropped term is ONE product of ONE output, and it fell on a product near zero or, under the GELU
# epilogue, on a pre-activation where gelu_new is flat (far negative, or at its minimum near -0.75).  The gates stay; the data of
# that shape is another draw of the same distributions (the first one at which every planted defect is visible in every case).
RESEED = {(17, 1536, 48, 0, 0): 1,      # n-edge K 1536, N 32, gelu: dropped term at rho 20.7 under a gate of 25.4
          (32, 1280, 90, 0, 0): 1}      # K class 1280, gelu without bias: dropped term at rho 18.9 under a gate of 23.7


class Data(dict):
    """name -> float32 array; ``key``: the (M, K, N, seed, ln) it was made for."""
    key = None


def make(M, K, N, seed=0, ln=False):
    """Seeded per shape.  x = randn (LayerNorm cases: 2 randn + 0.3), wT = 0.05 randn, bias = 0.1 randn, resid = randn,
    gain = 1 + 0.1 randn, shift = 0.1 randn; float32."""
    rng = np.random.default_rng([M, K, N, seed, int(ln), RESEED.get((M, K, N, seed, int(ln)), 0)])
    f = np.float32
    x = rng.standard_normal((M, K))
    d = Data({"x": (2.0 * x + 0.3 if ln else x).astype(f), "wT": (0.05 * rng.standard_normal((N, K))).astype(f),
              "bias": (0.1 * rng.standard_normal(N)).astype(f), "resid": rng.standard_normal((M, N)).astype(f)})
    d.key = (M, K, N, seed, int(ln))
    if ln:
        d["g"] = (1.0 + 0.1 * rng.standard_normal(K)).astype(f)
        d["beta"] = (0.1 * rng.standard_normal(K)).astype(f)
    return d


# ----------------------------------------------------------------------------------------------- float64
def gelu_new64(v):
    v = np.asarray(v, np.float64)
    return 0.5 * v * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))


def layernorm64(x, g, beta, eps):
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)          # two-pass
    return (x - mean) / np.sqrt(var + eps) * np.asarray(g, np.float64) + np.asarray(beta, np.float64)


def ref_pre(x, wT, bias, resid, epilogue, ln=None):
    """Float64 value in front of the GELU (for the other epilogues: the result)."""
    a = layernorm64(x, *ln) if ln is not None else np.asarray(x, np.float64)
    v = a @ np.asarray(wT, np.float64).T
    if bias is not None:
        v = v + np.asarray(bias, np.float64)
    if epilogue == "residual":
        v = v + np.asarray(resid, np.float64)
    return v


def ref(x, wT, bias, resid, epilogue, ln=None):
    v = ref_pre(x, wT, bias, resid, epilogue, ln)
    return gelu_new64(v) if epilogue == "gelu" else v


def denom(x, wT, bias, resid, epilogue, ln=None):
    """Per-element scale: without LayerNorm sum_k |x_k w_nk| + |bias_n| + |resid_mn|; with it (either form)
    rstd (sum_k |x_k g_k w_nk| + |mean| sum_k |g_k w_nk|) + sum_k |beta_k w_nk| + |bias_n| (+ |resid_mn|)."""
    x = np.asarray(x, np.float64)
    aw = np.abs(np.asarray(wT, np.float64))
    if ln is None:
        d = np.abs(x) @ aw.T
    else:
        g, beta, eps = np.asarray(ln[0], np.float64), np.asarray(ln[1], np.float64), ln[2]
        mean = x.mean(axis=1, keepdims=True)
        rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(axis=1, keepdims=True) + eps)
        d = rstd * (np.abs(x * g) @ aw.T + np.abs(mean) * (aw @ np.abs(g))[None, :]) + (aw @ np.abs(beta))[None, :]
    if bias is not None:
        d = d + np.abs(np.asarray(bias, np.float64))
    if epilogue == "residual":
        d = d + np.abs(np.asarray(resid, np.float64))
    return d


def rho(got, want, den, epilogue="none", pre=None):
    """max over elements of the error in units of 2^-24 denom (GELU: see the module docstring); inf if anything is not finite."""
    got = np.asarray(got, np.float64)
    if got.shape != want.shape or not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - want)
    if epilogue == "gelu":
        return float((np.maximum(err - GELU_ERR * np.abs(pre), 0.0) / (GELU_SLOPE * U * den)).max())
    return float((err / (U * den)).max())


# ----------------------------------------------------------------------------------------------- float32, k strictly in order
def seq32(x, wT, bias, resid, epilogue, ln=None):
    """The formula ``denom`` describes, in float32, every sum over k one chain in k order (LayerNorm: the folded form
    rstd (sum_k (x_k g_k) w_nk - mean sum_k g_k w_nk) + sum_k beta_k w_nk, statistics two-pass)."""
    f = np.float32
    x = np.asarray(x, f)
    w = np.ascontiguousarray(np.asarray(wT, f).T)                # [K, N]
    M, K = x.shape
    N = w.shape[1]
    a = x if ln is None else x * np.asarray(ln[0], f)[None, :]
    acc = np.zeros((M, N), f)
    for k in range(K):
        acc += a[:, k:k + 1] * w[k][None, :]
    if ln is not None:
        g, beta, eps = np.asarray(ln[0], f), np.asarray(ln[1], f), f(ln[2])
        s = np.zeros(M, f)
        for k in range(K):
            s += x[:, k]
        mean = s / f(K)
        q = np.zeros(M, f)
        for k in range(K):
            dx = x[:, k] - mean
            q += dx * dx
        rstd = f(1.0) / np.sqrt(q / f(K) + eps)
        c1, c2 = np.zeros(N, f), np.zeros(N, f)
        for k in range(K):
            c1 += g[k] * w[k]
            c2 += beta[k] * w[k]
        acc = rstd[:, None] * (acc - mean[:, None] * c1[None, :]) + c2[None, :]
    if bias is not None:
        acc = acc + np.asarray(bias, f)[None, :]
    if epilogue == "gelu":
        c = f(math.sqrt(2.0 / math.pi))
        acc = f(0.5) * acc * (f(1.0) + np.tanh(c * (acc + f(0.044715) * acc * acc * acc)))
    elif epilogue == "residual":
        acc = acc + np.asarray(resid, f)
    assert acc.dtype == f
    return acc


class Case:
    """One set of inputs with everything the gates need, computed once: float64 reference, scale, seq32's rho."""

    def __init__(self, x, wT, bias, resid, epilogue, ln=None, skinny16=True):
        self.args = (x, wT, bias, resid if epilogue == "residual" else None, epilogue, ln)
        self.M, self.K = x.shape
        self.N = wT.shape[0]
        self.epilogue = epilogue
        self.pre = ref_pre(*self.args)
        self.ref = gelu_new64(self.pre) if epilogue == "gelu" else self.pre
        self.den = denom(*self.args)
        self.hard = hard_gate(self.M, self.K, self.N, skinny16)
        pre_epi = "none" if epilogue == "gelu" else epilogue
        pre_args = self.args[:4] + (pre_epi, ln)
        self.rho_seq32 = rho(seq32(*pre_args), self.pre, self.den, pre_epi)
        self.measured = 8.0 * self.rho_seq32

    def rho(self, got):
        return rho(got, self.ref, self.den, self.epilogue, self.pre)

    def passes(self, got):
        r = self.rho(got)
        return r <= self.hard and r <= self.measured


# ----------------------------------------------------------------------------------------------- planted defects
def planted(kind, x, wT, bias, resid, epilogue, ln=None, prev=None):
    """The float64 reference with ONE defect, or None where the defect cannot occur at this shape.  ``prev``: what the output
    buffer held before (stale_column_tile); default: the reference of the same call on x rotated by one k."""
    M, K = x.shape
    N = wT.shape[0]
    if kind == "drop_k":                                         # ONE term of ONE output: the last row and column, mid-K
        k = K // 2 + 1
        a = layernorm64(x, *ln) if ln is not None else np.asarray(x, np.float64)
        v = ref_pre(x, wT, bias, resid, epilogue, ln)
        v[M - 1, N - 1] -= a[M - 1, k] * float(wT[N - 1, k])
        return gelu_new64(v) if epilogue == "gelu" else v
    if kind == "swap_rows_15_16":
        if M < 17:
            return None
        v = ref(x, wT, bias, resid, epilogue, ln)
        v[[15, 16]] = v[[16, 15]]
        return v
    if kind == "bias_missing_on_ragged_tile":
        if bias is None or N % 16 == 0:
            return None
        b = np.array(bias, np.float64)
        b[N - N % 16:] = 0.0
        return ref(x, wT, b, resid, epilogue, ln)
    if kind == "residual_from_row_above":
        if epilogue != "residual" or M < 2:
            return None
        r = np.array(resid, np.float64)
        r[1:] = r[:-1].copy()
        return ref(x, wT, bias, r, epilogue, ln)
    if kind == "stale_column_tile":
        if prev is None:
            prev = ref(np.roll(x, 1, axis=1), wT, bias, resid, epilogue, ln)
        v = ref(x, wT, bias, resid, epilogue, ln)
        t = cdiv(N, 16) // 2
        v[:, 16 * t:16 * t + 16] = np.asarray(prev, np.float64)[:, 16 * t:16 * t + 16]
        return v
    raise ValueError(kind)


# ----------------------------------------------------------------------------------------------- the shapes of the GPU tests
K_CLASSES = (256, 1280, 512, 768, 1024, 1536, 4096)                  # M 32, N 90, every epilogue, with and without bias
M_EDGES, M_EDGE_KS, M_EDGE_N = (1, 2, 15, 16, 17, 31, 32), (256, 768, 1024), 33
N_EDGES, N_EDGE_KS, N_EDGE_M, N_EDGE_FULL = (1, 15, 16, 17, 31, 32, 33), (256, 512, 1536), 17, 48
BOUNDARY = ((1024, 5, 4096), (1024, 5, 4112), (512, 5, 4112))        # (K, M, N)
INPLACE = ((768, 17, 90), (1024, 17, 90))
TICKET_SHAPES = ((1024, 5, 4096), (1536, 17, 48), (1024, 17, 33))
LN_KS, LN_MS, LN_NS, LN_EPILOGUES = (512, 768), (1, 17, 32), (33, 90), ("none", "gelu")
FOLD_NS, FOLD_KS = (1, 3, 4, 5), (100, 512, 768)
S8_KS, S8_MS, S8_NS, S8_SPLITK = (512, 768), (1, 17, 32), (31, 33, 90), (1024, 17, 33)


def ln_of(d):
    return (d["g"], d["beta"], LN_EPS)


def gate_cases():
    """Every (label, Case arguments, skinny16) of section 4 that goes through the gates: what test_host_skinny_gemm.py walks."""
    out = []

    def add(label, d, M, N, epilogue, bias=True, ln=False, skinny16=True):
        out.append((label, (d["x"][:M], d["wT"][:N], d["bias"][:N] if bias else None, np.ascontiguousarray(d["resid"][:M, :N]), epilogue,
                            ln_of(d) if ln else None), skinny16, d.key))

    for K in K_CLASSES:
        d = make(32, K, 90)
        for e in EPILOGUES:
            for bias in (True, False):
                add(f"kclass K{K} {e} bias{int(bias)}", d, 32, 90, e, bias)
    for K in M_EDGE_KS:
        d = make(32, K, M_EDGE_N)
        for M in M_EDGES:
            add(f"m-edge K{K} M{M}", d, M, M_EDGE_N, "residual")
    for K in N_EDGE_KS:
        d = make(N_EDGE_M, K, N_EDGE_FULL)
        for N in N_EDGES + (N_EDGE_FULL,):
            add(f"n-edge K{K} N{N}", d, N_EDGE_M, N, "gelu")
    for K, M, N in BOUNDARY:
        add(f"boundary K{K} N{N}", make(M, K, N), M, N, "residual")
    for K, M, N in INPLACE:
        add(f"in-place K{K}", make(M, K, N), M, N, "residual")
    for K, M, N in TICKET_SHAPES:
        for v in (0, 1):
            add(f"ticket K{K} N{N} x{v}", make(M, K, N, seed=v), M, N, "residual")
    for K in LN_KS:
        for N in LN_NS:
            d = make(32, K, N, ln=True)
            for M in LN_MS:
                for e in LN_EPILOGUES:
                    add(f"layernorm K{K} M{M} N{N} {e}", d, M, N, e, ln=True)
    for K in S8_KS:
        for N in S8_NS:
            d, dl = make(32, K, N, seed=8), make(32, K, N, seed=8, ln=True)
            for M in S8_MS:
                for e in EPILOGUES:
                    add(f"skinny8 K{K} M{M} N{N} {e}", d, M, N, e, skinny16=False)
                add(f"skinny8 K{K} M{M} N{N} layernorm", dl, M, N, "gelu", ln=True, skinny16=False)
    K, M, N = S8_SPLITK
    add(f"skinny8 split-K K{K} N{N}", make(M, K, N, seed=8), M, N, "residual", skinny16=False)
    return out


# ----------------------------------------------------------------------------------------------- r4d_fold_layernorm_f32 alone
def fold_ref(wT, g, beta):
    """(wTg as fp32 bits = fl32(g_k w_nk), lnc float64 [2,N], its scales [2,N] = sum |g w|, sum |beta w|)."""
    wTg = np.asarray(g, np.float32)[None, :] * np.asarray(wT, np.float32)
    w64, g64, b64 = np.asarray(wT, np.float64), np.asarray(g, np.float64), np.asarray(beta, np.float64)
    lnc = np.stack([w64 @ g64, w64 @ b64])
    den = np.stack([np.abs(w64) @ np.abs(g64), np.abs(w64) @ np.abs(b64)])
    return wTg, lnc, den


def fold_gate(K):
    return K / 64.0 + 6 + 16
