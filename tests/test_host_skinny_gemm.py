"""CPU-side checks for the single-op entry of the decode step's weight-stream GEMM (``r4d_conv1d_skinny_f32``; the GPU side is
tests/test_gpu_skinny_gemm.py): the symbols, the workspace query, every refusal before any launch, and the two things that make
the GPU file's gates mean something -- the float32 in-order reference stays inside them at every shape the GPU file runs, and
every planted defect of tests/_skinny_ref.py breaks them at every shape it applies to.

What the wrapper refuses beyond the dispatcher: a folded LayerNorm together with ``ln_w`` / ``ln_b`` (two LayerNorms for one
product); it ACCEPTS a folded LayerNorm with a residual (the kernel's fused epilogue serves it)."""
import ctypes
import os

import numpy as np
import pytest

import _skinny_ref as R
from conftest import REPO

R4D_ERR_INVALID, R4D_ERR_WORKSPACE = -1, -3
SYMBOLS = ("r4d_conv1d_skinny_workspace_bytes", "r4d_conv1d_skinny_f32")


@pytest.fixture(scope="module")
def lib():
    from rag4dyg_amd import _lib
    return _lib.load()


def test_error_codes_are_the_headers():
    hdr = open(os.path.join(REPO, "include", "r4d.h")).read()
    assert f"#define R4D_ERR_INVALID ({R4D_ERR_INVALID})" in hdr and f"#define R4D_ERR_WORKSPACE ({R4D_ERR_WORKSPACE})" in hdr


def test_symbols_in_header_binding_and_library(lib):
    from rag4dyg_amd import _lib, ops
    assert lib.r4d_abi_version() == 6 and _lib.R4D_ABI_VERSION == 6          # additive
    hdr = open(os.path.join(REPO, "include", "r4d.h")).read()
    for s in SYMBOLS:
        assert s in _lib.PROTOTYPES and hasattr(lib, s) and s + "(" in hdr, s
    assert callable(ops.conv1d_skinny) and callable(ops.conv1d_skinny_workspace)


@pytest.mark.parametrize("K,N", [(256, 1), (256, 33), (512, 4112), (768, 90), (1024, 4096), (1280, 90), (1536, 48), (4096, 90)])
def test_workspace_query(lib, K, N):
    from rag4dyg_amd import ops
    want = 4 * (-(-K // 256) * 32 * N + 256)
    assert lib.r4d_conv1d_skinny_workspace_bytes(K, N) == want == R.workspace_bytes(K, N) == ops.conv1d_skinny_workspace(K, N)


def test_workspace_query_of_an_unsupported_shape_is_zero(lib):
    for K, N in ((128, 8), (255, 8), (384, 8), (0, 8), (256, 0)):
        assert lib.r4d_conv1d_skinny_workspace_bytes(K, N) == 0, (K, N)


# Pointers that are never dereferenced: every refusal comes before any launch, so on a machine without a GPU these calls return
# their code and nothing else happens (a call that got as far as a launch would fail with R4D_ERR_HIP instead).
X, W, Y, WS, B, RES, G, S, F = (0x10000 * i for i in range(1, 10))


def call(lib, M=4, K=512, N=48, epi=0, x=X, w=W, bias=B, res=None, g=None, s=None, fold=None, y=Y, ws=WS, ws_bytes=None, zeroed=0):
    if ws_bytes is None:
        ws_bytes = R.workspace_bytes(K, N)
    rc = lib.r4d_conv1d_skinny_f32(x, w, bias, res, M, K, N, epi, g, s, ctypes.c_float(1e-5), fold, zeroed, y, ws, ws_bytes, None)
    return rc, lib.r4d_last_error().decode()


REFUSALS = {
    "M = 0": dict(M=0), "M = 33": dict(M=33), "K = 128": dict(K=128), "K = 384": dict(K=384), "K = 255": dict(K=255),
    "N = 0": dict(N=0),
    "null workspace": dict(ws=None), "null x": dict(x=None), "null wT": dict(w=None), "null y": dict(y=None),
    "misaligned x": dict(x=X + 4), "misaligned wT": dict(w=W + 8),
    "LayerNorm at K = 256": dict(K=256, g=G, s=S), "LayerNorm at K = 1024": dict(K=1024, g=G, s=S),
    "LayerNorm at K = 1536": dict(K=1536, g=G, s=S), "folded LayerNorm at K = 1024": dict(K=1024, fold=F),
    "folded LayerNorm at K = 256": dict(K=256, fold=F),
    "ln_w without ln_b": dict(g=G), "ln_b without ln_w": dict(s=S), "misaligned ln_w": dict(g=G + 4, s=S),
    "folded LayerNorm with ln_w": dict(fold=F, g=G, s=S),
    "epilogue 3": dict(epi=3), "residual epilogue without a residual": dict(epi=2), "residual without its epilogue": dict(res=RES),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_before_any_launch(lib, what):
    rc, msg = call(lib, **REFUSALS[what])
    assert rc == R4D_ERR_INVALID, (what, rc, msg)
    assert "conv1d_skinny" in msg and len(msg) > len("conv1d_skinny: "), (what, msg)


def test_short_workspace_is_its_own_code(lib):
    rc, msg = call(lib, ws_bytes=R.workspace_bytes(512, 48) - 1)
    assert rc == R4D_ERR_WORKSPACE and "workspace too small" in msg, (rc, msg)
    rc, msg = call(lib, M=33, ws_bytes=0)                       # an unsupported shape is named first
    assert rc == R4D_ERR_INVALID, (rc, msg)


# ------------------------------------------------------------------------------------------------ the gates
CASES = R.gate_cases()


def test_the_case_list_is_section_4():
    labels = [c[0] for c in CASES]
    assert len(set(labels)) == len(labels)
    assert sum(l.startswith("kclass") for l in labels) == 7 * 3 * 2
    assert sum(l.startswith("m-edge") for l in labels) == 21 and sum(l.startswith("n-edge") for l in labels) == 24
    assert sum(l.startswith("layernorm") for l in labels) == 24
    assert sum(l.startswith("skinny8") for l in labels) == 2 * 3 * 3 * 4 + 1


def test_dispatcher_model_matches_the_issue():
    assert R.form(256, 90) == ("plain", 0, 1) and R.form(1280, 90) == ("plain", 0, 5)
    assert R.form(512, 90) == ("skinny16", 2, 1) and R.form(768, 90) == ("skinny16", 3, 1)
    assert R.form(1024, 90) == ("skinny16", 2, 2) and R.form(1536, 90) == ("skinny16", 3, 2) and R.form(4096, 90) == ("skinny16", 2, 8)
    assert R.form(1024, 4096) == ("skinny16", 2, 2) and R.form(1024, 4112) == ("skinny8", 2, 2) and R.form(512, 4112) == ("skinny16", 2, 1)
    assert R.form(512, 33, False) == ("skinny8", 2, 1) and R.form(768, 33, False) == ("skinny8", 3, 1) and R.form(1024, 33, False) == ("skinny8", 2, 2)
    assert R.chain_depth(32, 256, 90) == 256 + 8 + 1 + 3 and R.chain_depth(32, 1280, 90) == 256 + 8 + 5 + 3
    assert R.chain_depth(32, 768, 90) == 96 + 8 + 1 + 3 and R.chain_depth(32, 4096, 90) == 64 + 8 + 8 + 3


@pytest.fixture(scope="module")
def built():
    """label -> Case, each built once (float64 reference, scale, seq32) and left unchanged."""
    return {label: (R.Case(*args, skinny16=sk), args) for label, args, sk, _key in CASES}


def test_seq32_stays_inside_both_gates(built):
    worst = 0.0
    for label, (c, args) in built.items():
        r_pre = c.rho_seq32
        r_full = c.rho(R.seq32(*args))                          # with its own float32 GELU, under the GELU budget
        print(f"[seq32] {label}: rho {r_pre:.2f} (with the epilogue {r_full:.2f}), hard gate {c.hard}, measured gate {c.measured:.1f}")
        assert 0.0 < r_pre <= c.hard, label
        assert r_full <= c.hard and r_full <= c.measured, label
        assert c.measured <= c.hard, label                      # the measured gate is the tighter one at every shape
        worst = max(worst, r_pre)
    assert worst < 8.0                                          # "2 to 4 at these shapes", with room for the 4112-column maximum


@pytest.mark.parametrize("kind", R.DEFECTS)
def test_every_planted_defect_breaks_the_gate(built, kind):
    applied = 0
    lows = []
    for label, (c, args) in built.items():
        bad = R.planted(kind, *args)
        if bad is None:
            continue
        applied += 1
        r = c.rho(bad)
        lows.append(r)
        # a result passes only inside BOTH gates, and the measured one is the tighter at every shape (asserted above)
        assert r > c.measured and not c.passes(bad), (kind, label, r, c.measured)
        assert c.passes(c.ref)
    print(f"[planted] {kind}: {applied} shapes, rho min {min(lows):.3g} median {float(np.median(lows)):.3g}")
    assert applied >= {"drop_k": len(built), "stale_column_tile": len(built), "swap_rows_15_16": 40,
                       "bias_missing_on_ragged_tile": 60, "residual_from_row_above": 30}[kind], applied


def test_fold_reference_is_exact_and_its_gate_is_derived():
    rng = np.random.default_rng(5)
    w, g, b = (rng.standard_normal(s).astype(np.float32) for s in ((3, 100), 100, 100))
    wTg, lnc, den = R.fold_ref(w, g, b)
    assert wTg.dtype == np.float32 and np.array_equal(wTg, (g.astype(np.float64) * w.astype(np.float64)).astype(np.float32))
    assert lnc.shape == den.shape == (2, 3) and (den >= np.abs(lnc)).all()
    assert R.fold_gate(768) == 768 / 64 + 6 + 16
