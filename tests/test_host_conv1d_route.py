"""CPU-side checks of the Conv1D routing query (``r4d_conv1d_route``, csrc/conv1d_route.h; the GPU side is
tests/test_gpu_conv1d_route.py): the precedence of DESIGN.md "Conv1D routing" restated in Python against the library over a
grid, a table of rows pinned by hand from the dispatchers as they stood BEFORE the routes existed, and the route names."""
import itertools
import os

import pytest

from conftest import REPO

WT, W3, W3T, H2, SK = 1, 2, 4, 8, 16            # the `have` bits
NONE, GELU, RESIDUAL, GELU_KEEP, GELU_GRAD, H2WORDS = 0, 1, 2, 5, 6, 7
NAMES = ("skinny", "h2", "s3", "b1", "f32_kcopy", "f32_ref", "dgrad_b1", "dgrad_s3", "dgrad_f32", "wgrad_b1tn", "wgrad_s3tn",
         "wgrad_f32tn")


@pytest.fixture(scope="module")
def lib():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    was = lib.r4d_get_gemm_split3()
    yield lib
    lib.r4d_set_gemm_split3(was)


# ---- the DESIGN.md table, one `if` per row
def _planes(M, K, N, bytes_per_weight):        # gemm_s3 (6) / gemm_h2 (4) / gemm_b1 (2): K % 32, 32-bit offsets
    return M >= 1 and K >= 32 and K % 32 == 0 and N >= 1 and N * K * bytes_per_weight < 2 ** 31 and M * K < 2 ** 29 and 128 * N < 2 ** 29


def _cdiv(a, b):
    return -(-a // b)


def expected(kind, mode, bf16, have, epi, M, K, N):
    wT, w3, w3t, h2, sk = (bool(have & b) for b in (WT, W3, W3T, H2, SK))
    if kind in (0, 1, 2):
        if kind == 1:                            # the cached decode step carries no planes and no bf16 switch
            w3 = h2 = bf16 = False
        if bf16 and (kind == 2 or epi <= RESIDUAL) and w3 and _planes(M, K, N, 2):
            return "b1"
        if kind == 1 and sk and wT and 1 <= M <= 32 and K >= 256 and K % 256 == 0 and N >= 1:
            return "skinny"
        if h2 and mode == 2 and epi in (NONE, GELU, RESIDUAL, GELU_KEEP, H2WORDS) and _planes(M, K, N, 4):
            return "h2"
        if w3 and mode and _planes(M, K, N, 6):
            return "s3"
        return "f32_kcopy" if wT else "f32_ref"
    if kind in (3, 4):                           # dx[M, K] = dy[M, N] . W^T: N is contracted
        if kind == 3 and bf16 and w3t and _planes(M, N, K, 2):
            return "dgrad_b1"
        if w3t and mode and _planes(M, N, K, 6):
            return "dgrad_s3"
        return "dgrad_f32"
    tiles = (K % 128 == 0 and N % 256 == 0 and M >= 32 and K % 4 == 0 and N % 4 == 0 and M * K < 2 ** 29 and M * N < 2 ** 29)
    if bf16 and tiles and K >= 128 and N >= 256 and (M + 64) * K < 2 ** 29 and (M + 64) * N < 2 ** 29:
        return "wgrad_b1tn"
    splits = max(1, min(_cdiv(1024, _cdiv(K, 128) * _cdiv(N, 128)), _cdiv(M, 256), 64))
    if mode and splits > 1 and tiles:
        return "wgrad_s3tn"
    return "wgrad_f32tn"


def test_the_table_restated_in_python_agrees_over_the_grid(lib):
    route, name = lib.r4d_conv1d_route, lib.r4d_conv1d_route_name
    names = [name(i).decode() for i in range(len(NAMES))]
    Ms, Ks, Ns, rows = (1, 32, 33, 4096), (48, 64, 256, 512), (64, 128, 192, 256, 1536), (31, 32, 390, 4100)
    n = 0
    for mode in (0, 1, 2):
        lib.r4d_set_gemm_split3(mode)
        assert lib.r4d_get_gemm_split3() == mode
        for kind in range(6):
            for bf16, have, epi, M, K, N in itertools.product((0, 1), range(32), range(8), Ms + rows if kind == 5 else Ms, Ks, Ns):
                got = route(kind, M, K, N, epi, have, bf16)
                want = expected(kind, mode, bf16, have, epi, M, K, N)
                assert 0 <= got < len(names) and names[got] == want, (kind, mode, bf16, have, epi, M, K, N, got, want)
                n += 1
    assert n == 3 * 2 * 32 * 8 * 4 * 5 * (5 * 4 + 8)


# (kind, mode, bf16, have, epilogue, M, K, N) -> route.  Derived by hand from the dispatchers of the commit BEFORE the routes
# ("parent": 6ca93d3), file and line per group; never from r4d_conv1d_route.
PINNED = [
    # parent csrc/encoder.hip:22-56 (conv1d) behind :60-70 (conv1d_encode, encode bf16 off): f16x2 under its epilogue whitelist
    # (:30) > bf16x3 (:39) > [N,K] copy (:51) > reference layout (:52); conv1d_encode hands no skinny scratch down (:69)
    ((0, 1, 0, WT | W3, NONE, 4096, 256, 768), "s3"),
    ((0, 2, 0, WT | W3 | W3T | H2, NONE, 4096, 256, 768), "h2"),
    ((0, 2, 0, WT | W3 | W3T | H2, GELU_GRAD, 4096, 256, 768), "s3"),         # :30: GELU_GRAD is not in the f16x2 whitelist
    ((0, 2, 0, WT | W3 | W3T | H2, H2WORDS, 32, 256, 768), "h2"),
    ((0, 2, 0, WT | W3, NONE, 4096, 256, 768), "s3"),                          # mode 2 without f16 planes: bf16x3
    ((0, 0, 0, WT | W3 | W3T | H2, NONE, 4096, 256, 768), "f32_kcopy"),
    ((0, 0, 0, W3 | W3T | H2, NONE, 4096, 256, 768), "f32_ref"),
    ((0, 1, 0, WT | W3 | W3T | H2, NONE, 4096, 48, 64), "f32_kcopy"),          # K = 48: no planes kernel (K % 32)
    ((0, 2, 0, WT | W3 | W3T | H2, NONE, 4096, 48, 64), "f32_kcopy"),
    ((0, 2, 0, H2, GELU_GRAD, 33, 256, 256), "f32_ref"),
    ((0, 1, 0, WT | SK, NONE, 1, 256, 768), "f32_kcopy"),                      # an encoder call is never skinny
    # parent csrc/encoder.hip:62 (conv1d_encode, encode bf16 on): plane 0 of w3, epilogue <= EPI_RESIDUAL, whatever the mode
    ((0, 1, 1, WT | W3, RESIDUAL, 4096, 256, 256), "b1"),
    ((0, 0, 1, WT | W3, GELU, 33, 256, 1024), "b1"),
    ((0, 1, 1, WT | W3, GELU_KEEP, 4096, 256, 1024), "s3"),                    # the encoder's epilogue limit
    ((0, 2, 1, WT | W3 | W3T | H2, H2WORDS, 32, 256, 768), "h2"),
    ((0, 1, 1, WT, NONE, 4096, 256, 768), "f32_kcopy"),
    ((0, 1, 1, WT | W3, NONE, 32, 48, 64), "f32_kcopy"),
    # parent csrc/encoder.hip:25 (skinny first) and :468,:492-508 (the decode step passes its scratch for B <= 32 and NO planes)
    ((1, 1, 0, WT | SK, NONE, 32, 512, 1536), "skinny"),
    ((1, 1, 0, WT | SK, RESIDUAL, 33, 512, 512), "f32_kcopy"),                 # M = 33 against skinny
    ((1, 1, 0, WT | W3 | W3T | H2 | SK, NONE, 33, 512, 1536), "f32_kcopy"),
    ((1, 2, 0, WT | W3 | W3T | H2, GELU, 33, 512, 1536), "f32_kcopy"),
    ((1, 1, 0, SK, NONE, 1, 512, 1536), "f32_ref"),
    ((1, 2, 0, WT | SK, NONE, 1, 64, 192), "f32_kcopy"),                       # K % 256
    ((1, 1, 0, WT, NONE, 32, 512, 512), "f32_kcopy"),
    ((1, 1, 1, WT | W3 | SK, NONE, 32, 512, 1536), "skinny"),
    # parent csrc/train.hip:164-176 (fwd_linear): plain bf16 first with ANY epilogue, then conv1d without a skinny scratch
    ((2, 1, 1, WT | W3, GELU_KEEP, 4096, 256, 1024), "b1"),
    ((2, 2, 1, WT | W3 | W3T | H2, NONE, 32, 256, 768), "b1"),
    ((2, 2, 0, WT | W3 | W3T | H2, GELU_KEEP, 4096, 256, 1024), "h2"),
    ((2, 1, 0, WT | W3 | W3T | H2, GELU_KEEP, 4096, 256, 1024), "s3"),
    ((2, 0, 0, WT | W3 | W3T | H2, NONE, 33, 256, 768), "f32_kcopy"),
    ((2, 1, 1, WT | H2, NONE, 4096, 256, 768), "f32_kcopy"),
    ((2, 2, 1, WT | H2, NONE, 4096, 256, 768), "h2"),
    ((2, 1, 1, WT | W3, NONE, 4096, 48, 64), "f32_kcopy"),
    # parent csrc/train.hip:188-218 (data_grad_gemm; :189 b1 for b_trans == 1 only, :202 bf16x3 in every split mode) and
    # csrc/lm_head.hip:411 (the head: b_trans = 0, no bf16 argument)
    ((3, 1, 1, W3T, NONE, 4096, 256, 1024), "dgrad_b1"),
    ((3, 0, 1, W3T, NONE, 4096, 256, 1024), "dgrad_b1"),
    ((3, 1, 0, W3T, NONE, 4096, 256, 1024), "dgrad_s3"),
    ((3, 2, 0, W3T | H2, NONE, 4096, 256, 1024), "dgrad_s3"),
    ((3, 0, 0, W3T, NONE, 4096, 256, 1024), "dgrad_f32"),
    ((3, 1, 1, WT | W3, NONE, 4096, 256, 1024), "dgrad_f32"),
    ((3, 1, 1, W3T, NONE, 32, 64, 48), "dgrad_f32"),                           # the contraction runs over N = 48
    ((4, 1, 1, W3T, NONE, 32, 256, 1536), "dgrad_s3"),                         # b_trans == 0 never takes b1
    ((4, 0, 1, W3T, NONE, 32, 256, 1536), "dgrad_f32"),
    # parent csrc/train.hip:228-244 (bwd_weight), csrc/gemm_b1tn.hip:208-211 (I >= 128, I % 128, J >= 256, J % 256, M >= 32),
    # csrc/gemm_f32.hip:366-373 (tn_splits) and :390 (s3tn under the split mode, S > 1 and its contract)
    ((5, 1, 1, 0, NONE, 390, 128, 512), "wgrad_b1tn"),
    ((5, 0, 1, 0, NONE, 390, 128, 512), "wgrad_b1tn"),
    ((5, 1, 1, 0, NONE, 32, 128, 512), "wgrad_b1tn"),
    ((5, 1, 1, 0, NONE, 390, 128, 384), "wgrad_f32tn"),                        # 384 columns: no whole 256-wide tiles -> fallback
    ((5, 1, 1, 0, NONE, 31, 128, 512), "wgrad_f32tn"),
    ((5, 1, 1, 0, NONE, 390, 64, 256), "wgrad_f32tn"),
    ((5, 1, 0, 0, NONE, 390, 128, 512), "wgrad_s3tn"),                         # S = min(256, ceil(390 / 256)) = 2
    ((5, 1, 0, 0, NONE, 32, 128, 512), "wgrad_f32tn"),                         # S == 1: stays on f32tn in the split mode
    ((5, 2, 0, 0, NONE, 4100, 256, 256), "wgrad_s3tn"),
    ((5, 0, 0, 0, NONE, 390, 128, 512), "wgrad_f32tn"),
]


def test_rows_pinned_from_the_dispatchers_before_the_routes(lib):
    assert len(PINNED) >= 40
    for (kind, mode, bf16, have, epi, M, K, N), want in PINNED:
        lib.r4d_set_gemm_split3(mode)
        got = lib.r4d_conv1d_route_name(lib.r4d_conv1d_route(kind, M, K, N, epi, have, bf16)).decode()
        assert got == want, ((kind, mode, bf16, have, epi, M, K, N), got, want)
        assert expected(kind, mode, bf16, have, epi, M, K, N) == want


def test_route_names_are_enumerable(lib):
    assert tuple(lib.r4d_conv1d_route_name(i).decode() for i in range(len(NAMES))) == NAMES
    for bad in (-1, len(NAMES), 99):
        assert lib.r4d_conv1d_route_name(bad) == b"unknown"
    assert lib.r4d_conv1d_route(6, 32, 256, 256, 0, 0, 0) == -1 and lib.r4d_conv1d_route(-1, 32, 256, 256, 0, 0, 0) == -1
    hdr = open(os.path.join(REPO, "include", "r4d.h")).read()
    from rag4dyg_amd import _lib
    assert lib.r4d_abi_version() == 6
    for s in ("r4d_conv1d_route", "r4d_conv1d_route_name"):
        assert s in _lib.PROTOTYPES and s + "(" in hdr


def test_an_empty_or_negative_shape_is_refused_not_divided_by(lib):
    """-1 for M, K or N <= 0 in every kind, mode and precision (kind 5 in a split mode once divided 1024 by zero tiles)."""
    for mode in (0, 1, 2):
        lib.r4d_set_gemm_split3(mode)
        for kind, bf16, bad in itertools.product(range(6), (0, 1), (0, -1, -128, -2 ** 31)):
            for M, K, N in ((bad, 128, 256), (390, bad, 256), (390, 128, bad), (bad, bad, bad)):
                assert lib.r4d_conv1d_route(kind, M, K, N, 0, 31, bf16) == -1, (mode, kind, bf16, M, K, N)
    assert lib.r4d_conv1d_route(5, 390, 128, 256, 0, 0, 0) >= 0
