// What the MFMA GEMM files share: vector types, gelu_new, the XCD-aware grouped tile order, and on the host side the
// 128 x 256 / 128 x 128 tile rule and the runtime-epilogue -> template-instantiation dispatch.  The device helpers are
// __forceinline__ FUNCTIONS: measured on the 256-VGPR kernels of gemm_h2.hip, that leaves the assembly as it was (DESIGN_LOG
// 12.15).  The row-major epilogue is shared as TEXT instead (gemm_epilogue_rowmajor.h) -- as a function it changes the register
// allocation of the whole kernel.
#pragma once
#include "common.h"
#include "h2.h"

namespace r4d {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// the plain-bf16 rounding (bf16x3.h builds its split on it; the row-major epilogue's bf16 output uses it)
__device__ __forceinline__ unsigned cvt_pk_bf16(float a, float b) {   // v_cvt_pk_bf16_f32: low half = bf16(a), RNE
    const f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

__device__ __forceinline__ float gelu_new1(float x) {
    // gelu_new(x) = 0.5x(1+tanh(u)), u = sqrt(2/pi)(x+0.044715x^3)  -- modeling_gpt2.py:25,206.
    // Algebraically 0.5(1+tanh(u)) = 1/(1+exp(-2u)) = 1/(1+exp2(x*(k0 + k1*x^2))) with k0 = -2 sqrt(2/pi) log2(e),
    // k1 = 0.044715 k0: mul, fma, mul, v_exp_f32, add, v_rcp_f32, mul -- every epilogue VALU instruction is taken from
    // the MFMA issue slots of the co-resident workgroup, the ocml tanhf form (~40) cost 15 % of a c_fc tile.
    // |error| < 3e-7 |x| (checked against the oracle at 1e-5 relative in tests/test_gpu_ops.py).
    const float k0 = -2.0f * 0.7978845608028654f * 1.4426950408889634f, k1 = 0.044715f * k0;
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * __builtin_fmaf(x * x, k1, k0)));
}

// two outputs at a time: the polynomial part as packed fp32 (v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32 on gfx950),
// only exp2 and rcp stay scalar -- 4.5 instead of 7 instructions per element
template <typename V2>
__device__ __forceinline__ V2 gelu_new2(V2 x) {
    const float k0 = -2.0f * 0.7978845608028654f * 1.4426950408889634f, k1 = 0.044715f * k0;
    const V2 a = x * x * k1 + k0;
    const V2 w = x * a;
    V2 e;
    e.x = __builtin_amdgcn_exp2f(w.x); e.y = __builtin_amdgcn_exp2f(w.y);
    e = e + 1.0f;
    V2 r;
    r.x = __builtin_amdgcn_rcpf(e.x); r.y = __builtin_amdgcn_rcpf(e.y);
    return x * r;
}

// d gelu_new / dx with the exponential of gelu_new1: tanh(u) = 1 - 2 / (1 + e^(2u))
__device__ __forceinline__ float gelu_new_grad(float x) {
    const float c = 0.7978845608028654f;
    const float x2 = x * x;
    const float u2 = 2.0f * c * 1.4426950408889634f * x * __builtin_fmaf(x2, 0.044715f, 1.0f);     // 2u log2(e)
    const float t = 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(u2));
    return 0.5f * (1.0f + t) + 0.5f * x * (1.0f - t * t) * c * __builtin_fmaf(x2, 3.0f * 0.044715f, 1.0f);
}

// XCD-aware grouped tile order, in two steps (grouped_tile below puts them together).
//
// Step 1, xcd_contiguous: workgroups are dealt round-robin over the 8 XCDs (v % 8 = XCD group), each with its own 4 MB L2.
// Remap so that an XCD walks a CONTIGUOUS range of tile positions: the workgroups that share one A row-panel then hit the same
// L2 instead of fetching it 8 times.  Bijective for any grid.  Returns the position of workgroup v of nblk in that order.
// (I: blockIdx.x is unsigned, the persistent kernel's virtual index an int -- each keeps its own shift.)
template <typename I>
__device__ __forceinline__ int xcd_contiguous(I v, int nblk) {
    const int xq = nblk >> 3, xr = nblk & 7, xcd = v & 7;
    return xcd * xq + min(xcd, xr) + (v >> 3);
}

// Step 2, grouped_origin: origin (m0, n0) of the BM x BN tile at position `bid`.  Inside an XCD's range the tiles are walked in
// groups of GROUP_M row-panels (m fastest inside a group, n across it): the ~64 tiles resident on an XCD then span ~8 row-panels
// x ~8 column-panels, i.e. ~2 MB of A + ~2 MB of B in its 4 MB L2, instead of 4 row-panels x every column-panel of B.
template <int BM, int BN>
__device__ __forceinline__ void grouped_origin(int bid, int tiles_m, int tiles_n, int& m0, int& n0) {
    constexpr int GROUP_M = 8;
    const int per_group = GROUP_M * tiles_n;
    const int grp = bid / per_group, first_m = grp * GROUP_M;
    const int gsz = min(tiles_m - first_m, GROUP_M);
    const int tile_m = first_m + (bid % per_group) % gsz, tile_n = (bid % per_group) / gsz;
    m0 = tile_m * BM;
    n0 = tile_n * BN;
}
// one tile per workgroup of a 1-D grid
template <int BM, int BN>
__device__ __forceinline__ void grouped_tile(int M, int N, int& m0, int& n0) {
    const int bid = xcd_contiguous(blockIdx.x, (int)gridDim.x);
    grouped_origin<BM, BN>(bid, (M + BM - 1) / BM, (N + BN - 1) / BN, m0, n0);
}
// explicit block index and count, tile counts computed by the caller: the persistent bf16x3 kernel walks a VIRTUAL index
template <int BM, int BN>
__device__ __forceinline__ void grouped_tile(int tiles_m, int tiles_n, int v, int nblk, int& m0, int& n0) {
    grouped_origin<BM, BN>(xcd_contiguous(v, nblk), tiles_m, tiles_n, m0, n0);
}

// ------------------------------------------------------------------ host side
// 128 x 256 (0) or 128 x 128 (1): fewest tile waves over the 256 CUs, the narrow tile at 0.9 of the wide one's efficiency, so
// the wide tile wins ties (a row's result never depends on the tile either way)
static inline int pick_tile_128(int M, int N) {
    const long long b0 = (long long)cdiv(M, 128) * cdiv(N, 256), b1 = (long long)cdiv(M, 128) * cdiv(N, 128);
    const double c0 = (double)((b0 + 255) / 256) * 128 * 256, c1 = (double)((b1 + 255) / 256) * 128 * 128 / 0.9;
    return c1 < c0 ? 1 : 0;
}

// Runtime epilogue -> template instantiation.  KINDS is the list of kinds a family instantiates, as an X-macro
// `#define FAMILY_KINDS(X, L) X(L, EPI_NONE) X(L, EPI_GELU) ...`; LAUNCH(E) is run with E the constant that equals EPILOGUE, the
// trailing statements when none does.
#define R4D_EPI_CASE_(LAUNCH, E) case E: LAUNCH(E); break;
#define R4D_EPI_DISPATCH(EPILOGUE, KINDS, LAUNCH, ...) \
    switch (EPILOGUE) { KINDS(R4D_EPI_CASE_, LAUNCH) default: __VA_ARGS__ }

}  // namespace r4d
