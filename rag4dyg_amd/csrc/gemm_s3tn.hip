// Weight gradients on the bf16 matrix cores at fp32 accuracy: C[I,J] = sum over the token rows m of X[m,I]^T . dY[m,J]
// (Conv1D under autograd, modeling_utils.py:1267-1271: dW = x^T . dy) -- the "TN" form of gemm_s3.hip: BOTH operands are
// activations, row-major over the CONTRACTED index, so
//   * both tiles (32 tokens x 128 features of X, 32 tokens x 256 features of dY) are split on the fly into three bf16 terms
//     (gemm_s3.hip: x = hi + mid + lo exactly; six partial products per fp32 product) while they are staged;
//   * their LDS images stay token-major -- exactly what the coalesced global rows deliver -- and the k-contiguous MFMA
//     fragments come out of `ds_read_b64_tr_b16`, gfx950's transposing LDS read (per 16 lanes: a 4-token x 16-feature block
//     delivered feature-major: lane i gets feature i of the four tokens), two reads per 8-token fragment.  The 16-byte chunk
//     index of a row is XOR-ed with (token & 3) << 2, which spreads the four token rows of a read over all 64 banks
//     (unswizzled, 256-byte and 512-byte rows put them on the same 16: 4-way conflicts);
//   * the contraction is split over the workgroups (the token rows are 40 - 170 thousand, the outputs 512 x 512 ... 512 x 2048):
//     slice z writes its own fp32 partial, summed in slice order by the caller's reduce launch -- deterministic.
// Tile 128 x 256 (I x J), BK = 32 tokens, 8 wavefronts as 2 x 4 (wave tile 64 x 64), two LDS stages of 72 KB, register-staged
// global loads one iteration ahead; I % 128 == 0 and J % 256 == 0 (every Conv1D of the GPT-2 shapes), rows past M read as zero
// through the buffer range check.
// Shared with gemm_b1tn.hip (gemm_tn_common.h, gemm_tn_tail.h): the shape, the A item's staging coordinates, the column sums, the
// transposed fragment read, the pipeline (TN_PIPELINE) and the tail.  This file's own: three plane images, TN_SPLIT8, two fragment sets, six products.
#include <string.h>
#include "gemm_tn_common.h"

namespace r4d {

// `dbp` (nullable): partial column sums of dY per slice, [slices][J] -- the bias gradient db = sum over the token rows of dY falls
// out of the staging of the dY tiles (the workgroups of the first I tile add the values they stage anyway: 16 adds per k-tile
// and thread), summed per thread over its tokens in order, then over the 16 threads of a column chunk in order: a fixed order
__global__ __launch_bounds__(512, 2) void gemm_s3tn_kernel(const float* __restrict__ Xg, const float* __restrict__ Yg,
                                                           float* __restrict__ Cg, const TnShape g, float* __restrict__ dbp) {
    constexpr int BI = 128, BJ = 256, BK = 32, WI = 64, WJ = 64, TI = 2, TJ = 2;
    constexpr int A_ROW = BI * 2, B_ROW = BJ * 2;                     // bytes per token row of one plane image
    constexpr int A_PLANE = BK * A_ROW, B_PLANE = BK * B_ROW;         // 8 KB, 16 KB
    constexpr int STAGE = 3 * (A_PLANE + B_PLANE);                    // 72 KB
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];
    const int tiles_j = g.J / BJ;
    const int ti = blockIdx.x / tiles_j, tj = blockIdx.x % tiles_j;
    const int i0 = ti * BI, j0 = tj * BJ;
    const int m_lo = blockIdx.z * g.kper, m_hi = min(g.M, m_lo + g.kper);
    const int nkt = (m_hi - m_lo + BK - 1) / BK;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wi = wid >> 2, wj = wid & 3;

    // staging: a thread owns 8 consecutive features of one token: the A item (TN_A_ITEM), B items (token = idx >> 5,
    // chunk = idx & 31) for idx = tid, tid + 512.  Rows past M: the buffer range check returns zeros.
    TN_A_ITEM
    int b_voff[2], b_dst[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int idx = tid + r * 512, tok = idx >> 5, ch = idx & 31;
        b_voff[r] = (tok * g.ldb + j0 + ch * 8) * 4;
        b_dst[r] = tok * B_ROW + ((ch ^ ((tok & 3) << 2)) << 4);
    }
    // descriptors end at row M: whole rows beyond it are out of range (zeros)
    const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Xg), 0, (int)((long long)g.M * g.lda * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Yg), 0, (int)((long long)g.M * g.ldb * 4), 0x00020000);
    u32x4 ra[2], rb[2][2];
    const bool do_cs = dbp != nullptr && ti == 0;                     // workgroup-uniform
    float cs[8];                                                      // TN_COLSUM
#pragma unroll
    for (int e = 0; e < 8; ++e) cs[e] = 0.f;
#define TN_LOAD(KT)                                                                                \
    {                                                                                              \
        const int so_a_ = (m_lo + (KT) * BK) * g.lda * 4, so_b_ = (m_lo + (KT) * BK) * g.ldb * 4; \
        ra[0] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, a_voff, so_a_, 0);                   \
        ra[1] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, a_voff + 16, so_a_, 0);              \
        _Pragma("unroll") for (int r = 0; r < 2; ++r) {                                            \
            rb[r][0] = __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, b_voff[r], so_b_, 0);         \
            rb[r][1] = __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, b_voff[r] + 16, so_b_, 0);    \
        }                                                                                          \
    }
#define TN_SPLIT8(R0, R1, H, Mi, L)                                                                \
    {                                                                                              \
        const f32x4 s0_ = __builtin_bit_cast(f32x4, R0), s1_ = __builtin_bit_cast(f32x4, R1);    \
        unsigned hh_[4], mm_[4], ll_[4];                                                           \
        split3_pair(s0_[0], s0_[1], hh_[0], mm_[0], ll_[0]); split3_pair(s0_[2], s0_[3], hh_[1], mm_[1], ll_[1]); \
        split3_pair(s1_[0], s1_[1], hh_[2], mm_[2], ll_[2]); split3_pair(s1_[2], s1_[3], hh_[3], mm_[3], ll_[3]); \
        H = u32x4{hh_[0], hh_[1], hh_[2], hh_[3]}; Mi = u32x4{mm_[0], mm_[1], mm_[2], mm_[3]}; L = u32x4{ll_[0], ll_[1], ll_[2], ll_[3]}; \
    }
#define TN_STORE(STG)                                                                              \
    {                                                                                              \
        unsigned char* st_ = lds + (STG) * STAGE;                                                  \
        u32x4 h_, m_, l_;                                                                          \
        TN_SPLIT8(ra[0], ra[1], h_, m_, l_)                                                        \
        *reinterpret_cast<u32x4*>(st_ + a_dst) = h_;                                               \
        *reinterpret_cast<u32x4*>(st_ + A_PLANE + a_dst) = m_;                                     \
        *reinterpret_cast<u32x4*>(st_ + 2 * A_PLANE + a_dst) = l_;                                 \
        _Pragma("unroll") for (int r = 0; r < 2; ++r) {                                            \
            TN_SPLIT8(rb[r][0], rb[r][1], h_, m_, l_)                                              \
            *reinterpret_cast<u32x4*>(st_ + 3 * A_PLANE + b_dst[r]) = h_;                          \
            *reinterpret_cast<u32x4*>(st_ + 3 * A_PLANE + B_PLANE + b_dst[r]) = m_;                \
            *reinterpret_cast<u32x4*>(st_ + 3 * A_PLANE + 2 * B_PLANE + b_dst[r]) = l_;            \
        }                                                                                          \
    }
    // transposed fragment reads (TN_FRAG has the lane decomposition): one offset per 32-feature tile
    const int fh = lane >> 5, fg = (lane >> 4) & 1, fq = (lane & 15) >> 2, fp = lane & 3;
    int a_foff[TI], b_foff[TJ];
#pragma unroll
    for (int t = 0; t < TI; ++t) {
        const int ft = (wi * WI + t * 32) >> 5;                       // 32-feature tile index inside the 128-wide image
        a_foff[t] = (8 * fh + fq) * A_ROW + ((((ft ^ fq) << 2) | (2 * fg + (fp >> 1))) << 4) + 8 * (fp & 1);
    }
#pragma unroll
    for (int t = 0; t < TJ; ++t) {
        const int ft = (wj * WJ + t * 32) >> 5;
        b_foff[t] = (8 * fh + fq) * B_ROW + ((((ft ^ fq) << 2) | (2 * fg + (fp >> 1))) << 4) + 8 * (fp & 1);
    }
    u32x4 fa[2][TI][3], fb[2][TJ][3];
#define TN_FRAGS(SET, STG, S)                                                                      \
    {                                                                                              \
        const unsigned char* st_ = lds + (STG) * STAGE;                                            \
        _Pragma("unroll") for (int t = 0; t < TI; ++t) TN_FRAG(fa[SET][t][2], st_ + 2 * A_PLANE + a_foff[t], A_ROW, S) \
        _Pragma("unroll") for (int t = 0; t < TJ; ++t) TN_FRAG(fb[SET][t][0], st_ + 3 * A_PLANE + b_foff[t], B_ROW, S) \
        _Pragma("unroll") for (int t = 0; t < TI; ++t) TN_FRAG(fa[SET][t][0], st_ + a_foff[t], A_ROW, S) \
        _Pragma("unroll") for (int t = 0; t < TJ; ++t) TN_FRAG(fb[SET][t][2], st_ + 3 * A_PLANE + 2 * B_PLANE + b_foff[t], B_ROW, S) \
        _Pragma("unroll") for (int t = 0; t < TI; ++t) TN_FRAG(fa[SET][t][1], st_ + A_PLANE + a_foff[t], A_ROW, S) \
        _Pragma("unroll") for (int t = 0; t < TJ; ++t) TN_FRAG(fb[SET][t][1], st_ + 3 * A_PLANE + B_PLANE + b_foff[t], B_ROW, S) \
    }
    f32x16 acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#define TN_MFMA(A_, B_, I_, J_) \
    acc[I_][J_] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A_), __builtin_bit_cast(bf16x8, B_), acc[I_][J_], 0, 0, 0)
#define TN_MFMAS(SET)                                                                              \
    {                                                                                              \
        _Pragma("unroll") for (int i = 0; i < TI; ++i) _Pragma("unroll") for (int j = 0; j < TJ; ++j) TN_MFMA(fa[SET][i][2], fb[SET][j][0], i, j); \
        _Pragma("unroll") for (int i = 0; i < TI; ++i) _Pragma("unroll") for (int j = 0; j < TJ; ++j) TN_MFMA(fa[SET][i][0], fb[SET][j][2], i, j); \
        _Pragma("unroll") for (int i = 0; i < TI; ++i) _Pragma("unroll") for (int j = 0; j < TJ; ++j) TN_MFMA(fa[SET][i][1], fb[SET][j][1], i, j); \
        _Pragma("unroll") for (int i = 0; i < TI; ++i) _Pragma("unroll") for (int j = 0; j < TJ; ++j) TN_MFMA(fa[SET][i][1], fb[SET][j][0], i, j); \
        _Pragma("unroll") for (int i = 0; i < TI; ++i) _Pragma("unroll") for (int j = 0; j < TJ; ++j) TN_MFMA(fa[SET][i][0], fb[SET][j][1], i, j); \
        _Pragma("unroll") for (int i = 0; i < TI; ++i) _Pragma("unroll") for (int j = 0; j < TJ; ++j) TN_MFMA(fa[SET][i][0], fb[SET][j][0], i, j); \
    }
    // iteration kt: registers (k-tile kt+1) -> the other stage, loads of k-tile kt+2 (rows past m_hi of THIS slice are
    // real rows of the next slice -- they must not be added here: the loop bound keeps kt + 1 < nkt for every store that is
    // used, and the slice length is a multiple of BK, so only the global tail relies on the zero fill)
#define TN_ITER(CUR)                                                                               \
    {                                                                                              \
        TN_FRAGS(0, CUR, 0)                                                                        \
        TN_COLSUM(kt + 1)                                                                          \
        TN_STORE((CUR) ^ 1)                                                                        \
        TN_LOAD(kt + 2)                                                                            \
        TN_FRAGS(1, CUR, 1)                                                                        \
        TN_MFMAS(0)                                                                                \
        TN_MFMAS(1)                                                                                \
        __syncthreads();                                                                           \
    }
    TN_PIPELINE(TN_LOAD, TN_STORE, TN_ITER)
#undef TN_ITER
#undef TN_MFMAS
#undef TN_MFMA
#undef TN_FRAGS
#undef TN_STORE
#undef TN_SPLIT8
#undef TN_LOAD
#include "gemm_tn_tail.h"
}

// partials [tn_row_slices(M, S)][I][J] <- X^T . dY per slice, ALWAYS as partials (also for one slice: train.hip's weight_grad launches
// the reduce either way); db_partials (nullable) [slices][J] <- the slices' column sums of dY
int launch_gemm_s3tn(const float* X, const float* dY, float* out, float* db_partials, int I, int J, int M, int lda, int ldb, int S,
                     hipStream_t stream) {
    R4D_REQUIRE(gemm_s3tn_supported(I, J, M, lda, ldb), "gemm_s3tn: unsupported shape I=%d J=%d M=%d", I, J, M);
    R4D_REQUIRE(((uintptr_t)X % 16) == 0 && ((uintptr_t)dY % 16) == 0 && ((uintptr_t)out % 16) == 0, "gemm_s3tn: 16-byte alignment");
    const TnShape sh = tn_shape(I, J, M, lda, ldb, S);
    ProfScope prof(PK_GEMM_S3TN, 2.0 * (double)I * J * M, stream);
    R4D_BRANCH(S3_TN);
    hipLaunchKernelGGL(gemm_s3tn_kernel, tn_grid(sh), dim3(512), 0, stream, X, dY, out, sh, db_partials);
    R4D_CHECK_LAUNCH("gemm_s3tn");
    return R4D_OK;
}

}  // namespace r4d
