// Weight gradients of the opt-in "bf16" training precision: C[I,J] = sum over the token rows m of RN_bf16(X[m,I]) . RN_bf16(dY[m,J])
// with ONE v_mfma_f32_32x32x16_bf16 per k-step and fp32 accumulation -- gemm_s3tn.hip without the split arithmetic, the way
// gemm_b1.hip is gemm_s3.hip without it.  NOT fp32-accurate: both operands carry 8 significant bits.
//   * both tiles (32 tokens x 128 features of X, 32 tokens x 256 features of dY) are rounded to bf16 (round to nearest even,
//     v_cvt_pk_bf16_f32) while they are staged: one conversion per pair instead of split3_pair's three and two subtractions;
//   * the LDS images stay token-major and the k-contiguous MFMA fragments come out of `ds_read_b64_tr_b16` with gemm_s3tn's
//     XOR swizzle (chunk index ^ (token & 3) << 2), one image per operand instead of three;
//   * the contraction is split over the workgroups: slice z writes its own fp32 partial, summed in slice order by the caller's
//     reduce launch.  One slice writes C itself.  No atomics, no state across workgroups: the same bits on every run.
// db[J] = column sums of the UNROUNDED dY, from the staged fp32 values in gemm_s3tn's fixed order.
// Tile 128 x 256 (I x J), BK = 32 tokens, 8 wavefronts as 2 x 4 (wave tile 64 x 64).  A stage is 24 KB instead of 72: the room
// goes to a SECOND WORKGROUP PER CU (two stages of 24 KB each, <= 128 VGPRs), not to a deeper ring -- with a sixth of the MFMA
// work per k-tile the loop waits on the global loads and on its one barrier per k-tile, and a co-resident workgroup fills both
// kinds of wait, where a third stage fills only the first.  The cap of 128 VGPRs that goes with it leaves room for ONE fragment
// set (the reads of k-step 1 are issued behind the MFMAs of k-step 0, not under them; a second set spilled).  I % 128 == 0, J % 256 == 0, M >= 32; rows past M read as zero
// through the buffer range check.
// Shared with gemm_s3tn.hip (gemm_tn_common.h, gemm_tn_tail.h): the shape, the A item's staging coordinates, the column sums, the
// transposed fragment read, the pipeline (TN_PIPELINE) and the tail.  This file's own: one image, BT_ROUND8, one fragment set, the second B item's addresses by
// uniform terms, the k-tile offset in the vector offset, the 128-VGPR cap.
#include <string.h>
#include "gemm_tn_common.h"

namespace r4d {

struct B1TnShape : TnShape {};                                         // (its own name: the kernel's symbol carries it)

// `dbp` (nullable): partial column sums of dY per slice, [slices][J], by the workgroups of the first I tile (gemm_s3tn.hip)
// XBF (training, r4d_set_train_act_bf16): X is bf16 [M, lda] in memory -- the bits its producer rounded once -- behind the float pointer:
// the A item is ONE 16-byte load of eight bf16 and no rounding; dY stays fp32 (db sums its unrounded values).  Same image, slices, order.
template <bool XBF>
__global__ __launch_bounds__(512, 4) void gemm_b1tn_kernel(const float* __restrict__ Xg, const float* __restrict__ Yg,
                                                           float* __restrict__ Cg, const B1TnShape g, float* __restrict__ dbp) {
    constexpr int BI = 128, BJ = 256, BK = 32, WI = 64, WJ = 64, TI = 2, TJ = 2;
    constexpr int A_ROW = BI * 2, B_ROW = BJ * 2;                     // bytes per token row of an image
    constexpr int A_IMG = BK * A_ROW, B_IMG = BK * B_ROW;             // 8 KB, 16 KB
    constexpr int STAGE = A_IMG + B_IMG;                              // 24 KB
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
    constexpr int XSZ = XBF ? 2 : 4;                                  // bytes per X element in memory
    const int ax_voff = XBF ? (a_voff >> 1) : a_voff;
    // (the second B item is 16 tokens further down: the same swizzle class, so both of its addresses are the first one's plus a
    //  uniform term -- kept as such, every VGPR counts under the 128 cap)
    const int b_tok = tid >> 5, b_ch = tid & 31;
    const int b_voff0 = (b_tok * g.ldb + j0 + b_ch * 8) * 4, b_vstep = 16 * g.ldb * 4;
    const int b_dst0 = A_IMG + b_tok * B_ROW + ((b_ch ^ ((b_tok & 3) << 2)) << 4);
    // descriptors end at row M: whole rows beyond it are out of range (zeros).  With lda > I / ldb > J the last row's range ends
    // behind its last feature, inside the caller's wider buffer.
    const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Xg), 0, (int)(((long long)(g.M - 1) * g.lda + g.I) * XSZ), 0x00020000);
    const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Yg), 0, (int)(((long long)(g.M - 1) * g.ldb + g.J) * 4), 0x00020000);
    u32x4 ra[XBF ? 1 : 2], rb[2][2];
    const bool do_cs = dbp != nullptr && ti == 0;                     // workgroup-uniform
    float cs[8];                                                      // TN_COLSUM
#pragma unroll
    for (int e = 0; e < 8; ++e) cs[e] = 0.f;
#define BT_LOAD(KT)                                                                                \
    {   /* the k-tile's row offset travels in the VECTOR offset: the range check then covers it whatever it does with a scalar one */ \
        const int so_a_ = (m_lo + (KT) * BK) * g.lda * XSZ, so_b_ = (m_lo + (KT) * BK) * g.ldb * 4; \
        ra[0] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, ax_voff + so_a_, 0, 0);              \
        if constexpr (!XBF) ra[XBF ? 0 : 1] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, ax_voff + so_a_ + 16, 0, 0); \
        _Pragma("unroll") for (int r = 0; r < 2; ++r) {                                            \
            rb[r][0] = __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, b_voff0 + r * b_vstep + so_b_, 0, 0); \
            rb[r][1] = __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, b_voff0 + r * b_vstep + so_b_ + 16, 0, 0); \
        }                                                                                          \
    }
    // (cast the WHOLE vector: __builtin_bit_cast on an ext-vector element reads element 0)
#define BT_ROUND8(R0, R1, H)                                                                       \
    {                                                                                              \
        const f32x4 s0_ = __builtin_bit_cast(f32x4, R0), s1_ = __builtin_bit_cast(f32x4, R1);    \
        H = u32x4{cvt_pk_bf16(s0_[0], s0_[1]), cvt_pk_bf16(s0_[2], s0_[3]), cvt_pk_bf16(s1_[0], s1_[1]), cvt_pk_bf16(s1_[2], s1_[3])}; \
    }
#define BT_STORE(STG)                                                                              \
    {                                                                                              \
        unsigned char* st_ = lds + (STG) * STAGE;                                                  \
        u32x4 h_;                                                                                  \
        if constexpr (XBF) h_ = ra[0]; else BT_ROUND8(ra[0], ra[XBF ? 0 : 1], h_)                  \
        *reinterpret_cast<u32x4*>(st_ + a_dst) = h_;                                               \
        _Pragma("unroll") for (int r = 0; r < 2; ++r) {                                            \
            BT_ROUND8(rb[r][0], rb[r][1], h_)                                                      \
            *reinterpret_cast<u32x4*>(st_ + b_dst0 + r * 16 * B_ROW) = h_;                         \
        }                                                                                          \
    }
    // transposed fragment reads (TN_FRAG has the lane decomposition).  32-feature tile index ft inside the image: a wave's first
    // tile is even, its second the next one -- (ft ^ q) << 6 differs in bit 6
    const int fh = lane >> 5, fg = (lane >> 4) & 1, fq = (lane & 15) >> 2, fp = lane & 3;
    const int a_foff0 = (8 * fh + fq) * A_ROW + (((((wi * WI) >> 5) ^ fq) << 2 | (2 * fg + (fp >> 1))) << 4) + 8 * (fp & 1);
    const int b_foff0 = A_IMG + (8 * fh + fq) * B_ROW + (((((wj * WJ) >> 5) ^ fq) << 2 | (2 * fg + (fp >> 1))) << 4) + 8 * (fp & 1);
    static_assert(TI == 2 && TJ == 2 && WI == 64 && WJ == 64, "the second tile's offset is the first one's with bit 6 flipped");
    u32x4 fa[1][TI], fb[1][TJ];                                       // ONE fragment set: a second one spills under the 128-VGPR cap
#define BT_FRAGS(SET, STG, S)                                                                      \
    {                                                                                              \
        const unsigned char* st_ = lds + (STG) * STAGE;                                            \
        _Pragma("unroll") for (int t = 0; t < TI; ++t) TN_FRAG(fa[SET][t], st_ + (a_foff0 ^ (t << 6)), A_ROW, S) \
        _Pragma("unroll") for (int t = 0; t < TJ; ++t) TN_FRAG(fb[SET][t], st_ + (b_foff0 ^ (t << 6)), B_ROW, S) \
    }
    f32x16 acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#define BT_MFMAS(SET)                                                                              \
    _Pragma("unroll") for (int i = 0; i < TI; ++i) _Pragma("unroll") for (int j = 0; j < TJ; ++j)  \
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[SET][i]), __builtin_bit_cast(bf16x8, fb[SET][j]), acc[i][j], 0, 0, 0);
    // iteration kt: registers (k-tile kt+1) -> the other stage, loads of k-tile kt+2 (rows past m_hi of THIS slice are real rows
    // of the next slice -- they must not be added here: the loop bound keeps kt + 1 < nkt for every store that is used, and the
    // slice length is a multiple of BK, so only the global tail relies on the zero fill)
#define BT_ITER(CUR)                                                                               \
    {                                                                                              \
        BT_FRAGS(0, CUR, 0)                                                                        \
        TN_COLSUM(kt + 1)                                                                          \
        BT_STORE((CUR) ^ 1)                                                                        \
        BT_LOAD(kt + 2)                                                                            \
        BT_MFMAS(0)                                                                                \
        BT_FRAGS(0, CUR, 1)                                                                        \
        BT_MFMAS(0)                                                                                \
        __syncthreads();                                                                           \
    }
    TN_PIPELINE(BT_LOAD, BT_STORE, BT_ITER)
#undef BT_ITER
#undef BT_MFMAS
#undef BT_FRAGS
#undef BT_STORE
#undef BT_ROUND8
#undef BT_LOAD
#include "gemm_tn_tail.h"
}

// out (S slices with rows: [S][I][J], else [I][J]) <- RN(X)^T . RN(dY) per slice, db_out (nullable; [S][J] / [J]) <- the slices' column
// sums of dY.  train.hip (wgrad_b1tn) sizes the slices and sums the partials.
int launch_gemm_b1tn(const float* X, const float* dY, float* out, float* db_out, int I, int J, int M, int lda, int ldb, int S,
                     hipStream_t stream, bool x_bf16) {
    R4D_REQUIRE(X && dY && out && S >= 1, "gemm_b1tn: null pointer");
    R4D_REQUIRE(!x_bf16 || lda % 8 == 0, "gemm_b1tn: a bf16 X operand wants lda %% 8 == 0 (lda=%d)", lda);
    R4D_REQUIRE(gemm_b1tn_supported(I, J, M, lda, ldb), "gemm_b1tn: unsupported shape I=%d J=%d M=%d lda=%d ldb=%d (I %% 128 == 0, J %% 256 == 0, M >= 32 wanted)", I, J, M, lda, ldb);
    R4D_REQUIRE(((uintptr_t)X % 16) == 0 && ((uintptr_t)dY % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)db_out % 16) == 0,
                "gemm_b1tn: 16-byte alignment");
    const B1TnShape sh{tn_shape(I, J, M, lda, ldb, S)};
    ProfScope prof(PK_GEMM_B1TN, 2.0 * (double)I * J * M, stream);
    if (x_bf16) hipLaunchKernelGGL(gemm_b1tn_kernel<true>, tn_grid(sh), dim3(512), 0, stream, X, dY, out, sh, db_out);
    else hipLaunchKernelGGL(gemm_b1tn_kernel<false>, tn_grid(sh), dim3(512), 0, stream, X, dY, out, sh, db_out);
    R4D_CHECK_LAUNCH("gemm_b1tn");
    return R4D_OK;
}

}  // namespace r4d
