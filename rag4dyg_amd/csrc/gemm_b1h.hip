// The per-head attention products of the opt-in "+attn" training precisions (r4d_set_train_attention_bf16): per batch index
// z = (sequence, head)   C[T, N] = epilogue(RN_bf16(A[T, K]) . RN_bf16(B))   with ONE v_mfma_f32_32x32x16_bf16 per k-step and fp32
// accumulation in a fixed k order.  NOT fp32-accurate: both operands carry 8 significant bits.
// It takes the GemmArgs train.hip's head_gemm builds for the exact-f32 kernel (gemm_f32.hip) and serves both operand forms:
//   NT (b_trans): B is [N, K], k-contiguous like A -- S = Q . K^T and dP = dO . V^T (K = head_dim);
//   NN:           B is [K, N], N = head_dim          -- P . V, dQ, dK, dV (K = T or up4(T)).
// Both fp32 operands are rounded (round to nearest even, v_cvt_pk_bf16_f32) while they are staged.  Every LDS image is
// [row][32 k] bf16 with 64-byte rows, so that a lane's MFMA fragment (8 consecutive k of its row) is ONE ds_read_b128: the NN form
// transposes while it stages -- a thread loads the same four columns of two consecutive k rows, packs the four (k, k + 1) pairs
// and writes each as one dword of its column's image row.  The 16-byte chunk index of a row is XORed with (row >> 2) & 3: the
// 16-lane groups of ds_read_b128 then meet 16 different (row & 3, chunk) slots of the 256-byte bank row (conflict-free), the
// ds_write_b64 of the k-contiguous staging is conflict-free as it stands, and the transposing ds_write_b32 rotates which of its
// four columns a lane writes first by (lane >> 2) & 3, which leaves it 2-way (free: the store's register transfer costs as much).
// Tile 64 x 64 x 32, four wavefronts as 2 x 2, one 32 x 32 accumulator each; two 8 KB stages, the next k-tile's global loads in
// flight under the MFMAs, one barrier per k-tile.  Small on purpose: T <= 1024 rows and head_dim columns per batch index give few
// tiles each, and 16 KB / 256 threads let several workgroups share a CU (5-6 wavefronts per SIMD).  The NN form at 64 < head_dim
// <= 128 takes a 64 x 128 tile (two accumulators per wavefront, 3 wavefronts per SIMD): ONE column tile, so that A -- P-shaped,
// the large operand -- is staged once per row tile (measured at head_dim 96: 1.64 -> 1.35 ms over the 24 launches of an LM step;
// at head_dim 256 a 64 x 256 tile at 2 wavefronts per SIMD was measured SLOWER than four 64-column tiles, which that shape keeps:
// profiles/train_bf16_attention.md).
// Memory rules (include/r4d.h "WHAT A BUFFER MAY HOLD ON ENTRY"): a contraction index at or past min(K, a_cols, the causal
// trim, and b_rows in the NN form) and rows / columns past M / N contribute an exact zero BY SELECTION on both operands, so
// what the memory holds there (NaN included) never reaches a product; out-of-range addresses are clamped to valid ones; nothing
// outside C's [M, N] block is written.  No atomics, no split-K, no state across workgroups: a (sequence, head)'s bits depend on
// its own operands alone.
#include <stdlib.h>
#include <string.h>
#include "gemm_common.h"
#include "bf16x3.h"               // cvt_pk_bf16: the rounding; bf16x8

namespace r4d {

struct B1hShape {
    int M, N, K, lda, ldb, ldc, b_rows, a_cols, nb1, epilogue, causal;
    long long sA0, sA1, sB0, sB1, sC0, sC1;
    float scale_div;
};

// TN: 32-column MFMA tiles per wavefront (1 or 2): the workgroup's tile is 64 x 64 TN
template <bool BT, int TN>
__global__ __launch_bounds__(256) void gemm_b1h_kernel(const float* __restrict__ Ag, const float* __restrict__ Bg,
                                                       float* __restrict__ Cg, const B1hShape g) {
    constexpr int BM = 64, BN = 64 * TN, BK = 32;
    constexpr int ROW = BK * 2;                                       // bytes per image row
    constexpr int IMG = BM * ROW, STAGE = IMG + BN * ROW;             // A: 4 KB, B: 4 KB x TN
    static_assert(TN == 1 || TN == 2, "tile");
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];

    const int tiles_n = (g.N + BN - 1) / BN;
    const int m0 = (int)(blockIdx.x / tiles_n) * BM, n0 = (int)(blockIdx.x % tiles_n) * BN;
    if (g.causal == CAUSAL_QK && n0 > m0 + BM - 1) return;            // tile strictly above the diagonal (workgroup-uniform)

    const int z0 = blockIdx.z / g.nb1, z1 = blockIdx.z % g.nb1;
    const float* __restrict__ A = Ag + z0 * g.sA0 + z1 * g.sA1;
    const float* __restrict__ B = Bg + z0 * g.sB0 + z1 * g.sB1;
    float* __restrict__ C = Cg + z0 * g.sC0 + z1 * g.sC1;

    // the contraction indices that count: [0, klim), the same bound on both operands (>= 1: the launcher checks its terms)
    int klim = min(g.K, g.a_cols);
    if (g.causal == CAUSAL_PV) klim = min(klim, m0 + BM);             // keys beyond the tile's last row are masked
    if (!BT) klim = min(klim, g.b_rows);
    const int nkt = (klim + BK - 1) / BK;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;

    // k-contiguous staging (A; B in the NT form): item idx = tid, tid + 256 is four k of row idx >> 3
    constexpr int NB = BT ? 2 * TN : TN;                              // B items per thread
    const float* a_src[2]; bool a_ok[2];
    const float* b_src[NB]; bool b_ok[NB];
    int kc_dst[2];                                                    // (an item 32 rows further down: + 32 ROW, the same swizzle)
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int idx = tid + r * 256, row = idx >> 3, c4 = idx & 7;
        a_ok[r] = m0 + row < g.M;
        a_src[r] = A + (long long)min(m0 + row, g.M - 1) * g.lda;
        kc_dst[r] = row * ROW + ((((c4 >> 1) ^ ((row >> 2) & 3)) << 4) | ((c4 & 1) << 3));
    }
    if (BT) {
#pragma unroll
        for (int r = 0; r < NB; ++r) {
            const int row = (tid >> 3) + 32 * r;
            b_ok[r] = n0 + row < g.b_rows;
            b_src[r] = B + (long long)min(n0 + row, g.b_rows - 1) * g.ldb;
        }
    }
    const int kc_k = 4 * (tid & 7);
    // transposing staging (B in the NN form): columns n0 + 4 c .. + 3 of the k rows 2 kp and 2 kp + 1
    // (item t is 64 columns further right: the same rotation, the same swizzle, + 64 ROW in the image)
    const int t_c = tid & 15, t_kp = tid >> 4, t_rot = (t_c >> 2) & 3;
    bool t_ok[TN];                                                    // (N % 4 == 0: the four columns stand or fall together)
    const float* t_src[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) {
        t_ok[t] = n0 + 64 * t + 4 * t_c < g.N;
        t_src[t] = B + (t_ok[t] ? n0 + 64 * t + 4 * t_c : 0);
    }
    // image row 4 c + j, chunk (kp >> 2) ^ (row >> 2 & 3) = (kp >> 2) ^ (c & 3), dword kp & 3
    const int t_dst = (4 * t_c) * ROW + ((((t_kp >> 2) ^ (t_c & 3)) << 4) | ((t_kp & 3) << 2));

    f32x4 ra[2], rb[BT ? NB : 2 * TN];                                // NN: the two k rows of item t in rb[2 t], rb[2 t + 1]
    int ra_k, rb_k[2];                                                // A and NT: the items' first k; NN: the two k rows
#define BH_LOAD(KT)                                                                                              \
    {                                                                                                            \
        const int k0_ = (KT) * BK;                                                                               \
        const int k_ = k0_ + kc_k, ko_ = k_ < klim ? k_ : 0;                                                     \
        ra_k = k_;                                                                                               \
        _Pragma("unroll") for (int r = 0; r < 2; ++r) ra[r] = *reinterpret_cast<const f32x4*>(a_src[r] + ko_);   \
        if (BT) {                                                                                                \
            _Pragma("unroll") for (int r = 0; r < NB; ++r) rb[r] = *reinterpret_cast<const f32x4*>(b_src[r] + ko_); \
        } else {                                                                                                 \
            _Pragma("unroll") for (int r = 0; r < 2; ++r) {                                                      \
                const int kr_ = k0_ + 2 * t_kp + r;                                                              \
                rb_k[r] = kr_;                                                                                   \
                _Pragma("unroll") for (int t = 0; t < TN; ++t)                                                   \
                    rb[2 * t + r] = *reinterpret_cast<const f32x4*>(t_src[t] + (long long)min(kr_, klim - 1) * g.ldb); \
            }                                                                                                    \
        }                                                                                                        \
    }
    // the selection happens here, after the MFMA phase: masking right behind the load would put its wait in front of the MFMAs
#define BH_SEL4(V, OK, K0)                                                                                       \
    {                                                                                                            \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) V[e] = ((OK) && (K0) + e < klim) ? V[e] : 0.f;             \
    }
#define BH_STORE(STG)                                                                                            \
    {                                                                                                            \
        unsigned char* st_ = lds + (STG) * STAGE;                                                                \
        _Pragma("unroll") for (int r = 0; r < 2; ++r) {                                                          \
            BH_SEL4(ra[r], a_ok[r], ra_k)                                                                        \
            *reinterpret_cast<u32x2*>(st_ + kc_dst[r]) = u32x2{cvt_pk_bf16(ra[r][0], ra[r][1]), cvt_pk_bf16(ra[r][2], ra[r][3])}; \
        }                                                                                                        \
        if (BT) {                                                                                                \
            _Pragma("unroll") for (int r = 0; r < NB; ++r) {                                                     \
                BH_SEL4(rb[r], b_ok[r], ra_k)                                                                    \
                *reinterpret_cast<u32x2*>(st_ + IMG + kc_dst[0] + r * 32 * ROW) = u32x2{cvt_pk_bf16(rb[r][0], rb[r][1]), cvt_pk_bf16(rb[r][2], rb[r][3])}; \
            }                                                                                                    \
        } else {                                                                                                 \
            _Pragma("unroll") for (int t = 0; t < TN; ++t) {                                                     \
                unsigned p_[4];                                                                                  \
                _Pragma("unroll") for (int e = 0; e < 4; ++e)                                                    \
                    p_[e] = cvt_pk_bf16((t_ok[t] && rb_k[0] < klim) ? rb[2 * t][e] : 0.f, (t_ok[t] && rb_k[1] < klim) ? rb[2 * t + 1][e] : 0.f); \
                _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                  \
                    const int j_ = (i + t_rot) & 3;                                                              \
                    const unsigned v_ = t_rot == 0 ? p_[i] : t_rot == 1 ? p_[(i + 1) & 3] : t_rot == 2 ? p_[(i + 2) & 3] : p_[(i + 3) & 3]; \
                    *reinterpret_cast<unsigned*>(st_ + IMG + t_dst + (64 * t + j_) * ROW) = v_;                   \
                }                                                                                                \
            }                                                                                                    \
        }                                                                                                        \
    }

    // fragment reads: lane (r = lane & 31, h = lane >> 5) holds k = 8 h .. 8 h + 7 of its row in k-step kk: chunk 2 kk + h
    const int fr = lane & 31, fh = lane >> 5;
    const int a_row = wm * 32 + fr, b_row = wn * 32 * TN + fr;         // (B tile j of the wave: + 32 j rows, the same swizzle)
    const int a_f0 = a_row * ROW + ((fh ^ ((a_row >> 2) & 3)) << 4), a_f1 = a_row * ROW + (((2 + fh) ^ ((a_row >> 2) & 3)) << 4);
    const int b_f0 = IMG + b_row * ROW + ((fh ^ ((b_row >> 2) & 3)) << 4), b_f1 = IMG + b_row * ROW + (((2 + fh) ^ ((b_row >> 2) & 3)) << 4);

    f32x16 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    BH_LOAD(0)
    BH_STORE(0)
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nkt;
        if (more) BH_LOAD(kt + 1)                                     // in flight under the MFMA phase
        const unsigned char* st = lds + cur * STAGE;
        const u32x4 fa0 = *reinterpret_cast<const u32x4*>(st + a_f0);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const u32x4 fb0 = *reinterpret_cast<const u32x4*>(st + b_f0 + j * 32 * ROW);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa0), __builtin_bit_cast(bf16x8, fb0), acc[j], 0, 0, 0);
        }
        if (klim - kt * BK > 16) {                                    // (workgroup-uniform; the second half of a short tile is all zero)
            const u32x4 fa1 = *reinterpret_cast<const u32x4*>(st + a_f1);
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const u32x4 fb1 = *reinterpret_cast<const u32x4*>(st + b_f1 + j * 32 * ROW);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa1), __builtin_bit_cast(bf16x8, fb1), acc[j], 0, 0, 0);
            }
        }
        if (more) BH_STORE(cur ^ 1)
        __syncthreads();
    }
#undef BH_STORE
#undef BH_SEL4
#undef BH_LOAD

    // MFMA C/D layout: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5): 32 lanes store 128 contiguous bytes of a row
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = n0 + wn * 32 * TN + 32 * j + fr;
        if (col >= g.N) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
            float v = acc[j][r];
            if (g.epilogue == EPI_SCALE_DIV) v = v / g.scale_div;
            if (row < g.M) C[(long long)row * g.ldc + col] = v;
        }
    }
}

template <bool BT, int TN>
static void launch_b1h(const GemmArgs& g, const B1hShape& sh, hipStream_t stream) {
    const dim3 grid(cdiv(g.M, 64) * cdiv(g.N, 64 * TN), 1, g.nbatch);
    hipLaunchKernelGGL((gemm_b1h_kernel<BT, TN>), grid, dim3(256), 0, stream, g.A, g.B, g.C, sh);
}

int launch_gemm_b1h(const GemmArgs& g0, hipStream_t stream) {
    GemmArgs g = g0;
    R4D_REQUIRE(g.A && g.B && g.C, "gemm_b1h: null pointer");
    R4D_REQUIRE(g.M > 0 && g.N > 0 && g.K > 0, "gemm_b1h: empty problem M=%d N=%d K=%d", g.M, g.N, g.K);
    R4D_REQUIRE(g.nbatch >= 1 && g.nbatch <= 65535 && g.nb1 >= 1, "gemm_b1h: batch count %d outside [1, 65535] (grid.z limit)", g.nbatch);
    R4D_REQUIRE(g.epilogue == EPI_NONE || g.epilogue == EPI_SCALE_DIV, "gemm_b1h: epilogue %d is neither none nor scale-div", g.epilogue);
    R4D_REQUIRE(!g.bias && !g.resid, "gemm_b1h: no bias, no residual");
    R4D_REQUIRE(g.causal == CAUSAL_NONE || g.causal == CAUSAL_QK || g.causal == CAUSAL_PV, "gemm_b1h: causal flag %d", g.causal);
    if (g.a_cols <= 0) g.a_cols = g.K;
    // 16-byte loads: every row start and every batch origin on a 16-byte boundary, whole float4 inside a row
    R4D_REQUIRE(((g.lda | g.ldb | g.sA0 | g.sA1 | g.sB0 | g.sB1) & 3) == 0, "gemm_b1h: lda / ldb / operand strides must be multiples of 4");
    R4D_REQUIRE(((uintptr_t)g.A % 16) == 0 && ((uintptr_t)g.B % 16) == 0, "gemm_b1h: A / B must be 16-byte aligned");
    R4D_REQUIRE(g.a_cols <= g.lda && g.b_rows >= 1 && g.ldc >= g.N, "gemm_b1h: a_cols=%d lda=%d b_rows=%d ldc=%d N=%d", g.a_cols, g.lda, g.b_rows, g.ldc, g.N);
    if (g.b_trans) R4D_REQUIRE(g.K <= g.ldb, "gemm_b1h: K=%d exceeds ldb=%d (B as [N, K])", g.K, g.ldb);
    else R4D_REQUIRE(g.N % 4 == 0 && g.N <= g.ldb, "gemm_b1h: N=%d must be a multiple of 4 within ldb=%d (B as [K, N])", g.N, g.ldb);
    B1hShape sh;
    sh.M = g.M; sh.N = g.N; sh.K = g.K; sh.lda = g.lda; sh.ldb = g.ldb; sh.ldc = g.ldc; sh.b_rows = g.b_rows; sh.a_cols = g.a_cols;
    sh.nb1 = g.nb1; sh.epilogue = g.epilogue; sh.causal = g.causal;
    sh.sA0 = g.sA0; sh.sA1 = g.sA1; sh.sB0 = g.sB0; sh.sB1 = g.sB1; sh.sC0 = g.sC0; sh.sC1 = g.sC1; sh.scale_div = g.scale_div;
    // algorithmic flop: 2MNK dense; the causal launches count only the lower-triangular half (as gemm_f32.hip)
    const double flop = (g.causal ? 1.0 : 2.0) * (double)g.M * g.N * g.K * g.nbatch;
    ProfScope prof(g.b_trans ? PK_GEMM_B1H_NT : PK_GEMM_B1H_NN, flop, stream);
    if (g.b_trans) {
        R4D_BRANCH(TBA_NT);                                           // N = T: the output dominates, the small tile fills the chip best
        launch_b1h<true, 1>(g, sh, stream);
    } else {
        R4D_BRANCH(TBA_NN);                                           // N = head_dim
        static const int wide = [] { const char* e = getenv("R4D_B1H_WIDE"); return e ? atoi(e) : 1; }();   // tuning aid: 0 keeps 64 columns
        if (wide && g.N > 64 && g.N <= 128) launch_b1h<false, 2>(g, sh, stream);
        else launch_b1h<false, 1>(g, sh, stream);
    }
    R4D_CHECK_LAUNCH("gemm_b1h");
    return R4D_OK;
}

}  // namespace r4d
