// Plain-bf16 GEMM of the encoder's opt-in "bf16" precision: C[M,N] = epilogue(RN_bf16(A)[M,K] . RN_bf16(W)^T + bias) with ONE
// v_mfma_f32_32x32x16_bf16 per k-step and fp32 accumulation.  NOT fp32-accurate: both operands carry 8 significant bits (relative
// error of a product <= 2^-8).  bf16 x bf16 is exact in fp32, so the only other rounding is the accumulation.
//
// Operands: A is the fp32 activation [M,K], rounded to bf16 (round to nearest even, v_cvt_pk_bf16_f32; a NaN stays a NaN) while its
// tile is staged -- the first term of gemm_s3.hip's split3_pair; W is ONE k-contiguous bf16 plane [N][K] = plane 0 of what
// r4d_split3_planes_bf16 writes.  Against gemm_s3_kernel the split arithmetic, five of the six MFMAs and two thirds of the LDS
// stage are gone; what stays is its tile structure: BK = 32, 8 wavefronts, LDS rows of 64 bytes with the 16-byte chunk index
// XOR-ed with (row >> 2) & 3 (conflict-free ds_read_b128 / ds_write_b128 without padding), buffer loads with a loop-invariant lane
// offset and the k-tile in the scalar offset, out-of-range rows clamped, register-staged pipeline, one barrier per k-tile.  A
// stage is 24 KB (128 x 256) or 16 KB (128 x 128) instead of 72 / 48, so the ring is three deep and two workgroups share a CU.
//
// Summation order: every output element adds its K / 16 MFMA steps in ascending k into one accumulator, whatever the tile, M, or
// the other rows of the call -- a row's bits do not depend on the launch it travels in.  One workgroup per tile, no state across
// workgroups, no atomics.
#include <stdlib.h>
#include <string.h>
#include "bf16x3.h"               // cvt_pk_bf16: the rounding

#ifndef B1_LOAD_EARLY
#define B1_LOAD_EARLY 0   // tuning aid: 1 requests k-tile kt+3 during k-step 0 (behind the LDS stores) instead of k-step 1
#endif

namespace r4d {

struct B1Shape { int M, N, K, lda, ldc, ldr; };

// Registers: two workgroups per CU (<= 128 VGPRs) -- except the 128 x 256 tile with an epilogue that READS the second buffer
// (residual; training: the GELU derivative), whose 64 accumulators and prefetched second-buffer values do not fit 128 without
// scratch: those keep the whole file (one workgroup per CU)
//
// ABF (training, r4d_set_train_act_bf16): A is bf16 [M, lda] in memory -- the bits its producer rounded once (the same RNE) -- behind
// the float pointer: an item is ONE 16-byte load of eight bf16 where the fp32 form has two loads of four floats and four
// conversions; the same LDS image, k order, MFMA sequence and epilogues.  The descriptor's range is the bf16 block's own length.
// (The encoder under r4d_set_encode_act_bf16 reads ln1, ln2 and the GELU output this way, and the attention output under "bf16+attn".)
template <int BM, int BN, int WGM, int WGN, int EPI, bool ABF = false>
__global__ __launch_bounds__(64 * WGM * WGN, ((EPI == EPI_RESIDUAL || EPI == EPI_GELU_GRAD) && BN == 256) ? 2 : 4) void gemm_b1_kernel(
    const float* __restrict__ Ag, const unsigned short* __restrict__ Bp, float* __restrict__ Cg,
    const float* __restrict__ biasg, const float* __restrict__ residg, const B1Shape g) {
    constexpr int BK = 32, NBUF = 3, D = NBUF - 1;                    // D k-tiles between an LDS store and its use
    constexpr int NTHREADS = 64 * WGM * WGN;
    constexpr int WM = BM / WGM, WN = BN / WGN, TM = WM / 32, TN = WN / 32;
    constexpr int NIA = BM * 4 / NTHREADS, NIB = BN * 4 / NTHREADS;   // (row, 8-k chunk) items per thread
    constexpr int A_TILE = BM * 4, B_TILE = BN * 4;                   // uint4 units (a row = 4 chunks of 16 bytes)
    constexpr int STAGE = A_TILE + B_TILE;
    constexpr int ASZ = ABF ? 2 : 4, NLA = ABF ? 1 : 2;                // bytes per A element in memory; 16-byte loads per A item
    static_assert(NIA >= 1 && NIB >= 1 && NIA <= 2 && NIB <= 2 && TM >= 1 && TN >= 1, "tile");
    __shared__ u32x4 lds[NBUF * STAGE];

    int m0, n0;
    grouped_tile<BM, BN>(g.M, g.N, m0, n0);                          // XCD-aware grouped tile order
    const int nkt = g.K / BK;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WGN, wn = wid % WGN;
    const int li = lane & 31, lh = lane >> 5;

    // staging coordinates: item idx = tid + i * NTHREADS -> row = idx >> 2, chunk = idx & 3 (8 consecutive k)
    int a_off[NIA], b_off[NIB], a_dst[NIA], b_dst[NIB];
#pragma unroll
    for (int i = 0; i < NIA; ++i) {
        const int idx = tid + i * NTHREADS, row = idx >> 2, c = idx & 3;
        a_off[i] = (min(m0 + row, g.M - 1) * g.lda + c * 8) * ASZ;
        a_dst[i] = row * 4 + (c ^ ((row >> 2) & 3));
    }
#pragma unroll
    for (int i = 0; i < NIB; ++i) {
        const int idx = tid + i * NTHREADS, row = idx >> 2, c = idx & 3;
        b_off[i] = (min(n0 + row, g.N - 1) * g.K + c * 8) * 2;
        b_dst[i] = A_TILE + row * 4 + (c ^ ((row >> 2) & 3));
    }
    const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(Ag), 0, (int)(((long long)(g.M - 1) * g.lda + g.K) * ASZ), 0x00020000);
    const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned short*>(Bp), 0, (int)((long long)g.N * g.K * 2), 0x00020000);

    u32x4 ra[NIA][NLA], rb[NIB];                                      // one k-tile in flight: 8 fp32 (ABF: 8 bf16) of A, 8 bf16 of W per item
#define B1_LOAD(KT)                                                                                \
    {                                                                                              \
        const int kt_ = min((KT), nkt - 1);                                                        \
        _Pragma("unroll") for (int i = 0; i < NIA; ++i) {                                          \
            ra[i][0] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, a_off[i], kt_ * (BK * ASZ), 0); \
            if constexpr (!ABF) ra[i][NLA - 1] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, a_off[i] + 16, kt_ * (BK * ASZ), 0); \
        }                                                                                          \
        _Pragma("unroll") for (int i = 0; i < NIB; ++i)                                            \
            rb[i] = __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, b_off[i], kt_ * (BK * 2), 0);    \
    }
#define B1_STORE(STG)                                                                              \
    {                                                                                              \
        u32x4* st_ = lds + (STG) * STAGE;                                                         \
        _Pragma("unroll") for (int i = 0; i < NIA; ++i) {                                          \
            if constexpr (ABF) { st_[a_dst[i]] = ra[i][0]; continue; }                             \
            /* (cast the WHOLE vector: __builtin_bit_cast on an ext-vector element reads element 0) */ \
            const f32x4 lo_ = __builtin_bit_cast(f32x4, ra[i][0]), hi_ = __builtin_bit_cast(f32x4, ra[i][NLA - 1]); \
            u32x4 h_;                                                                             \
            h_[0] = cvt_pk_bf16(lo_[0], lo_[1]); h_[1] = cvt_pk_bf16(lo_[2], lo_[3]);              \
            h_[2] = cvt_pk_bf16(hi_[0], hi_[1]); h_[3] = cvt_pk_bf16(hi_[2], hi_[3]);              \
            st_[a_dst[i]] = h_;                                                                    \
        }                                                                                          \
        _Pragma("unroll") for (int i = 0; i < NIB; ++i) st_[b_dst[i]] = rb[i];                     \
    }

    // fragment addresses: lane (li, lh), k-step s -> chunk 2s + lh of row li (+ 32 per tile)
    const int fq = (li >> 2) & 3;
    const int f_off0 = li * 4 + ((0 + lh) ^ fq), f_off1 = li * 4 + ((2 + lh) ^ fq);
    const int fa_base = wm * WM * 4, fb_base = A_TILE + wn * WN * 4;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // fragment registers, two sets: the reads of k-step 1 travel under the MFMAs of k-step 0
    u32x4 fa[2][TM], fb[2][TN];
#define B1_FRAGS(SET, STG, S)                                                                      \
    {                                                                                              \
        const u32x4* st_ = lds + (STG) * STAGE;                                                   \
        const int fo_ = (S) ? f_off1 : f_off0;                                                     \
        _Pragma("unroll") for (int i = 0; i < TM; ++i) fa[SET][i] = st_[fa_base + i * 128 + fo_];  \
        _Pragma("unroll") for (int j = 0; j < TN; ++j) fb[SET][j] = st_[fb_base + j * 128 + fo_];  \
    }
#define B1_MFMAS(SET)                                                                              \
    _Pragma("unroll") for (int i = 0; i < TM; ++i) _Pragma("unroll") for (int j = 0; j < TN; ++j)  \
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[SET][i]), __builtin_bit_cast(bf16x8, fb[SET][j]), acc[i][j], 0, 0, 0);

    // prologue: k-tiles 0 .. D-1 into their stages, k-tile D into the staging registers (loads beyond the last k-tile repeat it)
#pragma unroll
    for (int t = 0; t < D; ++t) {
        B1_LOAD(t)
        B1_STORE(t)
    }
    B1_LOAD(D)
    __syncthreads();

    // iteration kt (the staging registers hold k-tile kt+D, requested during iteration kt-1):
    //   the fragment reads of k-step 0 of stage kt % 3;
    //   k-step 0: its MFMAs with, between them, the reads of k-step 1, the bf16 rounding of the staged A elements and the LDS
    //             stores of k-tile kt+D into stage (kt+D) % 3 (last read in iteration kt-1: every wave is past that barrier);
    //   k-step 1: its MFMAs with the global loads of k-tile kt+D+1 between them;
    //   barrier.
    // sched_group_barrier pins that interleaving, as in gemm_s3_kernel.
    constexpr int NMF = TM * TN, NFR = TM + TN, NDW = NIA + NIB, NVM = NLA * NIA + NIB;
    constexpr int FR_PER = (NFR + NMF - 1) / NMF, DW_PER = (NDW + NMF - 1) / NMF, VM_PER = (NVM + NMF - 1) / NMF;
#define B1_ITER(CUR, WR)                                                                           \
    {                                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        B1_FRAGS(0, CUR, 0)                                                                        \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        B1_STORE(WR)                                                                               \
        if (B1_LOAD_EARLY) B1_LOAD(kt + D + 1)                                                     \
        B1_FRAGS(1, CUR, 1)                                                                        \
        B1_MFMAS(0)                                                                                \
        _Pragma("unroll") for (int m_ = 0; m_ < NMF; ++m_) {                                       \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                     \
            __builtin_amdgcn_sched_group_barrier(0x100, FR_PER, 0);                                \
            if (!ABF) __builtin_amdgcn_sched_group_barrier(0x002, 2 * NIA, 0);                     \
            __builtin_amdgcn_sched_group_barrier(0x200, DW_PER, 0);                                \
            if (B1_LOAD_EARLY) __builtin_amdgcn_sched_group_barrier(0x020, VM_PER, 0);             \
        }                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        if (!B1_LOAD_EARLY) B1_LOAD(kt + D + 1)                                                    \
        B1_MFMAS(1)                                                                                \
        _Pragma("unroll") for (int m_ = 0; m_ < NMF; ++m_) {                                       \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                     \
            if (!B1_LOAD_EARLY) __builtin_amdgcn_sched_group_barrier(0x020, VM_PER, 0);            \
        }                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        __syncthreads();                                                                           \
    }
    int kt = 0;
    for (; kt + 2 < nkt; kt += 3) {                                   // compile-time stages
        B1_ITER(0, 2)
        { ++kt; B1_ITER(1, 0) }
        { ++kt; B1_ITER(2, 1) }
        kt -= 2;
    }
    int cur = 0, wr = 2;                                              // kt is a multiple of 3 here: 0..2 k-tiles left
    for (; kt < nkt; ++kt) {
        B1_ITER(cur, wr)
        cur = cur == 2 ? 0 : cur + 1;
        wr = wr == 2 ? 0 : wr + 1;
    }
#undef B1_ITER
#undef B1_MFMAS
#undef B1_FRAGS
#undef B1_STORE
#undef B1_LOAD

    // epilogue: the shared row-major one
    float* __restrict__ C = Cg;
#define EPILOGUE_VALUE(i, j, r) acc[i][j][r]
#define EPILOGUE_EDGE_PRELOAD 1
#include "gemm_epilogue_rowmajor.h"
}

// ---------------------------------------------------------------------------------------------- host side
// what the encoder forward uses, and the two kinds of the training step (c_fc forward with the kept pre-activation; the mlp
// c_proj data gradient times gelu_new'(pre))
// (EPI_NONE_BF16: c_attn of the encoder's "bf16+attn" precision)
#define B1_KINDS(X, L) X(L, EPI_NONE) X(L, EPI_GELU) X(L, EPI_RESIDUAL) X(L, EPI_GELU_KEEP) X(L, EPI_GELU_GRAD) X(L, EPI_NONE_BF16)
// with a bf16 A operand: the training forward's three consumers of a bf16 block (c_attn, c_fc, mlp c_proj)
// (the encoder's r4d_set_encode_act_bf16: c_fc as EPI_GELU_BF16 -- EPI_GELU where mlp.c_proj keeps fp32 -- and c_attn as EPI_NONE_BF16
// under "bf16+attn")
#define B1_KINDS_ABF(X, L) X(L, EPI_NONE) X(L, EPI_RESIDUAL) X(L, EPI_GELU_KEEP) X(L, EPI_GELU_KEEP_BF16) X(L, EPI_GELU) X(L, EPI_GELU_BF16) X(L, EPI_NONE_BF16)
template <int BM, int BN, int WGM, int WGN>
static int launch_b1(const S3Args& a, hipStream_t stream) {
    const int tiles = cdiv(a.M, BM) * cdiv(a.N, BN);
    ProfScope prof(PK_GEMM_B1, 2.0 * (double)a.M * a.N * a.K, stream);
    B1Shape sh;
    sh.M = a.M; sh.N = a.N; sh.K = a.K; sh.lda = a.lda; sh.ldc = a.ldc; sh.ldr = a.ldr;
#define B1_LAUNCH_(E)                                                                              \
    hipLaunchKernelGGL((gemm_b1_kernel<BM, BN, WGM, WGN, E>), dim3(tiles), dim3(64 * WGM * WGN), 0, stream, a.A, a.planes, a.C, \
                       a.bias, a.resid, sh)
#define B1_LAUNCH_ABF_(E)                                                                          \
    hipLaunchKernelGGL((gemm_b1_kernel<BM, BN, WGM, WGN, E, true>), dim3(tiles), dim3(64 * WGM * WGN), 0, stream, a.A, a.planes, a.C, \
                       a.bias, a.resid, sh)
    if (a.a_bf16) {
        R4D_EPI_DISPATCH(a.epilogue, B1_KINDS_ABF, B1_LAUNCH_ABF_, set_error("gemm_b1: epilogue %d has no instantiation with a bf16 A operand", a.epilogue); return R4D_ERR_INVALID;)
    } else {
        R4D_EPI_DISPATCH(a.epilogue, B1_KINDS, B1_LAUNCH_, set_error("gemm_b1: epilogue %d has no instantiation", a.epilogue); return R4D_ERR_INVALID;)
    }
#undef B1_LAUNCH_ABF_
#undef B1_LAUNCH_
    R4D_CHECK_LAUNCH("gemm_b1");
    return R4D_OK;
}

int launch_gemm_b1(const S3Args& a, hipStream_t stream) {
    R4D_REQUIRE(a.A && a.planes && a.C, "gemm_b1: null pointer");
    R4D_REQUIRE(gemm_b1_supported(a.M, a.K, a.N), "gemm_b1: unsupported shape M=%d K=%d N=%d (K %% 32 == 0 wanted)", a.M, a.K, a.N);
    R4D_REQUIRE(a.lda % 4 == 0 && ((uintptr_t)a.A % 16) == 0 && ((uintptr_t)a.planes % 16) == 0, "gemm_b1: alignment");
    R4D_REQUIRE((a.epilogue != EPI_RESIDUAL && a.epilogue != EPI_GELU_KEEP && a.epilogue != EPI_GELU_GRAD && a.epilogue != EPI_GELU_KEEP_BF16) || a.resid, "gemm_b1: epilogue %d needs the second buffer", a.epilogue);
    R4D_REQUIRE(!a.a_bf16 || a.lda % 8 == 0, "gemm_b1: a bf16 A operand wants lda %% 8 == 0 (lda=%d)", a.lda);
    R4D_REQUIRE((a.epilogue != EPI_GELU_KEEP_BF16 && a.epilogue != EPI_NONE_BF16 && a.epilogue != EPI_GELU_BF16) || (a.N % 2 == 0 && a.ldc % 2 == 0 && ((uintptr_t)a.C % 4) == 0), "gemm_b1: the bf16 output wants even N and ldc");
    static int forced = -2;
    if (forced == -2) { const char* e = getenv("R4D_GEMM_B1_TILE"); forced = e ? atoi(e) : -1; }   // tuning aid: 0 / 1 forces a tile
    const int t = (forced == 0 || forced == 1) ? forced : pick_tile_128(a.M, a.N);
    if (t == 0) { R4D_BRANCH(B1_128x256); return launch_b1<128, 256, 2, 4>(a, stream); }
    R4D_BRANCH(B1_128x128);
    return launch_b1<128, 128, 2, 4>(a, stream);
}

}  // namespace r4d

using namespace r4d;

extern "C" {

int r4d_conv1d_bf16_f32(const float* x_d, const uint16_t* w_bf16_d, const float* bias_d, const float* residual_d, int32_t M,
                        int32_t K, int32_t N, int32_t epilogue, float* y_d, void* stream) {
    R4D_REQUIRE(epilogue >= 0 && epilogue <= 2, "conv1d_bf16: epilogue %d not in {0,1,2}", epilogue);
    return launch_gemm_b1(s3_args(x_d, w_bf16_d, bias_d, residual_d, M, K, N, epilogue, y_d), (hipStream_t)stream);
}

int r4d_conv1d_bf16_act_f32(const uint16_t* x_bf16_d, const uint16_t* w_bf16_d, const float* bias_d, int32_t M, int32_t K, int32_t N,
                            int32_t kind, float* second_d, void* y_d, void* stream) {
    R4D_REQUIRE(kind >= 0 && kind <= 4, "conv1d_bf16_act: kind %d not in {0 none, 1 residual, 2 gelu-keep with a bf16 output, 3 gelu as bf16, 4 none as bf16}", kind);
    const bool two = kind == 1 || kind == 2;
    R4D_REQUIRE(!two || (second_d && (void*)second_d != y_d), "conv1d_bf16_act: kind %d needs the second buffer", kind);
    static const int epilogues[5] = {EPI_NONE, EPI_RESIDUAL, EPI_GELU_KEEP_BF16, EPI_GELU_BF16, EPI_NONE_BF16};
    S3Args a = s3_args(reinterpret_cast<const float*>(x_bf16_d), w_bf16_d, bias_d, two ? second_d : nullptr, M, K, N, epilogues[kind], (float*)y_d);
    a.a_bf16 = 1;
    return launch_gemm_b1(a, (hipStream_t)stream);
}

}  // extern "C"
