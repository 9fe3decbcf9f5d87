// "f16x2" GEMM with BOTH operands pre-split (round 5): C[M,N] = epilogue(A . W^T + bias), the arithmetic of
// gemm_h2.hip -- same fragments, same three products per 16 k, same two accumulator sets, the epilogue arithmetic of gemm_epilogue_rowmajor.h --
// but the A operand arrives ALREADY as f16x2 lines, written by its producer (LayerNorm: encoder_ops.hip; the c_fc GELU epilogue:
// this file) in the layout r4d_split2_planes_f16 gives the weights:
//     [rows][K/32][2][32] fp16 -- per row and 32 consecutive k ONE 128-byte line of 32 hi = RN16(x/4) then 32 lo' = RN16((x/4 - hi) 2^11)
// (the same 4 bytes per element as fp32: nothing more is read or written).  Both tiles then travel global -> LDS by DMA
// (global_load_lds_dwordx4): no VGPR staging, no split arithmetic and no ds_write in the k-loop -- what is left beside the MFMAs is
// the fragment reads.  Round 4 measured this form once (402 / 427 us against 430 / 454 for c_attn / c_fc, bit-identical) and dropped
// it for want of producers; round 5 has them.
//
// Staging: one DMA instruction = 64 lanes x 16 bytes = 8 WHOLE lines (8 rows x 128 bytes) -> 1 KB of LDS, lane-linear: lane l lands
// in row l >> 3, 16-byte slot l & 7 of that row's 128 bytes.  The image wants logical chunk c (0..3 hi, 4..7 lo') of row r in slot
// c ^ ((r >> 1) & 7) (conflict-free ds_read_b128 fragments: score.hip's image), so the lane READS chunk (l & 7) ^ ((r >> 1) & 7):
// the permutation is on the global side.  A stage = (BM + BN) rows x 128 bytes = 48 KB at 128 x 256; three stages; wavefront w
// copies A row groups 2w, 2w+1 and W row groups 4w .. 4w+3 of every k-tile (6 instructions), k-tile kt + 2 while kt is multiplied.
// ONE barrier per k-tile, in the middle of the iteration: behind `s_waitcnt vmcnt` for the wave's own copies of k-tile kt + 1, in
// front of the first fragment read of that k-tile.
#include <stdlib.h>
#include <string.h>
#include "gemm_common.h"

namespace r4d {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

int g_gemm_h2p = 1;               // r4d_set_gemm_h2p: 0 keeps the register-staged gemm_h2 kernels and fp32 activations everywhere

struct H2PShape {
    int M, N, K, ldc, ldr;
    unsigned* kblk; int kb_hd;        // EPI_H2WORDS with N = 3 d: the K columns [d, 2d) go to the key-blocked image (attention_h2.hip) instead of C
};
// ROWMAP (layer 0's c_attn without its repeated pad-row blocks; common.h: PadRowsPlan): the 32-row block `i` of the launch's row
// space is block list[i] of A, C and the key-blocked image; hdr[0] = listed blocks (a multiple of 4, on the device; the
// grid holds the most there can be); rows [m_real, round_up(m_real, 32)) and rows from m_tab on exist but hold nothing: they are
// read as rows m_real - 1 and m_tab - 1 and written like any other (H2PShape::M = the rows that exist)
struct H2PRowMap { const int* hdr; const int* list; int m_real, m_tab; };

// NI DMA instructions of 1 KB each: global address = base + 32-bit lane offset + i KB, LDS address = M0 + i KB + 16 lane (the
// instruction offset moves BOTH sides, so the lane offsets of instruction i are built i KB short); M0 restored (the compiler owns it)
__device__ __forceinline__ void h2p_dma2(const void* base, unsigned v0, unsigned v1, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %3\n\t"
                 "global_load_lds_dwordx4 %2, %3 offset:1024\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(v0), "v"(v1), "s"(base), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void h2p_dma4(const void* base, unsigned v0, unsigned v1, unsigned v2, unsigned v3, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %6\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %5\n\t"
                 "global_load_lds_dwordx4 %2, %5 offset:1024\n\t"
                 "global_load_lds_dwordx4 %3, %5 offset:2048\n\t"
                 "global_load_lds_dwordx4 %4, %5 offset:3072\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(v0), "v"(v1), "v"(v2), "v"(v3), "s"(base), "s"(lds_dst) : "memory");
}
template <int N_> __device__ __forceinline__ void h2p_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N_) : "memory"); }

// OUT_LINES (with EPI_GELU): C is the f16x2-line image of the result, [M][N/32][2][32] fp16 (the A operand of the next GEMM)
// WGM x WGN wavefronts: 2 x 4 (wave tile 64 x 64 at 128 x 256, two wavefronts per SIMD).  The 2 x 2 grid (wave tile 64 x 128, ONE
// wavefront per SIMD with the whole register file, 256 VGPRs + 256 AGPRs: 12 fragment reads per 24 MFMAs instead of 8 per 12, a
// quarter fewer LDS bytes per flop) instantiates from the same template and was measured in round 5: bit-identical and 6-19 %
// SLOWER (c_attn 389 vs 367 us, c_fc 568 vs 513, K 2048 484 vs 448 on the stand-alone probe): with one wavefront per SIMD nothing
// runs under its barrier, its fragment waits and its epilogue.  Not launched.
template <int BM, int BN, int EPI, bool OUT_LINES, int WGM = 2, int WGN = 4>
__global__ __launch_bounds__(64 * WGM * WGN, (WGM * WGN) / 4) void gemm_h2p_kernel(const unsigned short* __restrict__ Al, const unsigned short* __restrict__ Bp,
                                                          float* __restrict__ Cg, const float* __restrict__ biasg,
                                                          const float* __restrict__ residg, const H2PShape g) {
    constexpr bool ROWMAP = false;
    const H2PRowMap rm{};
#include "gemm_h2p_body.h"
}
// the same text with the row-block map (h2-word c_attn at both tile widths; every parameter stays a template parameter so that the
// text's `if constexpr` branches are discarded the same way)
template <int BM, int BN, int EPI = EPI_H2WORDS, bool OUT_LINES = false, int WGM = 2, int WGN = 4, bool ROWMAP = true>
__global__ __launch_bounds__(64 * WGM * WGN, (WGM * WGN) / 4) void gemm_h2p_rowmap_kernel(const unsigned short* __restrict__ Al, const unsigned short* __restrict__ Bp,
                                                                 float* __restrict__ Cg, const float* __restrict__ biasg,
                                                                 const H2PShape g, const H2PRowMap rm) {
    const float* __restrict__ residg = nullptr;
#include "gemm_h2p_body.h"
}

// ---------------------------------------------------------------------------------------------- fp32 rows -> f16x2 lines
// (what the producers write, as a kernel of its own: tests, and callers whose A comes from somewhere else)
__global__ __launch_bounds__(256) void split2_lines_kernel(const float* __restrict__ x, long long n4, uint2* __restrict__ lines, int K) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;     // float4 index
    if (i >= n4) return;
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    unsigned h0, l0, h1, l1;
    split2_pair<true>(v.x, v.y, h0, l0);
    split2_pair<true>(v.z, v.w, h1, l1);
    const long long e = i * 4, row = e / K;
    const int k = (int)(e - row * K);
    unsigned char* dst = reinterpret_cast<unsigned char*>(lines) + row * (long long)K * 4 + (k >> 5) * 128 + (k & 31) * 2;
    *reinterpret_cast<uint2*>(dst) = make_uint2(h0, h1);
    *reinterpret_cast<uint2*>(dst + 64) = make_uint2(l0, l1);
}

// ---------------------------------------------------------------------------------------------- host side
bool gemm_h2p_supported(int M, int K, int N) {
    return g_gemm_h2p != 0 && gemm_h2_supported(M, K, N) && (long long)M * K * 4 + 4096 < (1ll << 32) && (long long)N * K * 4 + 4096 < (1ll << 32);
}

template <int BN>
static int launch_h2p(const S3Args& a, const unsigned short* a_lines, bool out_lines, int cls, hipStream_t stream) {
    const int tiles = cdiv(a.M, 128) * cdiv(a.N, BN);
    ProfScope prof(cls, 2.0 * (double)a.M * a.N * a.K, stream);
    H2PShape sh;
    sh.M = a.M; sh.N = a.N; sh.K = a.K; sh.ldc = a.ldc; sh.ldr = a.ldr;
    sh.kblk = a.kblk; sh.kb_hd = a.kblk ? a.kb_hd : 0;
#define H2P_LAUNCH_(E, OL) hipLaunchKernelGGL((gemm_h2p_kernel<128, BN, E, OL>), dim3(tiles), dim3(512), 0, stream, a_lines, a.planes, a.C, a.bias, a.resid, sh)
    if (out_lines) {
        if (a.epilogue != EPI_GELU) { set_error("gemm_h2p: line output exists for the GELU epilogue only"); return R4D_ERR_INVALID; }
        H2P_LAUNCH_(EPI_GELU, true);
    } else {
#define H2P_LAUNCH_ROWMAJOR_(E) H2P_LAUNCH_(E, false)
#define H2P_KINDS(X, L) X(L, EPI_NONE) X(L, EPI_GELU) X(L, EPI_RESIDUAL) X(L, EPI_H2WORDS)
        R4D_EPI_DISPATCH(a.epilogue, H2P_KINDS, H2P_LAUNCH_ROWMAJOR_, set_error("gemm_h2p: epilogue %d has no instantiation", a.epilogue); return R4D_ERR_INVALID;)
#undef H2P_KINDS
#undef H2P_LAUNCH_ROWMAJOR_
    }
#undef H2P_LAUNCH_
    R4D_CHECK_LAUNCH("gemm_h2p");
    return R4D_OK;
}

// a.A is ignored: the A operand is `a_lines` ([M][K/32][2][32] fp16); out_lines: a.C receives [M][N/32][2][32] fp16 instead of fp32
int launch_gemm_h2p(const S3Args& a, const unsigned short* a_lines, bool out_lines, hipStream_t stream) {
    R4D_REQUIRE(a_lines && a.planes && a.C, "gemm_h2p: null pointer");
    R4D_REQUIRE(gemm_h2p_supported(a.M, a.K, a.N), "gemm_h2p: unsupported shape M=%d K=%d N=%d", a.M, a.K, a.N);
    R4D_REQUIRE(((uintptr_t)a_lines % 16) == 0 && ((uintptr_t)a.planes % 16) == 0, "gemm_h2p: alignment");
    R4D_REQUIRE(!out_lines || a.N % 32 == 0, "gemm_h2p: line output needs N %% 32 == 0 (N = %d)", a.N);
    R4D_REQUIRE(a.epilogue != EPI_RESIDUAL || a.resid, "gemm_h2p: the residual epilogue needs the second buffer");
    R4D_REQUIRE(!a.kblk || (a.epilogue == EPI_H2WORDS && a.N % 3 == 0 && a.kb_hd >= 32 && a.kb_hd % 32 == 0 && (a.N / 3) % a.kb_hd == 0),
                "gemm_h2p: the key-blocked K image goes with the h2-word epilogue, N = 3 d and a head_dim that is a multiple of 32");
    if (pick_tile_128(a.M, a.N)) { R4D_BRANCH(H2P_128x128); return launch_h2p<128>(a, a_lines, out_lines, PK_GEMM_H2_128x128, stream); }
    R4D_BRANCH(H2P_128x256);
    return launch_h2p<256>(a, a_lines, out_lines, PK_GEMM_H2_128x256, stream);
}

// Layer 0's c_attn over the listed row blocks (common.h: PadRowsPlan).  The grid holds the worst case, every block kept plus the
// table; the class records the flop of the launch it replaces (the host does not know how many blocks are listed: an upper bound)
int launch_gemm_h2p_rowmap(const S3Args& a, const unsigned short* a_lines, const PadRowsPlan& p, const PadRowsBuf& b, hipStream_t stream) {
    R4D_REQUIRE(a_lines && a.planes && a.C && a.kblk && b.hdr, "gemm_h2p rowmap: null pointer");
    R4D_REQUIRE(a.M == (int)p.rows() && gemm_h2p_supported(a.M, a.K, a.N) && a.N % 256 == 0 && (long long)a.M * a.ldc * 4 < (1ll << 31),
                "gemm_h2p rowmap: unsupported shape M=%d K=%d N=%d", a.M, a.K, a.N);
    R4D_REQUIRE(((uintptr_t)a_lines % 16) == 0 && ((uintptr_t)a.planes % 16) == 0, "gemm_h2p rowmap: alignment");
    R4D_REQUIRE(a.epilogue == EPI_H2WORDS && a.N % 3 == 0 && a.kb_hd >= 32 && a.kb_hd % 32 == 0 && (a.N / 3) % a.kb_hd == 0,
                "gemm_h2p rowmap: the h2-word c_attn with the key-blocked K image only");
    R4D_BRANCH(H2P_ROWMAP);
    ProfScope prof(PK_GEMM_H2_ROWMAP, 2.0 * (double)p.M * a.N * a.K, stream);
    H2PShape sh;
    sh.M = a.M; sh.N = a.N; sh.K = a.K; sh.ldc = a.ldc; sh.ldr = a.ldr;
    sh.kblk = a.kblk; sh.kb_hd = a.kb_hd;
    H2PRowMap rm;
    rm.hdr = b.hdr; rm.list = b.list; rm.m_real = p.M; rm.m_tab = p.Mp + p.Tmax;
    const int tiles_m = p.lmax / 4;
    if (pick_tile_128(p.lmax * 32, a.N))
        hipLaunchKernelGGL((gemm_h2p_rowmap_kernel<128, 128>), dim3(tiles_m * (a.N / 128)), dim3(512), 0, stream, a_lines, a.planes, a.C, a.bias, sh, rm);
    else
        hipLaunchKernelGGL((gemm_h2p_rowmap_kernel<128, 256>), dim3(tiles_m * (a.N / 256)), dim3(512), 0, stream, a_lines, a.planes, a.C, a.bias, sh, rm);
    R4D_CHECK_LAUNCH("gemm_h2p rowmap");
    return R4D_OK;
}

int launch_split2_lines(const float* x, long long rows, int K, unsigned short* lines, hipStream_t s) {
    R4D_REQUIRE(x && lines && rows >= 0 && K >= 32 && K % 32 == 0, "split2_lines: bad arguments (K %% 32 == 0 wanted)");
    R4D_REQUIRE((((uintptr_t)x | (uintptr_t)lines) & 15) == 0, "split2_lines: alignment");
    const long long n4 = rows * K / 4;
    if (n4 == 0) return R4D_OK;
    hipLaunchKernelGGL(split2_lines_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, x, n4, reinterpret_cast<uint2*>(lines), K);
    R4D_CHECK_LAUNCH("split2_lines");
    return R4D_OK;
}

}  // namespace r4d

using namespace r4d;

extern "C" {

int r4d_set_gemm_h2p(int32_t on) {
    const int prev = g_gemm_h2p;
    g_gemm_h2p = on != 0;
    return prev;
}

int r4d_split2_lines_f16(const float* x_d, int64_t rows, int32_t K, uint16_t* lines_d, void* stream) {
    return launch_split2_lines(x_d, rows, K, lines_d, (hipStream_t)stream);
}

int r4d_conv1d_h2p_f32(const uint16_t* x_lines_d, const uint16_t* planes_d, const float* bias_d, const float* residual_d, int32_t M,
                       int32_t K, int32_t N, int32_t epilogue, int32_t out_lines, void* y_d, void* stream) {
    R4D_REQUIRE(epilogue >= 0 && epilogue <= 2, "conv1d_h2p: epilogue %d not in {0,1,2}", epilogue);
    return launch_gemm_h2p(s3_args(nullptr, planes_d, bias_d, residual_d, M, K, N, epilogue, (float*)y_d), x_lines_d, out_lines != 0, (hipStream_t)stream);
}

}  // extern "C"
