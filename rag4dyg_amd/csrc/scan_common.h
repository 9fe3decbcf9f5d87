// The pieces that the three forms of the pool scan of score.hip share (pool_scan_ks_kernel, pool_scan_dma_kernel,
// pool_scan_ring_kernel): the forms must give the same bits (shard merge == one GPU, query batching changes nothing), so the
// split, the MFMA step, the cross-wave reduction and the score store exist ONCE, here.
//
// Most pieces are statement macros, not functions: as a __forceinline__ function template already the score store changed
// address arithmetic and register assignment in 49 of the 51 sections of score.hip's assembly, as text the kernels are what their
// own copies gave (tools/isa_equal.py; DESIGN_LOG 12.22).  They use the names every scan kernel has in scope:
//     constants KW, NG, R (= 16 / KW), D (= 32 KW NG);   the kernel arguments qhat, pool, Q, N, scores, zero_d, nzero;
//     after SCAN_PROLOGUE: tid, lane, w, li, lh, q0.
// A .h so that build.py's dependency scan sees it; score.hip is the only includer.
#pragma once
#include "bf16x3.h"               // split3_pair: the split of the bf16x3 GEMMs, here per lane

#ifndef SCAN_DBG
#define SCAN_DBG 0   // tuning aid (tools/kc_ablate.sh score.hip SCAN_DBG n): bit 0 (1) skips the MFMAs (and the split), bit 1 (2) the score stores, bit 3 (8) writes s_memrealtime stamps (100 MHz) of workgroup and wavefront phases over the score rows of queries >= 16 (tools/scan_timeline.py), bit 4 (16) skips the bf16x3 split arithmetic only
#endif
#if SCAN_DBG & ~(1 | 2 | 8 | 16)
#error "SCAN_DBG: bits 1, 2, 8 and 16 only"
#endif

namespace r4d {

// ------------------------------------------------------------------------------------ SCAN_DBG hooks (all empty in the product build)
constexpr bool SCAN_NO_MFMA = (SCAN_DBG & 1) != 0;      // (the step sums its operand instead: the loads stay alive)
constexpr bool SCAN_NO_STORES = (SCAN_DBG & 2) != 0;
constexpr bool SCAN_NO_SPLIT = (SCAN_DBG & 16) != 0;    // (the raw words stand in for the bf16 planes)
#if SCAN_DBG & 8
// stamps: 16 slots per workgroup, then 8 per wavefront, over the score rows of queries >= 16 (which are then not stored); slots:
// workgroup 0 start, 1 loads issued, 2 first tile landed, 3 end, 4 XCC id, 5 / 6 s_memtime at start / end, 7 stores issued,
// 8 + 4 t / 9 + 4 t MFMAs / reduction of tile t done, 10 grid size; wavefront 0 start, 1 loads issued, 2 queries landed, 3 queries
// split, 4 / 5 MFMAs of tile 0 / 1 done, 6 barrier passed, 7 stores issued (tools/scan_timeline.py reads this layout)
#define SCAN_STAMPS 1
#define SCAN_STAMP_DECL() \
    unsigned long long* stamps = reinterpret_cast<unsigned long long*>(scores + (long long)16 * N) + blockIdx.x * 16; \
    unsigned long long* wst = reinterpret_cast<unsigned long long*>(scores + (long long)16 * N) + gridDim.x * 16 + (blockIdx.x * KW + w) * 8; \
    if (tid == 0) { stamps[0] = __builtin_amdgcn_s_memrealtime(); stamps[5] = __builtin_amdgcn_s_memtime(); stamps[10] = gridDim.x; } \
    if (lane == 0) wst[0] = __builtin_amdgcn_s_memrealtime()
#define SCAN_STAMP(slot) do { if (tid == 0) stamps[slot] = __builtin_amdgcn_s_memrealtime(); } while (0)        // per workgroup
#define SCAN_WSTAMP(slot) do { if (lane == 0) wst[slot] = __builtin_amdgcn_s_memrealtime(); } while (0)          // per wavefront
#define SCAN_STAMP_COPY(dst, src) do { if (tid == 0) stamps[dst] = stamps[src]; } while (0)                      // a phase this form does not have
#define SCAN_KEEP(v) asm volatile("" :: "v"(v))                                                                 // a stamp behind it waits for v
#define SCAN_STAMP_END() do { SCAN_STAMP(7); SCAN_WSTAMP(7); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); \
    if (tid == 0) { stamps[3] = __builtin_amdgcn_s_memrealtime(); stamps[6] = __builtin_amdgcn_s_memtime(); stamps[4] = (unsigned long long)__builtin_amdgcn_s_getreg(6164); } } while (0)
#else
#define SCAN_STAMPS 0
#define SCAN_STAMP_DECL() do { } while (0)
#define SCAN_STAMP(slot) do { } while (0)
#define SCAN_WSTAMP(slot) do { } while (0)
#define SCAN_STAMP_COPY(dst, src) do { } while (0)
#define SCAN_KEEP(v) do { } while (0)
#define SCAN_STAMP_END() do { } while (0)
#endif

// ------------------------------------------------------------------------------------ prologue
// thread indices (lane (li, lh) = row li of a tile, half lh of its 32-byte sector), the query block, and the ticket counters of
// the top-k launch that follows on this stream
#define SCAN_PROLOGUE() \
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6; \
    const int li = lane & 31, lh = lane >> 5; \
    const int q0 = blockIdx.y * 32; \
    if (blockIdx.x == 0 && blockIdx.y == 0) \
        for (int i = tid; i < nzero; i += 64 * KW) zero_d[i] = 0u

// ------------------------------------------------------------------------------------ split and MFMA step
// a lane's 8 k of one bf16 MFMA step (two 16-byte pieces) -> three bf16x8 operands
__device__ __forceinline__ void scan_split8(const float4& a, const float4& b, u32x4& h, u32x4& m, u32x4& l) {
    unsigned hh[4], mm[4], ll[4];
    split3_pair(a.x, a.y, hh[0], mm[0], ll[0]); split3_pair(a.z, a.w, hh[1], mm[1], ll[1]);
    split3_pair(b.x, b.y, hh[2], mm[2], ll[2]); split3_pair(b.z, b.w, hh[3], mm[3], ll[3]);
    h = u32x4{hh[0], hh[1], hh[2], hh[3]}; m = u32x4{mm[0], mm[1], mm[2], mm[3]}; l = u32x4{ll[0], ll[1], ll[2], ll[3]};
}
// the query side of one 128-byte line group: F_ = the lane's four 16-byte pieces of its query row (wherever the kernel got them
// from), zeroed for rows at or past Q (OK_ false), then (S3_) split ONCE into Q3G_[step][plane]
#define SCAN_SPLIT_QUERIES(Q3G_, F_, OK_, S3_) do { \
    if (!(OK_)) { \
        _Pragma("unroll") \
        for (int u_ = 0; u_ < 4; ++u_) { (F_)[u_].x = 0.f; (F_)[u_].y = 0.f; (F_)[u_].z = 0.f; (F_)[u_].w = 0.f; } \
    } \
    if constexpr (S3_) { \
        scan_split8((F_)[0], (F_)[1], (Q3G_)[0][0], (Q3G_)[0][1], (Q3G_)[0][2]); \
        scan_split8((F_)[2], (F_)[3], (Q3G_)[1][0], (Q3G_)[1][1], (Q3G_)[1][2]); \
    } } while (0)
// the six products of one 16-k step, smallest terms first: lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi (gemm_s3.hip)
#define SCAN_MFMA16(A_, B_, ACC_) ACC_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A_), __builtin_bit_cast(bf16x8, B_), ACC_, 0, 0, 0)
#define SCAN_STEP6(ACC_, Q_, BH_, BM_, BL_) do { SCAN_MFMA16(Q_[2], BH_, ACC_); SCAN_MFMA16(Q_[0], BL_, ACC_); SCAN_MFMA16(Q_[1], BM_, ACC_); \
    SCAN_MFMA16(Q_[1], BH_, ACC_); SCAN_MFMA16(Q_[0], BM_, ACC_); SCAN_MFMA16(Q_[0], BH_, ACC_); } while (0)

// ------------------------------------------------------------------------------------ pinning (sched_group_barrier: 0x008 MFMA, 0x002 VALU)
// The split of a step's pool operand (36 VALU instructions) is issued INSIDE the six MFMAs of the step before it, six per MFMA
// gap: left to the compiler the stream is split, split, ..., MFMA x 6, and two wavefronts of a SIMD fall into lock step -- both
// splitting, then both multiplying -- so that the vector ALU and the matrix pipe take turns (timeline: 4,600 cycles per tile and
// SIMD = 48 x 32 + 704 x 4.2).  Placed behind the SCAN_STEP6 whose gaps take the split written in front of it.
#define SCAN_PIN_SPLIT_IN_STEP() do { \
    _Pragma("unroll") \
    for (int j_ = 0; j_ < 6; ++j_) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 6, 0); } } while (0)
// the LDS-DMA forms, second step of a piece: the next piece's fragments are still on their way from LDS: two MFMAs first, then
// the split in the gaps
#define SCAN_PIN_SPLIT_BEHIND_LDS_READ() do { \
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); \
    _Pragma("unroll") \
    for (int j_ = 0; j_ < 4; ++j_) { __builtin_amdgcn_sched_group_barrier(0x002, 9, 0); __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); } } while (0)

// ------------------------------------------------------------------------------------ cross-wave reduction and store
// The KW partial 32 x 32 tiles of a pool tile meet in LDS as BASE_[src wave][dst wave][lane][R] (SCAN_RED_TILE floats):
// lane-contiguous vectors, conflict-free on both sides.  Every wave writes its accumulator, the CALLER puts its barrier, then
// wave w sums registers [w R, (w + 1) R) of the KW partial tiles in a FIXED order: deterministic, and the same in every form.
#define SCAN_RED_TILE (KW * KW * 64 * R)
#define SCAN_RED_WRITE(BASE_, ACC_) do { \
    _Pragma("unroll") \
    for (int wd_ = 0; wd_ < KW; ++wd_) \
        _Pragma("unroll") \
        for (int i_ = 0; i_ < R; ++i_) (BASE_)[((w * KW + wd_) * 64 + lane) * R + i_] = (ACC_)[wd_ * R + i_]; } while (0)
#define SCAN_RED_SUM(FIN_, BASE_) do { \
    _Pragma("unroll") \
    for (int i_ = 0; i_ < R; ++i_) (FIN_)[i_] = 0.f; \
    _Pragma("unroll") \
    for (int p_ = 0; p_ < KW; ++p_) \
        _Pragma("unroll") \
        for (int i_ = 0; i_ < R; ++i_) (FIN_)[i_] += (BASE_)[((p_ * KW + w) * 64 + lane) * R + i_]; } while (0)
// one finished row of scores: FIN_[i] is accumulator register r = w R + i of pool row ROW_, i.e. (C/D layout of the 32 x 32 MFMA)
// query q0 + (r & 3) + 8 (r >> 2) + 4 lh; (x + 1) / 2 is train_retriever.py:438.  ROW_OK_: the row is this workgroup's to store
// (rows past its share were computed on clamped loads).
#define SCAN_STORE_ROW(FIN_, ROW_, ROW_OK_) do { \
    if (ROW_OK_) { \
        _Pragma("unroll") \
        for (int i_ = 0; i_ < R; ++i_) { \
            const int r_ = w * R + i_; \
            const int q_ = q0 + (r_ & 3) + 8 * (r_ >> 2) + 4 * lh; \
            if (q_ < Q && !SCAN_NO_STORES && (!SCAN_STAMPS || q_ < 16)) scores[(long long)q_ * N + (ROW_)] = ((FIN_)[i_] + 1.0f) / 2.0f; \
        } \
    } } while (0)

// ------------------------------------------------------------------------------------ LDS-DMA staging (pool_scan_dma_kernel, pool_scan_ring_kernel)
// A "piece" = 32 rows x one 128-byte line = 4 KB = four DMA instructions of 1 KB (global_load_lds_dwordx4: lane l of instruction i
// copies 16 bytes of row 8 i + l / 8, no VGPRs), into a ring of P slots per wavefront; it comes back as ds_read_b128 fragments.
// LDS image: row r's 16-byte chunk c sits at slot c ^ ((r >> 1) & 7) of its 128 bytes -- written by permuting the SOURCE chunk per
// lane (the DMA destination is lane-linear), read with the same XOR: both sides conflict-free.
// global address = base + 32-bit lane offset + i KB, LDS address = M0 + i KB + 16 lane (the instruction offset moves BOTH sides,
// so the lane offsets of instruction i are built i KB short); M0 is written in the statement that uses it and restored (the
// compiler owns it)
__device__ __forceinline__ void scan_glds_piece(const void* base, unsigned v0, unsigned v1, unsigned v2, unsigned v3, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %6\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %5\n\t"
                 "global_load_lds_dwordx4 %2, %5 offset:1024\n\t"
                 "global_load_lds_dwordx4 %3, %5 offset:2048\n\t"
                 "global_load_lds_dwordx4 %4, %5 offset:3072\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(v0), "v"(v1), "v"(v2), "v"(v3), "s"(base), "s"(lds_dst) : "memory");
}
// the wavefront's ring (scan_lds and P in scope: P slots of 4 KB) and the lane's part of every piece: instruction i copies rows
// 8 i + lrow of the piece, lane % 8 picking the (permuted) chunk c0 ^ 4 (i & 1)  [= (lane & 7) ^ ((row >> 1) & 7)]
#define SCAN_DMA_RING() \
    unsigned char* ring = scan_lds + w * (P * 4096); \
    const unsigned ring_lds = __builtin_amdgcn_readfirstlane((unsigned)(size_t)ring); \
    const int c0 = (lane & 7) ^ (lane >> 4), lrow = lane >> 3
// instruction I_'s byte offset inside a row, counted from (pointer - 3 KB) and built I_ KB short (scan_glds_piece), and with it
// (IN_ROW_) the lane's source offset in a piece whose 32 rows start at FIRST_; rows past CLAMP_ (the last row of the share / the
// shard / the query block) are clamped to it: cache hits, always valid.  (Two macros: each kernel keeps the statement order
// it had -- the DMA form one loop over i, the ring form its in_row[] first -- which the instruction schedule follows.)
#define SCAN_DMA_IN_ROW(I_) (128u * w + 16u * (c0 ^ (4 * ((I_) & 1))) + 3072u - 1024u * (I_))
#define SCAN_DMA_OFFSET(IN_ROW_, I_, FIRST_, CLAMP_) ((unsigned)min((FIRST_) + 8 * (I_) + lrow, (CLAMP_)) * (unsigned)(D * 4) + (IN_ROW_))
// the bases those offsets count from, and fsw = the XOR of the lane's fragment reads
#define SCAN_DMA_BASES() \
    const char* qbase = reinterpret_cast<const char*>(qhat) - 3072; \
    const char* pbase = reinterpret_cast<const char*>(pool) - 3072; \
    const int fsw = (li >> 1) & 7
// issue: line group G_ of the rows V_ addresses (BASE_ = qbase or pbase) -> ring slot SLOT_
#define SCAN_DMA_ISSUE(BASE_, G_, V_, SLOT_) scan_glds_piece((BASE_) + 128 * KW * (G_), (V_)[0], (V_)[1], (V_)[2], (V_)[3], ring_lds + (SLOT_) * 4096)
// fragments: lane (row li, half lh) reads chunks lh, 2 + lh, 4 + lh, 6 + lh of its row of slot SLOT_
#define SCAN_DMA_READ(F_, SLOT_) do { \
    const float4* base_ = reinterpret_cast<const float4*>(ring + (SLOT_) * 4096 + li * 128); \
    _Pragma("unroll") \
    for (int u_ = 0; u_ < 4; ++u_) (F_)[u_] = base_[(2 * u_ + lh) ^ fsw]; } while (0)
// counted wait: a wavefront reads back only what it copied itself, so its own s_waitcnt vmcnt orders the DMA in front of the
// ds_read; n = DMA instructions (four per piece) that may stay outstanding BEHIND the piece waited for
template <int N_> __device__ __forceinline__ void scan_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N_) : "memory"); }
__device__ __forceinline__ void scan_wait_vmcnt(int n) {                                   // n: 0, 4, 8, or 12 and more
    if (n >= 12) scan_wait_vm<12>(); else if (n == 8) scan_wait_vm<8>(); else if (n == 4) scan_wait_vm<4>(); else scan_wait_vm<0>();
}

}  // namespace r4d
