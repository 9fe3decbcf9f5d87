// What attention_fused.hip and attention_h2.hip share; attention_b1.hip takes the group table, the 1-D work mapping (at 128-query
// tiles) and the grid from here and writes its own K / V descriptors beside ATTN_KV_RSRC (whose byte ranges are 4-byte elements).
//
// Device part: TEXT, not functions.  The pieces below are macros over the including kernel's own locals, in the idiom of
// gemm_epilogue_rowmajor.h / gemm_tn_tail.h: written as a __forceinline__ function that fills a small struct, the 1-D work mapping
// alone changed every kernel of attention_h2.hip (2,900 differing assembly lines in attn_h2ks_kernel<96, *>); as macros every
// kernel's assembly is what its own copy gave (tools/isa_equal.py, DESIGN_LOG 12.21).  Each macro names the locals it reads and the
// ones it declares.  (Comments inside a macro are /* */: a // comment would swallow the line continuation.)
//
// NOT shared: the key index of accumulator register r, `key0 + (r & 3) + 8 * (r >> 2) + 4 * lh`, stays written out at its ten
// uses (six as a key, four as a column of the output transpose).  As a function it changes the kernels; as a macro it only leaves them alone WITHOUT outer parentheses (with them
// `key0 + (...)` re-associates the integer sum) -- and an unparenthesised macro is worse than the repetition.
//
// Host part: plain functions (the group table of a launch, the 1-D grid, the exp2-domain logit scale).
#pragma once
#include <math.h>
#include "gemm_common.h"     // f32x2, f32x4, f32x16, u32x2, u32x4

namespace r4d {

// ------------------------------------------------------------------ device: shared text
// 1-D work mapping: all query tiles of one (sequence, head) run on the SAME XCD (workgroup ids are dealt round-robin to the 8 XCDs,
// each with its own L2), back to back, so K and V of that head are fetched from HBM once instead of once per query tile (measured
// before: 970 MB per launch against 290 MB of qkv + out, L2 hit rate 22 %, i.e. the kernel ran at the HBM limit).  Long (late)
// query tiles go first.  Declares qt, h, seq, gi, T, q0 and rowb (the first token row of the sequence); workgroups past the last
// pair or past their sequence's end return.  (attn_fused_kernel's 3-D grid is a different mapping and keeps its own text.)
// QT_: the queries of a tile -- 32 in the kernels of attention_fused.hip / attention_h2.hip, 128 in attention_b1.hip.
#define ATTN_TILE_1D(G_, H_, ntq_) ATTN_TILE_1D_Q(G_, H_, ntq_, 32)
#define ATTN_TILE_1D_Q(G_, H_, ntq_, QT_)                                                                           \
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;                                                         \
    const int pair = (slot / ntq_) * 8 + xcd;           /* (sequence, head) index */                                \
    if (pair >= G_.seq_prefix[G_.n] * H_) return;                                                                   \
    const int qt = ntq_ - 1 - slot % ntq_, h = pair % H_, seq = pair / H_;                                          \
    int gi = 0;                                                                                                     \
    while (gi + 1 < G_.n && seq >= G_.seq_prefix[gi + 1]) ++gi;                                                     \
    const int T = G_.T[gi];                                                                                         \
    const int q0 = qt * QT_;                                                                                        \
    if (q0 >= T) return;                                /* ntq covers the longest batch */                          \
    const long long rowb = G_.row0[gi] + (long long)(seq - G_.seq_prefix[gi]) * T;

// K / V of one head of the sequence as buffer descriptors (rows past the sequence are answered with zeros by the range check: no
// clamps, no 64-bit address arithmetic).  Reads rowb, h, T, d, HD; declares ld3, base (the head's Q columns of row rowb), seq_bytes,
// roff, kbase, kbytes, k_rsrc, v_rsrc.  K row-major: this head's K columns of the sequence's rows.  KBLK_ (a constant): K from the
// key-blocked image kblk_ instead -- from the 32-row block that holds the sequence's first row (which may start mid-block: roff) to
// the end of the block that holds its last one; block = 32 rows x d words, this head's chunks start h * HD / 8 KB into a block.
// All byte offsets are 32-bit: attn_groups_fill refuses the shapes at which they would wrap.
#define ATTN_KV_RSRC(ELEM_, qkv_, KBLK_, kblk_)                                                                     \
    const int ld3 = 3 * d;                                                                                          \
    const ELEM_* __restrict__ base = qkv_ + rowb * ld3 + (long long)h * HD;                                         \
    const int seq_bytes = ((T - 1) * ld3 + HD) * 4;    /* one head's K (or V) rows of this sequence, as a byte range */ \
    const int roff = (int)(rowb & 31);                                                                              \
    const ELEM_* kbase = KBLK_ ? kblk_ + (rowb >> 5) * (long long)(32 * d) + h * (HD / 8) * 256 : base + d;         \
    const int kbytes = KBLK_ ? (((roff + T - 1) >> 5) + 1) * (d * 128) - h * (HD / 8) * 1024 : seq_bytes;           \
    const __amdgpu_buffer_rsrc_t k_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<ELEM_*>(kbase), 0, kbytes, 0x00020000); \
    const __amdgpu_buffer_rsrc_t v_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<ELEM_*>(base + 2 * d), 0, seq_bytes, 0x00020000);

// A lane's K load offset (bytes; the scalar offset adds tile and step) for the lane whose key of tile 0 is key_lane_ (an expression
// WITHOUT outer parentheses at the use: see the key index above).  Reads roff, ld3, d, lh, KBLK; declares gl (key-blocked: the key
// counted from row 0 of the sequence's first block), k_voff, K_STEP (bytes between a lane's consecutive K loads) and k_tile (bytes
// per key of tile advance).
#define ATTN_K_LANE_H2(key_lane_)                                                                                   \
    const int gl = roff + key_lane_;                                                                                \
    const int k_voff = KBLK ? (gl >> 5) * (d * 128) + (lh * 32 + (gl & 31)) * 16 : ((key_lane_) * ld3 + 4 * lh) * 4; \
    constexpr int K_STEP = KBLK ? 1024 : 32;                                                                        \
    const int k_tile = KBLK ? d * 4 : ld3 * 4;

// Q tile -> LDS rows of LDQ elements: thread t stages row t/8, 16-byte pieces 4*(t%8) + 32j; rows past T repeat the last row (never
// stored).  All loads are issued before the first LDS write.  VEC_ = the 16-byte vector type.  Reads tid, q0, T, ld3, base, HD, LDQ.
#define ATTN_STAGE_Q(VEC_, Qs_)                                                                                     \
    {                                                                                                               \
        const int row = tid >> 3, seg = 4 * (tid & 7);                                                              \
        const auto* src = base + (long long)min(q0 + row, T - 1) * ld3 + seg;                                       \
        VEC_ qv[HD / 32];                                                                                           \
        _Pragma("unroll") for (int j = 0; j < HD / 32; ++j) qv[j] = *reinterpret_cast<const VEC_*>(src + 32 * j);   \
        _Pragma("unroll") for (int j = 0; j < HD / 32; ++j) *reinterpret_cast<VEC_*>(Qs_ + row * LDQ + seg + 32 * j) = qv[j]; \
    }

// Merge of the four key-split partial states (O_[NCB] of 16 registers, m_run, l_run per wave) through the float buffer lds_:
// (2,3) -> (0,1), then 1 -> 0.  Slot = NCB*16*64 O values + 64 m + 64 l floats.  The including file defines
// ATTN_MERGE_WEIGHT(m_old, m_new), the factor exp(m_old - m_new) in its softmax's domain.  Reads wid, lane, NCB; declares SLOT.
#define ATTN_MERGE4(O_, lds_)                                                                                       \
    constexpr int SLOT = NCB * 16 * 64 + 128;                                                                       \
    __syncthreads();                                    /* every wave is done with the query buffer */              \
    _Pragma("unroll 1") for (int step = 0; step < 2; ++step) {                                                      \
        const int writers_lo = step == 0 ? 2 : 1;       /* waves [writers_lo, 2*writers_lo) write, [0, writers_lo) merge */ \
        if (wid >= writers_lo && wid < 2 * writers_lo) {                                                            \
            float* sl = lds_ + (wid - writers_lo) * SLOT;                                                           \
            _Pragma("unroll") for (int c = 0; c < NCB; ++c)                                                         \
                _Pragma("unroll") for (int r = 0; r < 16; ++r) sl[(c * 16 + r) * 64 + lane] = O_[c][r];             \
            sl[NCB * 16 * 64 + lane] = m_run;                                                                       \
            sl[NCB * 16 * 64 + 64 + lane] = l_run;                                                                  \
        }                                                                                                           \
        __syncthreads();                                                                                            \
        if (wid < writers_lo) {                                                                                     \
            const float* sl = lds_ + wid * SLOT;                                                                    \
            const float m_b = sl[NCB * 16 * 64 + lane], l_b = sl[NCB * 16 * 64 + 64 + lane];                        \
            const float m_new = fmaxf(m_run, m_b);                                                                  \
            const float fa = (m_run == -INFINITY) ? 0.f : ATTN_MERGE_WEIGHT(m_run, m_new);                          \
            const float fb = (m_b == -INFINITY) ? 0.f : ATTN_MERGE_WEIGHT(m_b, m_new);                              \
            _Pragma("unroll") for (int c = 0; c < NCB; ++c)                                                         \
                _Pragma("unroll") for (int r = 0; r < 16; ++r) O_[c][r] = O_[c][r] * fa + sl[(c * 16 + r) * 64 + lane] * fb; \
            l_run = l_run * fa + l_b * fb;                                                                          \
            m_run = m_new;                                                                                          \
        }                                                                                                           \
        __syncthreads();                                                                                            \
    }

// The normalised output tile Os_[32][LDO] (LDS, fp32) -> rows of the merged-head layout out[rows][d], wave w the queries w, w + 4, ...
// Two fragments, because the tiles differ on purpose: the exact-f32 kernels write theirs transposed with an ODD stride
// (LDO = HD + 1: conflict-free) and read four scalars per lane; the f16x2 kernels keep 16-byte rows (LDO = HD + 4) for one
// ds_read_b128 per lane and piece.  Read wid, lane, q0, T, rowb, h, d, HD, LDO, out.
#define ATTN_STORE_ROWS_F32(Os_)                                                                                    \
    for (int q = wid; q < 32; q += 4) {                                                                             \
        if (q0 + q >= T) break;                                                                                     \
        float* dst = out + (rowb + q0 + q) * d + (long long)h * HD;                                                 \
        for (int c = lane * 4; c < HD; c += 256) {                                                                  \
            const float* sp = &Os_[q * LDO + c];                                                                    \
            *reinterpret_cast<float4*>(dst + c) = make_float4(sp[0], sp[1], sp[2], sp[3]);                          \
        }                                                                                                           \
    }
// out_lines (also read): the merged-head row as f16x2 LINES instead (gemm_h2p.hip: attn.c_proj stages them by LDS-DMA): the lane's
// four values are four consecutive k of one 128-byte line -- 8 bytes of its hi half, 8 of its lo' half; same bytes as fp32
#define ATTN_STORE_ROWS_H2(Os_)                                                                                     \
    for (int q = wid; q < 32; q += 4) {                                                                             \
        if (q0 + q >= T) break;                                                                                     \
        float* dst = out + (rowb + q0 + q) * d + (long long)h * HD;                                                 \
        for (int c = lane * 4; c < HD; c += 256) {                                                                  \
            const float4 o4 = *reinterpret_cast<const float4*>(&Os_[q * LDO + c]);                                  \
            if (out_lines) {                                                                                        \
                unsigned h0, l0, h1, l1;                                                                            \
                split2_pair<true>(o4.x, o4.y, h0, l0);                                                              \
                split2_pair<true>(o4.z, o4.w, h1, l1);                                                              \
                const int col = h * HD + c;                                                                         \
                unsigned char* ld = reinterpret_cast<unsigned char*>(out) + (rowb + q0 + q) * (long long)d * 4 + (col >> 5) * 128 + (col & 31) * 2; \
                *reinterpret_cast<uint2*>(ld) = make_uint2(h0, h1);                                                 \
                *reinterpret_cast<uint2*>(ld + 64) = make_uint2(l0, l1);                                            \
            } else {                                                                                                \
                *reinterpret_cast<float4*>(dst + c) = o4;                                                           \
            }                                                                                                       \
        }                                                                                                           \
    }

// ------------------------------------------------------------------ host
// The group table of one launch: n <= ATT_MAXG batches, batch g = Bs[g] sequences of Ts[g] tokens from token row row0s[g]; Tmax and
// the algorithmic flop count (causal half of Q.K^T and P.V: 2 * T^2 * hd per head).  `prefix` starts the error texts.
// Every kernel with the 1-D mapping forms 32-bit BYTE offsets inside a sequence (seq_bytes, k_voff, v_voff + the scalar row
// offset): T * 3d < 2^29 keeps them from wrapping.
static inline int attn_groups_fill(const char* prefix, int n, const int* Bs, const int* Ts, const long long* row0s, int H, int d,
                                   AttnGroups& G, int& Tmax, double& flop) {
    R4D_REQUIRE(n >= 1 && n <= ATT_MAXG, "%s: %d batches per launch (max %d)", prefix, n, ATT_MAXG);
    const int hd = d / H;
    G.n = n;
    G.seq_prefix[0] = 0;
    Tmax = 0;
    flop = 0.0;
    for (int g = 0; g < n; ++g) {
        R4D_REQUIRE((long long)Ts[g] * 3 * d < (1ll << 29), "%s: batch %d: B=%d T=%d", prefix, g, Bs[g], Ts[g]);
        G.seq_prefix[g + 1] = G.seq_prefix[g] + Bs[g];
        G.T[g] = Ts[g];
        G.row0[g] = row0s[g];
        if (Ts[g] > Tmax) Tmax = Ts[g];
        flop += 2.0 * Bs[g] * H * (double)Ts[g] * Ts[g] * hd;
    }
    for (int g = n; g < ATT_MAXG; ++g) { G.seq_prefix[g + 1] = G.seq_prefix[n]; G.T[g] = 0; G.row0[g] = 0; }
    R4D_REQUIRE(G.seq_prefix[n] <= 65535, "%s: %d sequences per launch exceed the grid limit", prefix, G.seq_prefix[n]);
    return R4D_OK;
}

// Workgroups of the 1-D mapping (ATTN_TILE_1D): the (sequence, head) pairs rounded up to the 8 XCDs, times ntq = query tiles of
// the longest batch (tiles of `qtile` queries).
static inline int attn_grid_1d(const char* prefix, const AttnGroups& G, int H, int Tmax, int& ntq, unsigned& grid, int qtile = 32) {
    ntq = cdiv(Tmax, qtile);
    const long long pairs8 = ((long long)G.seq_prefix[G.n] * H + 7) / 8;
    R4D_REQUIRE(pairs8 * 8 * ntq < (1ll << 31), "%s: grid too large", prefix);
    grid = (unsigned)(pairs8 * 8 * ntq);
    return R4D_OK;
}

// log2(e) / sqrt(hd) of the exp2-domain softmax on raw dot products, times the square of the operands' pre-scale (h2 words hold
// value / 4: both pre-scales are undone in the logits)
static inline float attn_qscale(int hd, double prescale) {
    return (float)(prescale * prescale * 1.4426950408889634 / sqrt((double)hd));
}

}  // namespace r4d
