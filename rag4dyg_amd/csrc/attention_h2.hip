// Fused causal multi-head attention on the fp16 matrix cores at fp32 accuracy (the f16x2 form of gemm_h2.hip) for head_dim
// 128 / 256 (attn_h2_kernel) and 32 / 64 / 96 (attn_h2ks_kernel, further down): softmax(Q.K^T / sqrt(hd), causal) . V  (Attention._attn + split/merge_heads, models/modeling_gpt2.py:140-175).
//
// Operands arrive as "h2 words" (csrc/h2.h): qkv [rows, 3d] uint32, every element  hi | lo' << 16  of value / 4 -- written by
// the c_attn GEMM's EPI_H2WORDS epilogue (gemm_h2.hip), so neither K nor V is converted here: a register of words IS an MFMA
// operand holding two k-slots (hi, lo') per element, and against it the other operand takes the two forms
//     F1 = (hi, 0)  -> sum hi.hi  (accumulator set 0)        F2 = (lo', hi)  -> sum hi.lo' + lo'.hi  (set 1, factor 2^11)
// i.e. TWO v_mfma_f32_32x32x16_f16 per 8 elements (the plane form of gemm_h2.hip needs three per 16, but would need K and V
// re-laid by whoever produces them) against sixteen v_mfma_f32_32x32x2_f32 in attention_fused.hip: the matrix work per
// (query, key) pair drops 4 x for Q.K^T and 8 x for P.V.  The dropped term 2^-22 lo'.lo' and the roundings are gemm_h2.hip's.
//
// Structure = attention_fused.hip's column-split kernel: one workgroup = one (sequence, head, 32-query tile); its 4 wavefronts
// walk 128-key super-tiles together -- wave w computes S^T = K.Q^T for its own 32 keys over the full head_dim (A = its K rows
// straight from global memory, 16 bytes = 4 words per lane and step; B = the Q tile from LDS, its two forms derived in
// registers: one AND and one rotate per word), the row max / row sum are combined across the waves through LDS, every wave
// publishes its probabilities to LDS as h2 words too (one image: with both forms stored the head_dim-256 workgroup needs 68 KB
// and only two fit a CU; 51 KB and 168 VGPRs give three, head_dim 128 four -- worth 5 % / 12 %), and wave w accumulates its
// quarter of the head columns of O^T over all 128 keys (A = V words, four 4-byte loads per tile column group; B = the two
// forms of the P words, derived like Q's, one ds_read_b128 per 8 keys).
// Logits: S = (acc0 + 2^-11 acc1) * 16 log2(e) / sqrt(hd)  (the 16 undoes the two 2^-2 pre-scales), exp2 domain, fp32 online
// softmax exactly as in attention_fused.hip; masked keys are skipped.
// Range: |q|, |k|, |v| < 2^18 (beyond: inf -> NaN in the output, never a quiet wrong number).
#include <math.h>
#include "attention_common.h"
#include "h2.h"

#ifndef ATH_DBG
#define ATH_DBG 0   // tuning aid (tools/kc_ablate.sh attention_h2.hip ATH_DBG n), attn_h2_kernel: bit 0 one Q.K^T step only, bit 1 one P.V group only, bit 2 no softmax barriers, bit 3 no K refills, bit 4 no V refills
#endif

namespace r4d {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// attn_h2_kernel's pipeline depths and the occupancies it is compiled for
constexpr int ATH_KD = 4;       // K loads (16 bytes per lane) in flight per wave (8 / 16: no faster, and the registers cost a workgroup per CU)
constexpr int ATH_VD = 3;       // V key-groups (8 keys) in flight per wave
constexpr int ATH_QP = 2;       // Q fragments (one ds_read_b128 each) in flight per wave
constexpr int ATH_OCC256 = 3;   // workgroups per CU the head_dim-256 instantiation is compiled for (168 VGPRs, 51 KB of LDS)
constexpr int ATH_OCC128 = 4;   // workgroups per CU the head_dim-128 instantiation is compiled for (128 VGPRs, 35 KB of LDS)

__global__ __launch_bounds__(256) void pack_h2_words_kernel(const float* __restrict__ x, long long n, unsigned* __restrict__ w) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 2;
    if (i >= n) return;
    unsigned w0, w1;
    h2_words<true>(x[i], i + 1 < n ? x[i + 1] : 0.f, w0, w1);
    w[i] = w0;
    if (i + 1 < n) w[i + 1] = w1;
}

#define ATH_MFMA(A_, B_, C_) __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A_), __builtin_bit_cast(f16x8, B_), C_, 0, 0, 0)

// KBLK: the K words come from the KEY-BLOCKED image `kblk` that the c_attn epilogue writes beside qkv (gemm_h2p.hip, EPI_H2WORDS with
// kb_hd set) instead of from the K columns of qkv: for every 32 consecutive token ROWS (global row index, blocks of 32), head and
// 8-element step u one contiguous 1 KB chunk [half h][row & 31][4 words] -- exactly the 64 x 16 bytes one K load instruction of a
// wavefront fetches.  Row-major K costs that instruction 32 cache lines (each lane its own key row, 32 bytes of each line used);
// blocked it is 8-10 whole lines.  PMC on the row-major form (round 5): TA busy 71 %, 14.5 tag lookups per load instruction, L1 hit
// rate 75 % = every line fetched once and looked up four times; with whole lines the head_dim-256 launch takes a third less.
template <int HD, bool KBLK>
__global__ __launch_bounds__(256, HD >= 256 ? ATH_OCC256 : ATH_OCC128) void attn_h2_kernel(const unsigned* __restrict__ qkv, const unsigned* __restrict__ kblk,
                                                                                  const AttnGroups G, int d, int H,
                                                                                  int ntq, float qscale, float* __restrict__ out, int out_lines) {
    constexpr int CW = HD / 4;                         // head columns owned by one wave
    constexpr int VW = CW / 32;                        // O^T tiles per wave (1 or 2): tile j = columns wid * CW + 32 j + lane
    constexpr int NSTEP = HD / 8;                      // 16-byte K loads (and Q reads) per key row: 8 elements per MFMA pair
    constexpr int LDQ = HD + 4, LDP = 132;             // row strides (words): 16-lane b128 groups hit 16 distinct slots
    constexpr int KD = NSTEP < ATH_KD ? NSTEP : ATH_KD;   // K loads in flight per lane
    constexpr int VD = ATH_VD;                         // V key-groups (8 keys) in flight
    constexpr int QP = ATH_QP;                         // Q fragments (ds_read_b128) in flight: a fragment feeds TWO 32-cycle MFMAs
    extern __shared__ unsigned ldsw[];                 //   (sixteen 64-cycle ones in attention_fused.hip), so the LDS latency shows unless the reads run ahead
    unsigned* Qs = ldsw;                               // [32][LDQ]  the query tile's words
    unsigned* Ps = ldsw + 32 * LDQ;                    // [32][LDP]  probabilities of the current super-tile as h2 words, [query][key]
    float* red = reinterpret_cast<float*>(Ps + 32 * LDP);   // [2][4][32] per-wave row max / row sum
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    ATTN_TILE_1D(G, H, ntq)                           // XCD-aware (sequence, head, query tile) -> qt, h, seq, T, q0, rowb
    ATTN_KV_RSRC(unsigned, qkv, KBLK, kblk)            // ld3, base, seq_bytes, roff, k_rsrc (row-major or key-blocked), v_rsrc
    const int qidx = q0 + li;
    const int key_limit = min(T, q0 + 32);             // keys >= key_limit are masked for every query of the tile
    ATTN_K_LANE_H2(32 * wid + li)                      // gl, k_voff, K_STEP, k_tile; + scalar (super-tile, step)
    // (V: measured and taken out -- one 16-byte load per lane (key 4lh + (li & 3) x four columns: eight whole lines per instruction
    //  instead of four 4-byte loads of two lines each) followed by a 4 x 4 transpose inside the quad, 16 DPP / select instructions per
    //  column tile: head_dim 256 102 -> 119 us, head_dim 128 218 -> 208 us at B 128, T 277 / 300: the VALU work costs more than the
    //  vector-memory path gains)
    const int v_voff = (4 * lh * ld3 + wid * CW + li) * 4;                   // bytes; + scalar ((st0 + 8s + c) * ld3 + 32 j) * 4
    u32x4 kb[KD];
    if (wid * 32 < key_limit) {
#pragma unroll
        for (int u = 0; u < KD; ++u) kb[u] = __builtin_amdgcn_raw_buffer_load_b128(k_rsrc, k_voff, K_STEP * u, 0);
    }
    ATTN_STAGE_Q(u32x4, Qs)
    __syncthreads();

    f32x16 O0[VW], O1[VW];
#pragma unroll
    for (int c = 0; c < VW; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) { O0[c][r] = 0.f; O1[c][r] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;
    const unsigned* q_frag = Qs + li * LDQ + 4 * lh;
    const unsigned* p_frag = Ps + li * LDP + 4 * lh;

    for (int st0 = 0; st0 < key_limit; st0 += 128) {
        const int key0 = st0 + wid * 32;
        const bool active = key0 < key_limit;           // wave-uniform
        f32x16 S;
        float mt = -INFINITY;
        if (active) {
            f32x16 S0, S1;
#pragma unroll
            for (int r = 0; r < 16; ++r) { S0[r] = 0.f; S1[r] = 0.f; }
            const int k_soff = st0 * k_tile;
            u32x4 qb[QP];
#pragma unroll
            for (int u = 0; u < QP; ++u) qb[u] = *reinterpret_cast<const u32x4*>(q_frag + 8 * u);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < ((ATH_DBG & 1) ? 1 : NSTEP); ++u) {
                const u32x4 kw = kb[u % KD];
                const u32x4 qw = qb[u % QP];
                u32x4 f1, f2;
#pragma unroll
                for (int e = 0; e < 4; ++e) { f1[e] = qw[e] & 0xffffu; f2[e] = __builtin_amdgcn_alignbit(qw[e], qw[e], 16); }
                S0 = ATH_MFMA(kw, f1, S0);
                S1 = ATH_MFMA(kw, f2, S1);
                if (u + QP < NSTEP) qb[u % QP] = *reinterpret_cast<const u32x4*>(q_frag + 8 * (u + QP));
                if (!(ATH_DBG & 8) && u + KD < NSTEP)  // refill AFTER the slot's MFMAs in program order: no register copies
                    kb[u % KD] = __builtin_amdgcn_raw_buffer_load_b128(k_rsrc, k_voff, k_soff + K_STEP * (u + KD), 0);
                // pinned: the step's eight VALU, its two MFMAs, then the Q read of step u + QP and the K load of step u + KD
                __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                if (u + QP < NSTEP) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                if (!(ATH_DBG & 8) && u + KD < NSTEP) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 16; ++r) S[r] = __builtin_fmaf(S1[r], H2_LO_UNSCALE, S0[r]);      // RAW (q/4).(k/4): scaled AFTER the max is subtracted
            if (key0 + 31 > q0) {                      // the sub-tile touches the diagonal (or runs past T): mask
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = key0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    S[r] = (key <= qidx) ? S[r] : -INFINITY;
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) mt = fmaxf(mt, S[r]);
            mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        }
        const int ngroups = (min(128, key_limit - st0) + 7) >> 3;      // 8-key groups of the P.V phase, wave-uniform
        const int v_soff = st0 * ld3 * 4;
        u32x4 vb[VD][VW];                              // vb[u][j][c] = V word of key 8 (s0 + u) + 4 lh + c, column tile j
#define ATH_VLOAD(U, SG)                                                                            \
    {                                                                                               \
        _Pragma("unroll") for (int c = 0; c < 4; ++c)                                               \
            _Pragma("unroll") for (int j = 0; j < VW; ++j)                                          \
                vb[U][j][c] = __builtin_amdgcn_raw_buffer_load_b32(v_rsrc, v_voff, v_soff + ((8 * (SG) + c) * ld3 + 32 * j) * 4, 0); \
    }
#pragma unroll
        for (int u = 0; u < VD; ++u) ATH_VLOAD(u, u)
        if (lh == 0) red[wid * 32 + li] = mt;
        if (!(ATH_DBG & 4)) __syncthreads();
        const float m_tile = fmaxf(fmaxf(red[li], red[32 + li]), fmaxf(red[64 + li], red[96 + li]));
        const float m_new = fmaxf(m_run, m_tile);      // finite from the first super-tile on (key 0 is never masked)
        // p = exp2((s - max) * qscale) on the raw dot products (round 5; attention_fused.hip has the reasoning): the difference of
        // nearby logits is exact, only a small number is rounded by the scale.  Same instruction count as scale-then-subtract.
        const float alpha = (m_run == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((m_run - m_new) * qscale);
        float ps = 0.f;
        if (active) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float p[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) p[e] = __builtin_amdgcn_exp2f((S[4 * g + e] - m_new) * qscale);
                ps += (p[0] + p[1]) + (p[2] + p[3]);
                unsigned a[4];
                h2_words<false>(p[0], p[1], a[0], a[1]);
                h2_words<false>(p[2], p[3], a[2], a[3]);
                const u32x4 w4 = {a[0], a[1], a[2], a[3]};
                *reinterpret_cast<u32x4*>(Ps + li * LDP + wid * 32 + 8 * g + 4 * lh) = w4;            // keys 8g + 4lh + 0..3
            }
            ps += __shfl_xor(ps, 32, 64);
        }
        if (lh == 0) red[128 + wid * 32 + li] = ps;
        if (!(ATH_DBG & 4)) __syncthreads();
        l_run = l_run * alpha + ((red[128 + li] + red[160 + li]) + (red[192 + li] + red[224 + li]));
        if (__any(alpha != 1.0f && m_run != -INFINITY)) {
#pragma unroll
            for (int c = 0; c < VW; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) { O0[c][r] *= alpha; O1[c][r] *= alpha; }
        }
        m_run = m_new;
        // ---- O^T[c][q] += sum over the valid keys of this super-tile of V[key][c] * P[q][key], 8 keys per group:
        // lane half lh handles keys 8s + 4lh + c (c = 0..3) -- the four words of its ds_read_b128 of each P form
        if (!(ATH_DBG & 8) && st0 + 128 + wid * 32 < key_limit) {         // this wave's K rows of the next super-tile
            const int kn_soff = (st0 + 128) * k_tile;
#pragma unroll
            for (int u = 0; u < KD; ++u) kb[u] = __builtin_amdgcn_raw_buffer_load_b128(k_rsrc, k_voff, kn_soff + K_STEP * u, 0);
        }
        // the P words of group s + 1 are read before the MFMAs of group s (a group is 2 VW MFMAs: 64-128 cycles, the LDS latency);
        // group 16 does not exist: its read stays inside the allocation (LDP = 132, then `red`) and is never used
        u32x4 pn = *reinterpret_cast<const u32x4*>(p_frag);
        for (int s0 = 0; s0 < ((ATH_DBG & 2) ? min(ngroups, 1) : ngroups); s0 += VD) {
#pragma unroll
            for (int u = 0; u < VD; ++u) {
                const int sg = s0 + u;
                if (sg < ngroups) {
                    u32x4 pf1, pf2;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { pf1[e] = pn[e] & 0xffffu; pf2[e] = __builtin_amdgcn_alignbit(pn[e], pn[e], 16); }
                    pn = *reinterpret_cast<const u32x4*>(p_frag + 8 * (sg + 1));
#pragma unroll
                    for (int j = 0; j < VW; ++j) {
                        O0[j] = ATH_MFMA(vb[u][j], pf1, O0[j]);
                        O1[j] = ATH_MFMA(vb[u][j], pf2, O1[j]);
                    }
                    if (!(ATH_DBG & 16)) ATH_VLOAD(u, sg + VD)             // refill behind the slot's MFMAs; past the range: zeros
                    __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 2 * VW, 0);
                    if (!(ATH_DBG & 16)) __builtin_amdgcn_sched_group_barrier(0x020, 4 * VW, 0);
                }
            }
        }
#undef ATH_VLOAD
    }
    // ---- join the two sets, normalise, transpose through LDS (re-using the Q / P buffers), coalesced row stores
    __syncthreads();
    constexpr int LDO = HD + 4;                         // (16-byte rows: one ds_read_b128 per lane and output piece)
    float* Os = reinterpret_cast<float*>(ldsw);
    {
        const float inv = H2_A_UNSCALE / l_run;
#pragma unroll
        for (int j = 0; j < VW; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = wid * CW + 32 * j + (r & 3) + 8 * (r >> 2) + 4 * lh;
                Os[li * LDO + c] = __builtin_fmaf(O1[j][r], H2_LO_UNSCALE, O0[j][r]) * inv;
            }
    }
    __syncthreads();
    ATTN_STORE_ROWS_H2(Os)
}

template <int HD, bool KBLK>
static int launch_ah2(const unsigned* qkv, const unsigned* kblk, const AttnGroups& G, int Tmax, double flop, int H, int d, float* out, int out_lines, hipStream_t s) {
    const size_t lds = ((size_t)32 * (HD + 4) + 32 * 132 + 256) * 4;       // >= the [32][HD+4] output tile
    if (lds > 64 * 1024) {
        static bool raised = false;                     // (one process drives one device: include/r4d.h, PROCESS MODEL)
        if (!raised) {
            if (hipFuncSetAttribute((const void*)attn_h2_kernel<HD, KBLK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
                set_error("attention_h2: cannot raise the dynamic LDS limit");
                return R4D_ERR_HIP;
            }
            raised = true;
        }
    }
    ProfScope prof(PK_ATTN_FUSED, flop, s);
    int ntq, rc;
    unsigned grid;
    if ((rc = attn_grid_1d("attention_h2", G, H, Tmax, ntq, grid))) return rc;
    hipLaunchKernelGGL((attn_h2_kernel<HD, KBLK>), dim3(grid), dim3(256), lds, s, qkv, kblk, G, d, H, ntq, attn_qscale(HD, H2_A_UNSCALE), out, out_lines);
    R4D_CHECK_LAUNCH("attn_h2");
    return R4D_OK;
}

// ---------------------------------------------------------------------------------------------- head_dim 32 / 64 / 96: key-split form
// (round 5; VERDICT r4 missing 2: SimpleDyG UCI_13 is head_dim 96, the reddit generator 64 -- they stayed on the exact-f32 kernels.)
// attention_fused.hip's key-split structure on h2 words: one workgroup = one (sequence, head, 32-query tile), wavefront w walks the
// 32-key tiles w, w + 4, ... ON ITS OWN with its own online softmax and its own O^T accumulators (no barrier in the loop), the four
// partial states merged at the end.  S^T = K.Q^T as in attn_h2_kernel (A = the wave's K rows straight from global memory, 4 words per
// lane and step; B = the Q tile's forms from the LDS word image).  What the small head dims allow: the probabilities never touch LDS
// -- in the S^T accumulator lane (q, lh) holds keys 8g + 4lh + {0..3} of every 8-key group g, which ARE the k-slots 8lh .. 8lh+7 that
// lane supplies to the P.V MFMA of that group: four exp2, two h2_words, the two forms by AND / rotate, straight into the operand.
template <int HD, bool KBLK>      // KBLK: K from the key-blocked image (attn_h2_kernel: whole cache lines per K load instruction)
__global__ __launch_bounds__(256, 2) void attn_h2ks_kernel(const unsigned* __restrict__ qkv, const unsigned* __restrict__ kblk, const AttnGroups G, int d, int H, int ntq,
                                                          float qscale, float* __restrict__ out, int out_lines) {
    constexpr int NCB = HD / 32;                       // 32-column blocks of O^T
    constexpr int NSTEP = HD / 8;                      // 16-byte K loads per key row (8 elements per MFMA pair)
    constexpr int LDQ = HD + 4;
    extern __shared__ unsigned ldsw[];                 // Q words [32][LDQ]; later 2 merge slots; later the O tile [32][HD+4]
    unsigned* Qs = ldsw;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    ATTN_TILE_1D(G, H, ntq)
    ATTN_KV_RSRC(unsigned, qkv, KBLK, kblk)            // (key-blocked: blocks of 32 GLOBAL rows; the sequence may start mid-block)
    const int qidx = q0 + li;
    ATTN_K_LANE_H2(li)                                 // gl, k_voff, K_STEP, k_tile; + scalar (tile, step)
    const int v_voff = (4 * lh * ld3 + li) * 4;                              // bytes; + scalar ((key0 + 8g + e) * ld3 + 32 j) * 4
    u32x4 kb[NSTEP];
    if (wid <= qt) {                                                         // this wave's first key tile
#pragma unroll
        for (int u = 0; u < NSTEP; ++u) kb[u] = __builtin_amdgcn_raw_buffer_load_b128(k_rsrc, k_voff, wid * 32 * k_tile + K_STEP * u, 0);
    }
    ATTN_STAGE_Q(u32x4, Qs)
    __syncthreads();

    f32x16 O0[NCB], O1[NCB];
#pragma unroll
    for (int c = 0; c < NCB; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) { O0[c][r] = 0.f; O1[c][r] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;
    const unsigned* q_frag = Qs + li * LDQ + 4 * lh;

    for (int kt = wid; kt <= qt; kt += 4) {
        const int key0 = kt * 32;
        // V words: groups 0 and 1 (16 keys) are requested before the Q.K^T MFMAs and land under them, groups 2 and 3 behind them (they
        // land under the softmax and the first P.V MFMAs): all four up front cost 16 NCB registers beside the K rows, S and O^T
        u32x4 vb[4][NCB];
#define ATK_VLOAD(g_)                                                                              \
        _Pragma("unroll") for (int j = 0; j < NCB; ++j) _Pragma("unroll") for (int e = 0; e < 4; ++e) \
            vb[g_][j][e] = __builtin_amdgcn_raw_buffer_load_b32(v_rsrc, v_voff, ((key0 + 8 * (g_) + e) * ld3 + 32 * j) * 4, 0);
        ATK_VLOAD(0)
        ATK_VLOAD(1)
        if (HD > 64 && kt != wid) {                                           // head_dim 96: no K prefetch across tiles (registers)
#pragma unroll
            for (int u = 0; u < NSTEP; ++u) kb[u] = __builtin_amdgcn_raw_buffer_load_b128(k_rsrc, k_voff, key0 * k_tile + K_STEP * u, 0);
        }
        f32x16 S0, S1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { S0[r] = 0.f; S1[r] = 0.f; }
#pragma unroll
        for (int u = 0; u < NSTEP; ++u) {
            const u32x4 qw = *reinterpret_cast<const u32x4*>(q_frag + 8 * u);
            u32x4 f1, f2;
#pragma unroll
            for (int e = 0; e < 4; ++e) { f1[e] = qw[e] & 0xffffu; f2[e] = __builtin_amdgcn_alignbit(qw[e], qw[e], 16); }
            S0 = ATH_MFMA(kb[u], f1, S0);
            S1 = ATH_MFMA(kb[u], f2, S1);
        }
        __builtin_amdgcn_sched_barrier(0);
        ATK_VLOAD(2)
        ATK_VLOAD(3)
#undef ATK_VLOAD
        if (HD <= 64 && kt + 4 <= qt) {                                       // the next tile's K rows travel under the softmax and P.V
#pragma unroll
            for (int u = 0; u < NSTEP; ++u) kb[u] = __builtin_amdgcn_raw_buffer_load_b128(k_rsrc, k_voff, (key0 + 128) * k_tile + K_STEP * u, 0);
        }
        // online softmax on the raw dot products (attn_h2_kernel: subtract the maximum first, scale the small difference)
        float S[16];
        float mt = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = key0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const float s_ = __builtin_fmaf(S1[r], H2_LO_UNSCALE, S0[r]);
            S[r] = (key <= qidx) ? s_ : -INFINITY;
            mt = fmaxf(mt, S[r]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float m_new = fmaxf(m_run, mt);                                 // (a tile whose keys are all masked for this query: -inf stays -inf)
        const float alpha = (m_run == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((m_run - m_new) * qscale);
        float ps = 0.f;
        if (__any(alpha != 1.0f && m_run != -INFINITY)) {
#pragma unroll
            for (int c = 0; c < NCB; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) { O0[c][r] *= alpha; O1[c][r] *= alpha; }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float p[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                p[e] = (m_new == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((S[4 * g + e] - m_new) * qscale);      // exp2(-inf) = 0 for masked keys
                ps += p[e];
            }
            unsigned a[4];
            h2_words<false>(p[0], p[1], a[0], a[1]);
            h2_words<false>(p[2], p[3], a[2], a[3]);
            u32x4 pf1, pf2;
#pragma unroll
            for (int e = 0; e < 4; ++e) { pf1[e] = a[e] & 0xffffu; pf2[e] = __builtin_amdgcn_alignbit(a[e], a[e], 16); }
#pragma unroll
            for (int j = 0; j < NCB; ++j) {
                O0[j] = ATH_MFMA(vb[g][j], pf1, O0[j]);
                O1[j] = ATH_MFMA(vb[g][j], pf2, O1[j]);
            }
        }
        ps += __shfl_xor(ps, 32, 64);
        l_run = l_run * alpha + ps;
        m_run = m_new;
    }

    // ---- join the two accumulator sets, merge the 4 partial states: (2,3) -> (0,1), then 1 -> 0 (attention_fused.hip)
    f32x16 O[NCB];
#pragma unroll
    for (int c = 0; c < NCB; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[c][r] = __builtin_fmaf(O1[c][r], H2_LO_UNSCALE, O0[c][r]);
    float* lds = reinterpret_cast<float*>(ldsw);
#define ATTN_MERGE_WEIGHT(m_old, m_new) __builtin_amdgcn_exp2f((m_old - m_new) * qscale)
    ATTN_MERGE4(O, lds)
#undef ATTN_MERGE_WEIGHT
    constexpr int LDO = HD + 4;
    if (wid == 0) {
        const float inv = H2_A_UNSCALE / l_run;
#pragma unroll
        for (int j = 0; j < NCB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) lds[li * LDO + 32 * j + (r & 3) + 8 * (r >> 2) + 4 * lh] = O[j][r] * inv;
    }
    __syncthreads();
    ATTN_STORE_ROWS_H2(lds)
}

template <int HD, bool KBLK>
static int launch_ah2ks(const unsigned* qkv, const unsigned* kblk, const AttnGroups& G, int Tmax, double flop, int H, int d, float* out, int out_lines, hipStream_t s) {
    constexpr int NCB = HD / 32;
    size_t words = (size_t)32 * (HD + 4);                                     // Q tile / O tile
    const size_t merge = 2 * ((size_t)NCB * 16 * 64 + 128);
    if (merge > words) words = merge;
    const size_t lds = words * 4;
    ProfScope prof(PK_ATTN_FUSED, flop, s);
    int ntq, rc;
    unsigned grid;
    if ((rc = attn_grid_1d("attention_h2", G, H, Tmax, ntq, grid))) return rc;
    hipLaunchKernelGGL((attn_h2ks_kernel<HD, KBLK>), dim3(grid), dim3(256), lds, s, qkv, kblk, G, d, H, ntq, attn_qscale(HD, H2_A_UNSCALE), out, out_lines);
    R4D_CHECK_LAUNCH("attn_h2ks");
    return R4D_OK;
}

bool attention_h2_supported(int H, int d) {
    if (H < 1 || d % H) return false;
    const int hd = d / H;
    return hd == 32 || hd == 64 || hd == 96 || hd == 128 || hd == 256;
}

// Attention of n <= ATT_MAXG batches in one launch (launch_attention_fused_groups's contract) on h2 words
// out_lines: `out` receives the merged-head rows as f16x2 lines [rows][d/32][2][32] fp16 (d % 32 == 0) instead of fp32 [rows][d]
// kblk (nullable): the key-blocked K image (attn_h2_kernel) -- the K columns of `qkv` are then not read
int launch_attention_h2_groups(const unsigned* qkv, int n, const int* Bs, const int* Ts, const long long* row0s, int H, int d,
                               float* out, hipStream_t s, bool out_lines, const unsigned* kblk) {
    R4D_REQUIRE(qkv && out, "attention_h2: null pointer");
    R4D_REQUIRE(attention_h2_supported(H, d), "attention_h2: head_dim %d has no instantiation (32 / 64 / 96 / 128 / 256)", H > 0 ? d / H : 0);
    AttnGroups G;
    int Tmax, rc;
    double flop;
    if ((rc = attn_groups_fill("attention_h2", n, Bs, Ts, row0s, H, d, G, Tmax, flop))) return rc;
    for (int g = 0; g < n; ++g) R4D_REQUIRE(Bs[g] >= 1 && Ts[g] >= 1, "attention_h2: batch %d: B=%d T=%d", g, Bs[g], Ts[g]);
    // (head_dim, key-blocked K) -> launcher and dispatch branch.  The rows stand in the order in which the kernels have always been
    // instantiated, which is the order of the functions in the code object.
#define ATH_KERNELS(X)                                                                                              \
    X(32, true, launch_ah2ks, ATT_H2_KS32_KBLK) X(64, true, launch_ah2ks, ATT_H2_KS64_KBLK) X(96, true, launch_ah2ks, ATT_H2_KS96_KBLK) \
    X(32, false, launch_ah2ks, ATT_H2_KS32) X(64, false, launch_ah2ks, ATT_H2_KS64) X(96, false, launch_ah2ks, ATT_H2_KS96)   \
    X(128, true, launch_ah2, ATT_H2_128_KBLK) X(128, false, launch_ah2, ATT_H2_128)                                 \
    X(256, true, launch_ah2, ATT_H2_256_KBLK) X(256, false, launch_ah2, ATT_H2_256)
#define X(HD_, KBLK_, LAUNCH_, BRANCH_)                                                                             \
    if (d / H == HD_ && (kblk != nullptr) == KBLK_) {                                                               \
        R4D_BRANCH(BRANCH_);                                                                                        \
        return LAUNCH_<HD_, KBLK_>(qkv, kblk, G, Tmax, flop, H, d, out, out_lines ? 1 : 0, s);                      \
    }
    ATH_KERNELS(X)
#undef X
#undef ATH_KERNELS
    return R4D_ERR_INVALID;                             // not reached: attention_h2_supported has passed
}

// K columns of row-major qkv words -> the key-blocked image (what gemm_h2p's epilogue writes directly; tests, external producers)
__global__ __launch_bounds__(256) void pack_kblk_words_kernel(const unsigned* __restrict__ qkv, long long M, int H, int d, unsigned* __restrict__ kblk) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;      // one thread per 4 words (16 bytes) of the image
    const long long n4 = (M + 31) / 32 * 32 * (long long)(d / 4);
    if (i >= n4) return;
    const int hd = d / H, nstep = hd / 8;
    const int slot = (int)(i & 63);                                     // [half][row & 31]
    const long long chunk = i >> 6;                                     // (block * H + head) * nstep + u
    const int u = (int)(chunk % nstep), head = (int)((chunk / nstep) % H);
    const long long row = (chunk / nstep / H) * 32 + (slot & 31);
    u32x4 v = {0u, 0u, 0u, 0u};
    if (row < M) v = *reinterpret_cast<const u32x4*>(qkv + row * 3 * d + d + head * hd + 8 * u + 4 * (slot >> 5));
    reinterpret_cast<u32x4*>(kblk)[i] = v;
}
int launch_pack_kblk_words(const unsigned* qkv, long long M, int H, int d, unsigned* kblk, hipStream_t s) {
    R4D_REQUIRE(qkv && kblk && M >= 1 && attention_h2_supported(H, d), "pack_kblk_words: bad arguments (head_dim 32 / 64 / 96 / 128 / 256)");
    const long long n4 = (M + 31) / 32 * 32 * (long long)(d / 4);
    hipLaunchKernelGGL(pack_kblk_words_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, qkv, M, H, d, kblk);
    R4D_CHECK_LAUNCH("pack_kblk_words");
    return R4D_OK;
}

int launch_pack_h2_words(const float* x, long long n, unsigned* words, hipStream_t s) {
    R4D_REQUIRE(x && words && n >= 1 && n < (1ll << 39), "pack_h2_words: bad arguments");
    hipLaunchKernelGGL(pack_h2_words_kernel, dim3((unsigned)((n + 511) / 512)), dim3(256), 0, s, x, n, words);
    R4D_CHECK_LAUNCH("pack_h2_words");
    return R4D_OK;
}

int dbgflag_att_h2() { return ATH_DBG != 0; }

}  // namespace r4d

using namespace r4d;

extern "C" {

int r4d_pack_h2_words_f32(const float* x_d, int64_t n, uint32_t* words_d, void* stream) {
    return launch_pack_h2_words(x_d, n, words_d, (hipStream_t)stream);
}

int r4d_pack_kblk_words(const uint32_t* qkv_words_d, int64_t rows, int32_t n_head, int32_t d, uint32_t* kblk_d, void* stream) {
    return launch_pack_kblk_words(qkv_words_d, rows, n_head, d, kblk_d, (hipStream_t)stream);
}

int r4d_attention_h2_kblk_f32(const uint32_t* qkv_words_d, const uint32_t* kblk_d, int32_t B, int32_t T, int32_t n_head, int32_t d,
                              float* a_d, void* stream) {
    R4D_REQUIRE(B >= 1 && T >= 1 && kblk_d, "attention_h2_kblk: B=%d T=%d", B, T);
    const long long row0 = 0;
    return launch_attention_h2_groups(qkv_words_d, 1, &B, &T, &row0, n_head, d, a_d, (hipStream_t)stream, false, kblk_d);
}

int r4d_attention_h2_f32(const uint32_t* qkv_words_d, int32_t B, int32_t T, int32_t n_head, int32_t d, float* a_d, void* stream) {
    R4D_REQUIRE(B >= 1 && T >= 1, "attention_h2: B=%d T=%d", B, T);
    const long long row0 = 0;
    return launch_attention_h2_groups(qkv_words_d, 1, &B, &T, &row0, n_head, d, a_d, (hipStream_t)stream);
}

}  // extern "C"
