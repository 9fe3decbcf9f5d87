// The opt-in FUSED attention of the training steps (r4d_set_train_attention_fused): forward and backward of
// Attention._attn (modeling_gpt2.py:140-160) per (sequence, head) with NO [T, T] block in global memory.  The arithmetic is the
// "+attn" one of gemm_b1h.hip: Q, K, V, dO, the probabilities and dS enter every product as bf16 (round to nearest even,
// v_cvt_pk_bf16_f32, where they are staged or produced), ONE v_mfma_f32_32x32x16_bf16 per k-step, fp32 accumulation; the division
// by sqrt(hd), max, exp, the sums and the dS arithmetic are fp32.  NOT fp32-accurate.
//
//   forward   one workgroup per 128 queries (a wavefront owns 32), key tiles of 32 up to the diagonal, online softmax:
//             S^T = K . Q^T, so that a LANE holds one query (column) and 16 keys (rows) -- four groups of four consecutive keys;
//             row maximum and sum are in-lane plus ONE exchange with lane ^ 32.  The unnormalised p = exp(s - m) goes through the
//             dropout mask, is rounded and is the B operand of O^T += V^T . p^T as it stands: the MFMA's k slots are the
//             accumulator's own row order, and V^T is staged in that order (perm32 below).  O = acc / l into `att` (merged heads),
//             lse = m + log(l) per (sequence, head, query).
//   backward  three kernels that form P = exp(s - lse) again and need no atomics, no split-K and no state across workgroups:
//             D     = rowsum(P o mask dP / (1-p)) in fp32, the dQ kernel's walk without its last product (see taf_dq_kernel);
//             dQ    one workgroup per 128 queries, the forward's orientation:  dP^T = V . dO^T,  dS = P (mask dP / (1-p) - D) /
//                   sqrt(hd),  dQ^T += K^T . dS^T;
//             dK/dV one workgroup per 128 (head_dim <= 128) or 64 keys, looping over the 32-query tiles at or below them, in the
//                   other orientation (S = Q . K^T: a lane holds one key and 16 queries):  dV^T += dO^T . Pd,  dK^T += Q^T . dS.
//   Outputs go straight into this head's columns of att [B, T, d] / dqkv [B, T, 3d], 16 bytes per store.
// Dropout: the mask of element (bh, i, j) is launch_dropout's at pbase + (bh T + i) ld + j, ld = ceil128(T) (philox.h); a Philox
// block is four consecutive keys of one query: the forward and the dQ kernel own whole blocks (one generator call per four
// elements), the dK/dV kernel owns one key per lane and generates a block per ELEMENT (4 x the generator work, with dropout only).
// Causal masking is by selection: a key right of the diagonal or at / past T gives p = 0 exactly, whatever the memory holds; rows
// and columns past T / head_dim are staged as zeros by selection with clamped addresses; nothing outside the head's own
// columns of the T valid rows is written.  Every loop is bounded by T; a (sequence, head)'s bits depend on its own operands alone.
// LDS images: row-major [32 rows][HDP + 8] bf16 (a lane's fragment, eight consecutive head-dim elements of its row, is one
// ds_read_b128) and transposed [HDP][32 + 8] bf16 in perm32 order; HDP = 32 NT >= head_dim, NT in {1, 2, 3, 4, 8}.
#include <math.h>
#include "gemm_common.h"
#include "bf16x3.h"
#include "philox.h"

namespace r4d {

struct TafShape {
    int T, H, d, hd, ld;
    float sd;                       // sqrt(hd): the logits are DIVIDED by it, like the EPI_SCALE_DIV epilogue of the products
    int drop; unsigned threshold; float scale;
    DropKey key; unsigned site; unsigned long long pbase4;      // pbase / 4
};

// slot of row t of a 32-row tile in the transposed images = the order in which the 32x32 accumulator holds its rows: register
// i of lane half h is row (i & 3) + 8 (i >> 2) + 4 h, and registers 8 kk .. 8 kk + 7 are the eight k slots of k-step kk
__device__ __forceinline__ int perm32(int t) {
    const int u = t & 15;
    return (t & 16) | (((u >> 2) & 1) << 3) | ((u >> 3) << 2) | (u & 3);
}
__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// rows r0 .. r0 + 31 of src (fp32, `hd` columns, row stride lds) -> bf16 images; rows at / past T and columns at / past hd are zeros
template <int NT, int NTH, bool RM, bool TR>
__device__ __forceinline__ void taf_stage(const float* __restrict__ src, int ldsrc, int r0, int T, int hd, unsigned short* rm,
                                          unsigned short* tr, int tid) {
    constexpr int HDP = 32 * NT, C4 = HDP / 4, LDR = HDP + 8;
#pragma unroll 2
    for (int idx = tid; idx < 32 * C4; idx += NTH) {
        const int row = idx / C4, col = 4 * (idx % C4);
        const bool ok = r0 + row < T && col < hd;
        f32x4 v = *reinterpret_cast<const f32x4*>(src + (long long)min(r0 + row, T - 1) * ldsrc + (ok ? col : 0));
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = ok ? v[e] : 0.f;
        const unsigned lo = cvt_pk_bf16(v[0], v[1]), hi = cvt_pk_bf16(v[2], v[3]);
        if (RM) *reinterpret_cast<u32x2*>(rm + row * LDR + col) = u32x2{lo, hi};
        if (TR) {
            const int p = perm32(row);
            tr[(col + 0) * 40 + p] = (unsigned short)(lo & 0xffffu); tr[(col + 1) * 40 + p] = (unsigned short)(lo >> 16);
            tr[(col + 2) * 40 + p] = (unsigned short)(hi & 0xffffu); tr[(col + 3) * 40 + p] = (unsigned short)(hi >> 16);
        }
    }
}

// a lane's register fragments of ITS row of src: k-step kk holds columns 16 kk + 8 h .. + 7 (zeros at / past hd)
template <int NT>
__device__ __forceinline__ void taf_row_frags(const float* __restrict__ rowp, int hd, int h, u32x4* f) {
#pragma unroll
    for (int kk = 0; kk < 2 * NT; ++kk) {
        const int col = 16 * kk + 8 * h;
        const bool ok = col < hd;
        const f32x4 a = *reinterpret_cast<const f32x4*>(rowp + (ok ? col : 0)), b = *reinterpret_cast<const f32x4*>(rowp + (ok ? col + 4 : 0));
        f[kk] = ok ? u32x4{cvt_pk_bf16(a[0], a[1]), cvt_pk_bf16(a[2], a[3]), cvt_pk_bf16(b[0], b[1]), cvt_pk_bf16(b[2], b[3])} : u32x4{0u, 0u, 0u, 0u};
    }
}

__device__ __forceinline__ f32x16 taf_mfma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ u32x4 taf_lds16(const unsigned short* p) { return *reinterpret_cast<const u32x4*>(p); }
// registers 8 kk .. 8 kk + 7 of an accumulator-shaped array, rounded: the operand of k-step kk
__device__ __forceinline__ u32x4 taf_pack8(const float* v) {
    return u32x4{cvt_pk_bf16(v[0], v[1]), cvt_pk_bf16(v[2], v[3]), cvt_pk_bf16(v[4], v[5]), cvt_pk_bf16(v[6], v[7])};
}
__device__ __forceinline__ f32x16 taf_zero16() {
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    return z;
}
// acc [NT] (rows = head-dim index, column = the lane's token) -> out row `rowp` of this head, 16 bytes per store
template <int NT>
__device__ __forceinline__ void taf_store_row(const f32x16* acc, float mul, float* __restrict__ rowp, int hd, int h) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = 32 * nt + 8 * g + 4 * h;
            if (c < hd)
                *reinterpret_cast<f32x4*>(rowp + c) = f32x4{acc[nt][4 * g] * mul, acc[nt][4 * g + 1] * mul, acc[nt][4 * g + 2] * mul, acc[nt][4 * g + 3] * mul};
        }
}

// ---------------------------------------------------------------------------------------------------------------- forward
template <int NT>
__global__ __launch_bounds__(256) void taf_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ att, float* __restrict__ lse,
                                                      const TafShape g) {
    constexpr int HDP = 32 * NT, LDR = HDP + 8;
    extern __shared__ __attribute__((aligned(16))) unsigned short taf_lds[];
    unsigned short* Ks = taf_lds;                    // [32][LDR]
    unsigned short* Vt = Ks + 32 * LDR;              // [HDP][40]
    const int bh = blockIdx.z, b = bh / g.H, hh = bh % g.H;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
    const int T = g.T, m0 = blockIdx.x * 128, q0 = m0 + 32 * w, qi = q0 + r;
    const float* __restrict__ base = qkv + (long long)b * T * 3 * g.d + (long long)hh * g.hd;
    const bool active = q0 < T;                      // wave-uniform
    u32x4 qf[2 * NT];
    taf_row_frags<NT>(base + (long long)min(qi, T - 1) * 3 * g.d, g.hd, h, qf);
    f32x16 o[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) o[nt] = taf_zero16();
    float m = -INFINITY, l = 0.f;
    const int kend = min(T, m0 + 128);
    for (int k0 = 0; k0 < kend; k0 += 32) {
        __syncthreads();
        taf_stage<NT, 256, true, false>(base + g.d, 3 * g.d, k0, T, g.hd, Ks, nullptr, tid);
        taf_stage<NT, 256, false, true>(base + 2 * g.d, 3 * g.d, k0, T, g.hd, nullptr, Vt, tid);
        __syncthreads();
        if (!active || k0 > q0 + 31) continue;       // wave-uniform: every key of the tile is right of the wave's queries
        f32x16 s = taf_zero16();
#pragma unroll
        for (int kk = 0; kk < 2 * NT; ++kk) s = taf_mfma(taf_lds16(Ks + r * LDR + 16 * kk + 8 * h), qf[kk], s);
        float p[16];
        float tmax = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = k0 + acc_row(i, h);
            p[i] = (key <= qi && key < T) ? s[i] / g.sd : -INFINITY;
            tmax = fmaxf(tmax, p[i]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float mn = fmaxf(m, tmax);             // finite: key 0 is left of every query and in the first tile
        const float alpha = __expf(m - mn);
        float lsum = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            p[i] = p[i] == -INFINITY ? 0.f : __expf(p[i] - mn);
            lsum += p[i];
        }
        lsum += __shfl_xor(lsum, 32);
        l = l * alpha + lsum;
        m = mn;
        if (g.drop) {
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int kb = k0 + 8 * q4 + 4 * h;
                if (kb > qi) continue;               // the four are zeros already
                const uint4 rr = attn_philox(g.pbase4 + (unsigned long long)((((long long)bh * T + qi) * g.ld + kb) >> 2), g.key, g.site);
                p[4 * q4 + 0] = rr.x >= g.threshold ? p[4 * q4 + 0] * g.scale : 0.f;
                p[4 * q4 + 1] = rr.y >= g.threshold ? p[4 * q4 + 1] * g.scale : 0.f;
                p[4 * q4 + 2] = rr.z >= g.threshold ? p[4 * q4 + 2] * g.scale : 0.f;
                p[4 * q4 + 3] = rr.w >= g.threshold ? p[4 * q4 + 3] * g.scale : 0.f;
            }
        }
        const u32x4 pf0 = taf_pack8(p), pf1 = taf_pack8(p + 8);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
            for (int i = 0; i < 16; ++i) o[nt][i] *= alpha;
            o[nt] = taf_mfma(taf_lds16(Vt + (32 * nt + r) * 40 + 8 * h), pf0, o[nt]);
            o[nt] = taf_mfma(taf_lds16(Vt + (32 * nt + r) * 40 + 16 + 8 * h), pf1, o[nt]);
        }
    }
    if (!active || qi >= T) return;
    taf_store_row<NT>(o, 1.f / l, att + ((long long)b * T + qi) * g.d + (long long)hh * g.hd, g.hd, h);
    if (h == 0) lse[(long long)bh * T + qi] = m + logf(l);
}

// ---------------------------------------------------------------------------------------------------------------- dQ
// ROWSUM: the first backward launch -- the same walk without the K^T image and the dQ products: D_i = sum_j P_ij g_ij in fp32, g = mask
// dP / (1 - p), what the unfused backward's softmax kernel sums (D = rowsum(dO o O) from the bf16-rounded forward output was measured at
// up to 2.1 x the unfused chain's dQ / dK error on short rows: profiles/train_attention_fused.md); D is WRITTEN here, read below
template <int NT, bool ROWSUM>
__global__ __launch_bounds__(256) void taf_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ dao, const float* __restrict__ lse,
                                                     float* __restrict__ D, float* __restrict__ dqkv, const TafShape g) {
    constexpr int HDP = 32 * NT, LDR = HDP + 8;
    extern __shared__ __attribute__((aligned(16))) unsigned short taf_lds[];
    unsigned short* Ks = taf_lds;                    // [32][LDR]
    unsigned short* Vs = Ks + 32 * LDR;              // [32][LDR]
    unsigned short* Kt = Vs + 32 * LDR;              // [HDP][40]
    const int bh = blockIdx.z, b = bh / g.H, hh = bh % g.H;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
    const int T = g.T, m0 = blockIdx.x * 128, q0 = m0 + 32 * w, qi = q0 + r, qc = min(qi, T - 1);
    const float* __restrict__ base = qkv + (long long)b * T * 3 * g.d + (long long)hh * g.hd;
    const bool active = q0 < T;
    u32x4 qf[2 * NT], gf[2 * NT];
    taf_row_frags<NT>(base + (long long)qc * 3 * g.d, g.hd, h, qf);
    taf_row_frags<NT>(dao + ((long long)b * T + qc) * g.d + (long long)hh * g.hd, g.hd, h, gf);
    const float Li = lse[(long long)bh * T + qc], Di = ROWSUM ? 0.f : D[(long long)bh * T + qc];
    f32x16 dq[ROWSUM ? 1 : NT];
#pragma unroll
    for (int nt = 0; nt < (ROWSUM ? 1 : NT); ++nt) dq[nt] = taf_zero16();
    float dsum = 0.f;
    const int kend = min(T, m0 + 128);
    for (int k0 = 0; k0 < kend; k0 += 32) {
        __syncthreads();
        taf_stage<NT, 256, true, !ROWSUM>(base + g.d, 3 * g.d, k0, T, g.hd, Ks, Kt, tid);
        taf_stage<NT, 256, true, false>(base + 2 * g.d, 3 * g.d, k0, T, g.hd, Vs, nullptr, tid);
        __syncthreads();
        if (!active || k0 > q0 + 31) continue;
        f32x16 s = taf_zero16(), dp = taf_zero16();
#pragma unroll
        for (int kk = 0; kk < 2 * NT; ++kk) {
            s = taf_mfma(taf_lds16(Ks + r * LDR + 16 * kk + 8 * h), qf[kk], s);
            dp = taf_mfma(taf_lds16(Vs + r * LDR + 16 * kk + 8 * h), gf[kk], dp);
        }
        float ds[16];
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int kb = k0 + 8 * q4 + 4 * h;
            uint4 rr = make_uint4(~0u, ~0u, ~0u, ~0u);
            if (g.drop && kb <= qi)
                rr = attn_philox(g.pbase4 + (unsigned long long)((((long long)bh * T + qi) * g.ld + kb) >> 2), g.key, g.site);
            const unsigned rw[4] = {rr.x, rr.y, rr.z, rr.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = 4 * q4 + e, key = kb + e;
                const bool valid = key <= qi && key < T;
                const float P = valid ? __expf(s[i] / g.sd - Li) : 0.f;
                float gd = dp[i];
                if (g.drop) gd = rw[e] >= g.threshold ? gd * g.scale : 0.f;
                if (ROWSUM) dsum += valid ? P * gd : 0.f;
                ds[i] = valid ? P * (gd - Di) / g.sd : 0.f;
            }
        }
        if (ROWSUM) continue;
        const u32x4 f0 = taf_pack8(ds), f1 = taf_pack8(ds + 8);
#pragma unroll
        for (int nt = 0; nt < (ROWSUM ? 1 : NT); ++nt) {
            dq[nt] = taf_mfma(taf_lds16(Kt + (32 * nt + r) * 40 + 8 * h), f0, dq[nt]);
            dq[nt] = taf_mfma(taf_lds16(Kt + (32 * nt + r) * 40 + 16 + 8 * h), f1, dq[nt]);
        }
    }
    if (ROWSUM) {
        dsum += __shfl_xor(dsum, 32);
        if (active && qi < T && h == 0) D[(long long)bh * T + qi] = dsum;
        return;
    }
    if (!active || qi >= T) return;
    taf_store_row<NT>(dq, 1.f, dqkv + ((long long)b * T + qi) * 3 * g.d + (long long)hh * g.hd, g.hd, h);
}

// ---------------------------------------------------------------------------------------------------------------- dK, dV
// NTO: the 32-column output tiles a workgroup accumulates, blockIdx.y picks which (head_dim > 128: two halves of 4 -- 2 x 128
// accumulator registers beside the operands do not fit 512; each half forms S and dP itself, the same bits)
template <int NT, int NW, int NTO>
__global__ __launch_bounds__(64 * NW) void taf_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ dao,
                                                          const float* __restrict__ lse, const float* __restrict__ D,
                                                          float* __restrict__ dqkv, const TafShape g) {
    constexpr int HDP = 32 * NT, LDR = HDP + 8, NTH = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) unsigned short taf_lds[];
    unsigned short* Ks = taf_lds;                    // [32 NW][LDR]: the workgroup's keys, staged once
    unsigned short* Vs = Ks + 32 * NW * LDR;
    unsigned short* Qs = Vs + 32 * NW * LDR;         // [32][LDR] and [HDP][40] of the query tile at hand
    unsigned short* Gs = Qs + 32 * LDR;
    unsigned short* Qt = Gs + 32 * LDR;
    unsigned short* Gt = Qt + HDP * 40;
    float* Ls = reinterpret_cast<float*>(Gt + HDP * 40);   // lse [32], D [32]
    float* Ds = Ls + 32;
    const int bh = blockIdx.z, b = bh / g.H, hh = bh % g.H;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
    const int T = g.T, n0 = blockIdx.x * 32 * NW, kq0 = n0 + 32 * w, kj = kq0 + r;
    const float* __restrict__ base = qkv + (long long)b * T * 3 * g.d + (long long)hh * g.hd;
    const float* __restrict__ gbase = dao + (long long)b * T * g.d + (long long)hh * g.hd;
    const bool active = kq0 < T;
    const int nt0 = blockIdx.y * NTO;
#pragma unroll
    for (int t = 0; t < NW; ++t) {
        taf_stage<NT, NTH, true, false>(base + g.d, 3 * g.d, n0 + 32 * t, T, g.hd, Ks + 32 * t * LDR, nullptr, tid);
        taf_stage<NT, NTH, true, false>(base + 2 * g.d, 3 * g.d, n0 + 32 * t, T, g.hd, Vs + 32 * t * LDR, nullptr, tid);
    }
    f32x16 dk[NTO], dv[NTO];
#pragma unroll
    for (int nt = 0; nt < NTO; ++nt) { dk[nt] = taf_zero16(); dv[nt] = taf_zero16(); }
    const unsigned short* kfrag = Ks + (32 * w + r) * LDR + 8 * h;
    const unsigned short* vfrag = Vs + (32 * w + r) * LDR + 8 * h;
    for (int q0 = n0; q0 < T; q0 += 32) {            // n0 is a multiple of 32: the first tile holds the diagonal
        __syncthreads();
        taf_stage<NT, NTH, true, true>(base, 3 * g.d, q0, T, g.hd, Qs, Qt, tid);
        taf_stage<NT, NTH, true, true>(gbase, g.d, q0, T, g.hd, Gs, Gt, tid);
        if (tid < 32) {
            const long long o = (long long)bh * T + min(q0 + tid, T - 1);
            Ls[tid] = lse[o]; Ds[tid] = D[o];
        }
        __syncthreads();
        if (!active || q0 + 31 < kq0) continue;      // wave-uniform: every query of the tile is left of the wave's keys
        f32x16 s = taf_zero16(), dp = taf_zero16();
#pragma unroll
        for (int kk = 0; kk < 2 * NT; ++kk) {
            s = taf_mfma(taf_lds16(Qs + r * LDR + 16 * kk + 8 * h), taf_lds16(kfrag + 16 * kk), s);
            dp = taf_mfma(taf_lds16(Gs + r * LDR + 16 * kk + 8 * h), taf_lds16(vfrag + 16 * kk), dp);
        }
        float pd[16], ds[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int qr = acc_row(i, h), q = q0 + qr;
            const bool valid = kj <= q && q < T;     // (kj <= q < T: the key is inside T too)
            const float P = valid ? __expf(s[i] / g.sd - Ls[qr]) : 0.f;
            float Pd = P, gd = dp[i];
            if (g.drop && valid) {
                const uint4 rr = attn_philox(g.pbase4 + (unsigned long long)((((long long)bh * T + q) * g.ld + kj) >> 2), g.key, g.site);
                const unsigned rw = (kj & 3) == 0 ? rr.x : (kj & 3) == 1 ? rr.y : (kj & 3) == 2 ? rr.z : rr.w;
                const bool keep = rw >= g.threshold;
                Pd = keep ? P * g.scale : 0.f;
                gd = keep ? gd * g.scale : 0.f;
            }
            pd[i] = Pd;
            ds[i] = valid ? P * (gd - Ds[qr]) / g.sd : 0.f;
        }
        const u32x4 p0 = taf_pack8(pd), p1 = taf_pack8(pd + 8), s0 = taf_pack8(ds), s1 = taf_pack8(ds + 8);
#pragma unroll
        for (int nt = 0; nt < NTO; ++nt) {
            const int row = (32 * (nt0 + nt) + r) * 40 + 8 * h;
            dv[nt] = taf_mfma(taf_lds16(Gt + row), p0, dv[nt]);
            dv[nt] = taf_mfma(taf_lds16(Gt + row + 16), p1, dv[nt]);
            dk[nt] = taf_mfma(taf_lds16(Qt + row), s0, dk[nt]);
            dk[nt] = taf_mfma(taf_lds16(Qt + row + 16), s1, dk[nt]);
        }
    }
    if (!active || kj >= T) return;
    float* __restrict__ orow = dqkv + ((long long)b * T + kj) * 3 * g.d + (long long)hh * g.hd;
    taf_store_row<NTO>(dk, 1.f, orow + g.d + 32 * nt0, g.hd - 32 * nt0, h);
    taf_store_row<NTO>(dv, 1.f, orow + 2 * g.d + 32 * nt0, g.hd - 32 * nt0, h);
}

// ---------------------------------------------------------------------------------------------------------------- host side
static size_t taf_fwd_lds(int NT) { return (size_t)(32 * (32 * NT + 8) + 32 * NT * 40) * 2; }
static size_t taf_dq_lds(int NT) { return (size_t)(2 * 32 * (32 * NT + 8) + 32 * NT * 40) * 2; }
static size_t taf_dkv_lds(int NT, int NW) { return (size_t)((2 * NW + 2) * 32 * (32 * NT + 8) + 2 * 32 * NT * 40) * 2 + 64 * sizeof(float); }

template <typename K>
static int taf_allow_lds(K kernel, size_t bytes, const char* name) {
    if (bytes > 48 * 1024 && hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
        set_error("%s: %zu bytes of LDS refused", name, bytes);
        return R4D_ERR_HIP;
    }
    return R4D_OK;
}

bool attn_train_fused_supported(int B, int T, int H, int d) {
    return B >= 1 && T >= 1 && T <= 1024 && H >= 1 && d >= 1 && d % H == 0 && (d / H) % 16 == 0 && d / H >= 16 && d / H <= 256 &&
           (long long)B * H <= 65535;
}

static int taf_shape(const char* who, int B, int T, int H, int d, float attn_p, DropKey key, unsigned site, unsigned long long pbase,
                     TafShape& g, int& NT) {
    R4D_REQUIRE(attn_train_fused_supported(B, T, H, d),
                "%s: bad shape B=%d T=%d H=%d d=%d (head_dim %% 16 == 0 in 16 .. 256, T in 1 .. 1024, B * H <= 65535 wanted)", who, B, T, H, d);
    R4D_REQUIRE(attn_p >= 0.f && attn_p < 1.f && site < 65536u && pbase % 4 == 0, "%s: dropout p=%g site=%u base=%llu (p in [0, 1), site < 65536, base %% 4 == 0 wanted)",
                who, (double)attn_p, site, pbase);
    g.T = T; g.H = H; g.d = d; g.hd = d / H; g.ld = (T + 127) / 128 * 128;
    g.sd = (float)sqrt((double)g.hd);
    g.drop = attn_p > 0.f;
    g.threshold = (unsigned)((double)attn_p * 4294967296.0);          // launch_dropout's: keep iff u32 >= threshold
    g.scale = 1.0f / (1.0f - attn_p);
    g.key = key; g.site = site; g.pbase4 = pbase / 4;
    NT = g.hd <= 32 ? 1 : g.hd <= 64 ? 2 : g.hd <= 96 ? 3 : g.hd <= 128 ? 4 : 8;
    return R4D_OK;
}

#define TAF_NT_SWITCH(NT, CALL) \
    switch (NT) { case 1: CALL(1) break; case 2: CALL(2) break; case 3: CALL(3) break; case 4: CALL(4) break; default: CALL(8) break; }

int launch_attn_train_fused_fwd(const float* qkv, int B, int T, int H, int d, float* att, float* lse, float attn_p, DropKey key,
                                unsigned site, unsigned long long pbase, hipStream_t s) {
    R4D_REQUIRE(qkv && att && lse, "train_attn_fused_fwd: null pointer");
    R4D_REQUIRE(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)att % 16) == 0, "train_attn_fused_fwd: qkv / att must be 16-byte aligned");
    TafShape g; int NT;
    int rc = taf_shape("train_attn_fused_fwd", B, T, H, d, attn_p, key, site, pbase, g, NT);
    if (rc) return rc;
    const dim3 grid(cdiv(T, 128), 1, B * H);
    R4D_BRANCH(TAF_FWD);
    ProfScope prof(PK_ATTN_TRAIN_FUSED_FWD, 2.0 * (double)B * H * T * T * g.hd, s);   // two causal products
#define TAF_FWD(N) { if ((rc = taf_allow_lds(taf_fwd_kernel<N>, taf_fwd_lds(N), "train_attn_fused_fwd"))) return rc; \
                     hipLaunchKernelGGL(taf_fwd_kernel<N>, grid, dim3(256), taf_fwd_lds(N), s, qkv, att, lse, g); }
    TAF_NT_SWITCH(NT, TAF_FWD)
#undef TAF_FWD
    R4D_CHECK_LAUNCH("train_attn_fused_fwd");
    return R4D_OK;
}

size_t attn_train_fused_bwd_scratch_floats(int B, int T, int H) { return (size_t)B * H * T; }

int launch_attn_train_fused_bwd(const float* qkv, const float* att, const float* lse, const float* dao, int B, int T, int H, int d,
                                float* dqkv, float* Dscr, float attn_p, DropKey key, unsigned site, unsigned long long pbase, hipStream_t s) {
    R4D_REQUIRE(qkv && att && lse && dao && dqkv && Dscr, "train_attn_fused_bwd: null pointer");         // (att: part of the contract, not read)
    R4D_REQUIRE(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)dao % 16) == 0 && ((uintptr_t)dqkv % 16) == 0,
                "train_attn_fused_bwd: qkv / dao / dqkv must be 16-byte aligned");
    TafShape g; int NT;
    int rc = taf_shape("train_attn_fused_bwd", B, T, H, d, attn_p, key, site, pbase, g, NT);
    if (rc) return rc;
    const double flop = (double)B * H * T * T * g.hd;                 // per causal product
    {
        R4D_BRANCH(TAF_ROWSUM);
        ProfScope prof(PK_ATTN_TRAIN_FUSED_ROWSUM, 2.0 * flop, s);
#define TAF_D(N) { if ((rc = taf_allow_lds(taf_dq_kernel<N, true>, taf_dq_lds(N), "train_attn_fused_bwd"))) return rc; \
                   hipLaunchKernelGGL((taf_dq_kernel<N, true>), dim3(cdiv(T, 128), 1, B * H), dim3(256), taf_dq_lds(N), s, qkv, dao, lse, Dscr, dqkv, g); }
        TAF_NT_SWITCH(NT, TAF_D)
#undef TAF_D
        R4D_CHECK_LAUNCH("train_attn_fused_bwd (row sums)");
    }
    {
        R4D_BRANCH(TAF_DKV);
        ProfScope prof(PK_ATTN_TRAIN_FUSED_DKV, 4.0 * flop, s);
#define TAF_DKV(N) { constexpr int NW = N <= 4 ? 4 : 2, NTO = N <= 4 ? N : 4; \
                     if ((rc = taf_allow_lds(taf_dkv_kernel<N, NW, NTO>, taf_dkv_lds(N, NW), "train_attn_fused_bwd"))) return rc; \
                     hipLaunchKernelGGL((taf_dkv_kernel<N, NW, NTO>), dim3(cdiv(T, 32 * NW), N / NTO, B * H), dim3(64 * NW), taf_dkv_lds(N, NW), s, qkv, dao, lse, Dscr, dqkv, g); }
        TAF_NT_SWITCH(NT, TAF_DKV)
#undef TAF_DKV
        R4D_CHECK_LAUNCH("train_attn_fused_bwd (dK, dV)");
    }
    {
        R4D_BRANCH(TAF_DQ);
        ProfScope prof(PK_ATTN_TRAIN_FUSED_DQ, 3.0 * flop, s);
#define TAF_DQ(N) { if ((rc = taf_allow_lds(taf_dq_kernel<N, false>, taf_dq_lds(N), "train_attn_fused_bwd"))) return rc; \
                    hipLaunchKernelGGL((taf_dq_kernel<N, false>), dim3(cdiv(T, 128), 1, B * H), dim3(256), taf_dq_lds(N), s, qkv, dao, lse, Dscr, dqkv, g); }
        TAF_NT_SWITCH(NT, TAF_DQ)
#undef TAF_DQ
        R4D_CHECK_LAUNCH("train_attn_fused_bwd (dQ)");
    }
    return R4D_OK;
}

}  // namespace r4d
