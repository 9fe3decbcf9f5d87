// The encoder's opt-in bf16 attention (r4d_set_encode_attention_bf16 under r4d_set_encode_bf16; ops.set_encode_precision("bf16+attn");
// DESIGN.md 7 item 13): softmax(Q . K^T / sqrt(hd), causal) . V per (sequence, head) with no T x T block in memory, over up to
// ATT_MAXG batches of different T in one launch.  NOT fp32-accurate.  The arithmetic, per (sequence, head):
//   * q, k and v are rounded to bf16, round to nearest even (v_cvt_pk_bf16_f32, the rounding gemm_b1 applies) -- while they are staged
//     (fp32 qkv) or by their producer (bf16 qkv, gemm_b1's EPI_NONE_BF16): the same values rounded once by the same rule, the same bits;
//   * S = q . k^T on ONE v_mfma_f32_32x32x16_bf16 per 16 k with fp32 accumulation, DIVIDED by sqrt(hd) in fp32;
//   * the causal mask is by selection: a key right of the diagonal or at / past T contributes p = 0 exactly, whatever memory holds
//     (K rows past T are never trusted; V rows past T are staged as zeros, so that 0 x garbage cannot arise);
//   * the online softmax (running maximum m, sum l, exp) is fp32;
//   * the UNNORMALISED p = exp(s - m) enters P . V rounded to bf16; the row sum l adds the UNROUNDED fp32 p;
//   * O is accumulated in fp32 (rescaled by exp(m_old - m_new) when the maximum rises) and multiplied by 1 / l at the end; a bf16
//     output is RN(O / l).
// A (sequence, head)'s bits depend on its own operands alone: the tile walk is a function of T and the query's position, there is no
// state across workgroups, and nothing outside the head's own columns of the T valid rows is read into a result or written.
//
// Structure: the orientation and LDS images of taf_fwd_kernel (attention_train_fused.hip; register table in DESIGN.md 7.10) --
// S^T = K . Q^T, so that a LANE holds one query (column) and 16 keys (rows), row maximum and sum are in-lane plus ONE exchange with
// lane ^ 32, and the rounded p is the B operand of O^T += V^T . p^T as it stands (V^T staged in the accumulator's row order) -- with
// the group table, the XCD-aware 1-D work mapping (all query tiles of a (sequence, head) on one XCD, late tiles first) and the
// buffer-descriptor K / V addressing of attention_common.h (one descriptor per head's K and V rows of the sequence: 32-bit byte
// offsets, no 64-bit address arithmetic in the loop; the row is clamped to the sequence besides, so the range check is a second
// line of defence, not the first).  One workgroup = 128 queries (a wavefront owns 32), key tiles of 32 up
// to the diagonal.  The two LDS images are DOUBLE-BUFFERED: the next tile's K / V loads are issued before the current tile's MFMAs
// (unconditionally, with clamped rows: no branch between them and the MFMAs) and the wait for them, with their LDS stores into the
// other buffer, follows the tile's MFMAs (two sched_barriers pin that order; it is what the assembly of all ten variants shows) --
// one barrier per tile.  No dropout, no lse.
// LDS per buffer: K row-major [32][HDP + 8] bf16 (a lane's fragment = one ds_read_b128), V^T [HDP][32 + 8] bf16; HDP = 32 NT >=
// head_dim, NT in {1, 2, 3, 4, 8}; columns in [head_dim, HDP) are staged as zeros.
#include <math.h>
#include "attention_common.h"
#include "bf16x3.h"

namespace r4d {

// slot of row t of a 32-row tile in the transposed image = the order in which the 32 x 32 accumulator holds its rows (register i of
// lane half lh is row (i & 3) + 8 (i >> 2) + 4 lh; registers 8 kk .. 8 kk + 7 are the eight k slots of k-step kk)
__device__ __forceinline__ int ab1_perm32(int t) {
    const int u = t & 15;
    return (t & 16) | (((u >> 2) & 1) << 3) | ((u >> 3) << 2) | (u & 3);
}
__device__ __forceinline__ f32x16 ab1_mfma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ u32x4 ab1_pack8(const float* v) {
    return u32x4{cvt_pk_bf16(v[0], v[1]), cvt_pk_bf16(v[2], v[3]), cvt_pk_bf16(v[4], v[5]), cvt_pk_bf16(v[6], v[7])};
}
// eight consecutive elements as bf16: the bits as they are (QBF), or two 16-byte halves of fp32 rounded
template <bool QBF>
__device__ __forceinline__ u32x4 ab1_bf16x8(u32x4 lo, u32x4 hi) {
    if constexpr (QBF) return lo;
    const f32x4 a = __builtin_bit_cast(f32x4, lo), b = __builtin_bit_cast(f32x4, hi);
    return u32x4{cvt_pk_bf16(a[0], a[1]), cvt_pk_bf16(a[2], a[3]), cvt_pk_bf16(b[0], b[1]), cvt_pk_bf16(b[2], b[3])};
}

// QBF: qkv is bf16 [rows, 3d] behind the pointer (else fp32); out_bf16: out is bf16 [rows, d] (else fp32)
template <int NT, bool QBF>
__global__ __launch_bounds__(256) void attn_b1_kernel(const void* __restrict__ qkv, const AttnGroups G, int d, int H, int hd, int ntq,
                                                      float sd, void* __restrict__ out, int out_bf16) {
    constexpr int HDP = 32 * NT, LDR = HDP + 8, ESZ = QBF ? 2 : 4, NL = QBF ? 1 : 2;
    constexpr int KS = 32 * LDR, BUF = KS + HDP * 40;                  // bf16 elements: K image, one buffer (K image + V^T image)
    constexpr int NITEM = 128 * NT, ITER = (NITEM + 255) / 256;        // (row, 8 columns) items of a 32 x HDP tile; per thread
    extern __shared__ __attribute__((aligned(16))) unsigned short ab1_lds[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, lh = lane >> 5;
    ATTN_TILE_1D_Q(G, H, ntq, 128)                                     // qt, h, seq, gi, T, q0 (the workgroup's first query), rowb
    const int ld3 = 3 * d;
    const char* __restrict__ base = reinterpret_cast<const char*>(qkv) + (rowb * ld3 + (long long)h * hd) * ESZ;     // q of row rowb, this head
    const int seq_bytes = ((T - 1) * ld3 + hd) * ESZ;                  // one head's K (or V) rows of this sequence, as a byte range
    const __amdgpu_buffer_rsrc_t k_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(base + (long long)d * ESZ), 0, seq_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t v_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(base + 2ll * d * ESZ), 0, seq_bytes, 0x00020000);
    const int qw = q0 + 32 * w, qi = qw + r;
    const bool active = qw < T;                                        // wave-uniform
    (void)qt; (void)gi;

    // this lane's query row as the B fragments of S^T: k-step kk holds columns 16 kk + 8 lh .. + 7 (zeros at / past head_dim)
    u32x4 qf[2 * NT];
    {
        const char* qrow = base + (long long)min(qi, T - 1) * ld3 * ESZ;
#pragma unroll
        for (int kk = 0; kk < 2 * NT; ++kk) {
            const int col = 16 * kk + 8 * lh;
            const bool ok = col < hd;
            const u32x4 lo = *reinterpret_cast<const u32x4*>(qrow + (ok ? col : 0) * ESZ);
            const u32x4 hi = QBF ? lo : *reinterpret_cast<const u32x4*>(qrow + (ok ? col : 0) * ESZ + 16);
            qf[kk] = ok ? ab1_bf16x8<QBF>(lo, hi) : u32x4{0u, 0u, 0u, 0u};
        }
    }
    // staging coordinates: item idx = tid + 256 i -> row = idx / (4 NT), eight columns from col = 8 (idx % (4 NT))
    int it_row[ITER], it_col[ITER], it_voff[ITER];
#pragma unroll
    for (int i = 0; i < ITER; ++i) {
        const int idx = tid + 256 * i;
        it_row[i] = idx / (4 * NT);
        it_col[i] = 8 * (idx % (4 * NT));
        it_voff[i] = (idx < NITEM && it_col[i] < hd) ? it_col[i] * ESZ : 0;
    }
    u32x4 kr[ITER][NL], vr[ITER][NL];                                  // one key tile in flight
#define AB1_LOAD(K0)                                                                                                \
    {                                                                                                               \
        /* UNCONDITIONAL (no branch between the loads and the MFMAs they travel under): the row is clamped to the sequence, so */ \
        /* no address leaves its own rows whatever the range check does; a thread without an item, or a tile past the last one, */ \
        /* loads a valid row that is never stored */                                                                \
        _Pragma("unroll") for (int i = 0; i < ITER; ++i) {                                                          \
            const int off_ = min((K0) + it_row[i], T - 1) * ld3 * ESZ + it_voff[i];                                 \
            _Pragma("unroll") for (int j = 0; j < NL; ++j) {                                                        \
                kr[i][j] = __builtin_amdgcn_raw_buffer_load_b128(k_rsrc, off_ + 16 * j, 0, 0);                      \
                vr[i][j] = __builtin_amdgcn_raw_buffer_load_b128(v_rsrc, off_ + 16 * j, 0, 0);                      \
            }                                                                                                       \
        }                                                                                                           \
    }
    // rows at / past T and columns at / past head_dim are zeros BY SELECTION (a clamped row is a copy of row T - 1, a column past
    // head_dim is the next head's)
#define AB1_STORE(K0, BUFP)                                                                                         \
    {                                                                                                               \
        unsigned short* ks_ = (BUFP);                                                                               \
        unsigned short* vt_ = ks_ + KS;                                                                             \
        _Pragma("unroll") for (int i = 0; i < ITER; ++i) {                                                          \
            if (tid + 256 * i < NITEM) {                                                                            \
                const bool ok_ = (K0) + it_row[i] < T && it_col[i] < hd;                                            \
                u32x4 k8_ = ab1_bf16x8<QBF>(kr[i][0], kr[i][NL - 1]), v8_ = ab1_bf16x8<QBF>(vr[i][0], vr[i][NL - 1]); \
                _Pragma("unroll") for (int e = 0; e < 4; ++e) { k8_[e] = ok_ ? k8_[e] : 0u; v8_[e] = ok_ ? v8_[e] : 0u; } \
                *reinterpret_cast<u32x4*>(ks_ + it_row[i] * LDR + it_col[i]) = k8_;                                 \
                unsigned short* t_ = vt_ + it_col[i] * 40 + ab1_perm32(it_row[i]);                                  \
                _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                     \
                    t_[(2 * e) * 40] = (unsigned short)(v8_[e] & 0xffffu);                                          \
                    t_[(2 * e + 1) * 40] = (unsigned short)(v8_[e] >> 16);                                          \
                }                                                                                                   \
            }                                                                                                       \
        }                                                                                                           \
    }

    f32x16 o[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[nt][i] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int kend = min(T, q0 + 128);                                 // keys at / past kend are masked for every query of the workgroup
    AB1_LOAD(0)
    AB1_STORE(0, ab1_lds)
    __syncthreads();
    int cur = 0;
    for (int k0 = 0; k0 < kend; k0 += 32, cur ^= 1) {
        const bool more = k0 + 32 < kend;                              // workgroup-uniform
        AB1_LOAD(k0 + 32)                                              // in flight under this tile's MFMAs (past the last tile: a clamped row, dropped)
        __builtin_amdgcn_sched_barrier(0);                             // the loads stay in front of the tile's work ...
        const unsigned short* Ks = ab1_lds + cur * BUF;
        const unsigned short* Vt = Ks + KS;
        if (active && k0 <= qw + 31) {                                 // wave-uniform: else every key of the tile is right of the wave's queries
            f32x16 s;
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
            for (int kk = 0; kk < 2 * NT; ++kk) s = ab1_mfma(*reinterpret_cast<const u32x4*>(Ks + r * LDR + 16 * kk + 8 * lh), qf[kk], s);
            float p[16];
            float tmax = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) p[i] = s[i] / sd;             // the division for all 16, outside any lane-divergent branch
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = k0 + (i & 3) + 8 * (i >> 2) + 4 * lh;
                p[i] = (key <= qi && key < T) ? p[i] : -INFINITY;
                tmax = fmaxf(tmax, p[i]);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
            const float mn = fmaxf(m, tmax);                           // finite: key 0 is left of every query and in the first tile
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
            const u32x4 pf0 = ab1_pack8(p), pf1 = ab1_pack8(p + 8);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
                for (int i = 0; i < 16; ++i) o[nt][i] *= alpha;
                o[nt] = ab1_mfma(*reinterpret_cast<const u32x4*>(Vt + (32 * nt + r) * 40 + 8 * lh), pf0, o[nt]);
                o[nt] = ab1_mfma(*reinterpret_cast<const u32x4*>(Vt + (32 * nt + r) * 40 + 16 + 8 * lh), pf1, o[nt]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);                             // ... and their LDS stores (with the wait for them) behind it
        if (more) AB1_STORE(k0 + 32, ab1_lds + (cur ^ 1) * BUF)        // last read in the previous iteration: every wave is past that barrier
        __syncthreads();
    }
#undef AB1_STORE
#undef AB1_LOAD
    if (!active || qi >= T) return;
    // acc [NT] (rows = head-dim index, column = the lane's query) -> this head's columns of the query's row
    const float mul = 1.f / l;
    const long long orow = (rowb + qi) * (long long)d + (long long)h * hd;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = 32 * nt + 8 * g + 4 * lh;
            if (c < hd) {
                const float a0 = o[nt][4 * g] * mul, a1 = o[nt][4 * g + 1] * mul, a2 = o[nt][4 * g + 2] * mul, a3 = o[nt][4 * g + 3] * mul;
                if (out_bf16) *reinterpret_cast<u32x2*>(reinterpret_cast<unsigned short*>(out) + orow + c) = u32x2{cvt_pk_bf16(a0, a1), cvt_pk_bf16(a2, a3)};
                else *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out) + orow + c) = f32x4{a0, a1, a2, a3};
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------- host side
static size_t ab1_lds_bytes(int NT) { return (size_t)2 * (32 * (32 * NT + 8) + 32 * NT * 40) * 2; }

bool attention_b1_supported(int H, int d) {
    return H >= 1 && H <= 65535 && d >= 1 && d % H == 0 && (d / H) % 16 == 0 && d / H >= 16 && d / H <= 256;
}

template <int NT, bool QBF>
static int ab1_launch(const void* qkv, const AttnGroups& G, int Tmax, double flop, int H, int d, void* out, bool out_bf16, hipStream_t s) {
    const size_t lds = ab1_lds_bytes(NT);
    if (lds > 48 * 1024) {
        static bool raised = false;
        if (!raised) {
            if (hipFuncSetAttribute((const void*)attn_b1_kernel<NT, QBF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
                set_error("attention_bf16: %zu bytes of LDS refused", lds);
                return R4D_ERR_HIP;
            }
            raised = true;
        }
    }
    int ntq, rc;
    unsigned grid;
    if ((rc = attn_grid_1d("attention_bf16", G, H, Tmax, ntq, grid, 128))) return rc;
    ProfScope prof(PK_ATTN_B1, flop, s);
    hipLaunchKernelGGL((attn_b1_kernel<NT, QBF>), dim3(grid), dim3(256), lds, s, qkv, G, d, H, d / H, ntq, (float)sqrt((double)(d / H)), out,
                       out_bf16 ? 1 : 0);
    R4D_CHECK_LAUNCH("attention_bf16");
    return R4D_OK;
}

int launch_attention_b1_groups(const void* qkv, bool qkv_bf16, int n, const int* Bs, const int* Ts, const long long* row0s, int H, int d,
                               void* out, bool out_bf16, hipStream_t s) {
    R4D_REQUIRE(qkv && out && Bs && Ts && row0s, "attention_bf16: null pointer");
    R4D_REQUIRE(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)out % 16) == 0, "attention_bf16: qkv / out must be 16-byte aligned");
    R4D_REQUIRE(attention_b1_supported(H, d), "attention_bf16: bad shape H=%d d=%d (head_dim %% 16 == 0 in 16 .. 256 wanted)", H, d);
    R4D_REQUIRE(n >= 1 && n <= ATT_MAXG, "attention_bf16: %d batches per launch (1 .. %d wanted)", n, ATT_MAXG);
    for (int g = 0; g < n; ++g)
        R4D_REQUIRE(Bs[g] >= 1 && Ts[g] >= 1 && Ts[g] <= 1024 && row0s[g] >= 0, "attention_bf16: batch %d: B=%d T=%d (B >= 1, T in 1 .. 1024 wanted)", g, Bs[g], Ts[g]);
    AttnGroups G;
    int Tmax, rc;
    double flop;
    if ((rc = attn_groups_fill("attention_bf16", n, Bs, Ts, row0s, H, d, G, Tmax, flop))) return rc;
    const int hd = d / H, NT = hd <= 32 ? 1 : hd <= 64 ? 2 : hd <= 96 ? 3 : hd <= 128 ? 4 : 8;
    if (qkv_bf16) R4D_BRANCH(EBA_BF16);
    else R4D_BRANCH(EBA_F32);
#define AB1_CASE(N) case N: return qkv_bf16 ? ab1_launch<N, true>(qkv, G, Tmax, flop, H, d, out, out_bf16, s) \
                                          : ab1_launch<N, false>(qkv, G, Tmax, flop, H, d, out, out_bf16, s);
    switch (NT) { AB1_CASE(1) AB1_CASE(2) AB1_CASE(3) AB1_CASE(4) default: break; }
    return qkv_bf16 ? ab1_launch<8, true>(qkv, G, Tmax, flop, H, d, out, out_bf16, s) : ab1_launch<8, false>(qkv, G, Tmax, flop, H, d, out, out_bf16, s);
#undef AB1_CASE
}

}  // namespace r4d

using namespace r4d;

extern "C" {

int r4d_attention_bf16_groups(const void* qkv_d, int32_t qkv_is_bf16, int32_t n_groups, const int32_t* Bs, const int32_t* Ts,
                              const int64_t* row0s, int32_t n_head, int32_t d, void* a_d, int32_t out_is_bf16, void* stream) {
    R4D_REQUIRE(n_groups >= 1 && n_groups <= ATT_MAXG && Bs && Ts && row0s, "attention_bf16: %d batches per launch (1 .. %d wanted)", n_groups, ATT_MAXG);
    int B_[ATT_MAXG], T_[ATT_MAXG];
    long long r_[ATT_MAXG];
    for (int g = 0; g < n_groups; ++g) { B_[g] = Bs[g]; T_[g] = Ts[g]; r_[g] = (long long)row0s[g]; }
    return launch_attention_b1_groups(qkv_d, qkv_is_bf16 != 0, n_groups, B_, T_, r_, n_head, d, a_d, out_is_bf16 != 0, (hipStream_t)stream);
}

}  // extern "C"
