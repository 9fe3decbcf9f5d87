// The sampled choice of the next token (include/r4d.h, "Sampled decoding"): repetition penalty, temperature, top-k, top-p and
// one Philox draw per sequence, in the greedy bookkeeping kernel's place in the decode step.  One workgroup of 16 wavefronts
// owns one row of logits; nothing is handed from workgroup to workgroup.
//
// Every selection is a radix select on the order-preserving keys of topk_key.h, 8 bits a level: top-k counts the keys of a
// bucket, top-p adds their WEIGHT.  Weights are 64-bit fixed point, floor(expf(y - max) * 2^40), and all sums are integer sums:
// exact in that unit and the same in any order, so LDS atomics may build the histograms and the token still depends on the row
// alone (no floating-point sum anywhere; the quantum 2^-40 per entry is far below fp32's own rounding of expf).  Only two
// questions need INDEX order -- which of several equal keys on the top-p cut stay, and where u * Z falls -- and both are one
// routine: sixteen contiguous segments summed by one wavefront each, then the one segment that holds the target searched by its
// wavefront, a contiguous chunk per lane.
// Rows of up to SAMPLE_LDS_COLS columns keep their keys in LDS; longer rows are re-read (and re-penalised) on every pass.
#include <string.h>
#include "common.h"
#include "advance_tail.h"
#include "philox.h"
#include "radix_select.h"

namespace r4d {

// the row as the sampler sees it: penalised, divided by the temperature (each an IEEE fp32 operation of its own)
struct SampleRow {
    const float* __restrict__ x; const unsigned* seen; float r, tau; bool pen, temp;
    __device__ __forceinline__ float y(int j) const {
        float v = x[j];
        if (pen && ((seen[j >> 5] >> (j & 31)) & 1u)) v = v < 0.f ? v * r : v / r;
        if (temp) v = v / tau;
        return v;
    }
};
template <bool LDS> __device__ __forceinline__ unsigned row_key(const SampleRow& row, const unsigned* skey, int j) {
    return LDS ? skey[j] : FK::make(row.y(j));
}
// fixed-point weight of a key against the row maximum (finite): at most 2^40; NaN and -inf give 0
__device__ __forceinline__ u64 weight_fix(unsigned key, float ymax) { return (u64)(expf(FK::value(key) - ymax) * 1099511627776.f); }

// Radix select over the keys >= thr of the row, called by the whole workgroup.  MASS = false: the key of rank `target` (0 = the
// largest), ties counted.  MASS = true: the key K in whose run of equal keys the weight, summed from the largest key down, first
// exceeds P = floor(top_p * all weight); *above = the weight of the keys > K, *bmass that of the keys == K.  Returns false when no
// such key exists.
template <bool LDS, bool MASS>
__device__ bool radix_select(const SampleRow& row, const unsigned* skey, int V, unsigned thr, u64 target, float top_p, float ymax,
                             u64* hist, SelectOut* so, unsigned* K, u64* above_out, u64* bmass_out, u64* target_out) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    unsigned prefix = 0, mask = 0;
    u64 above = 0, bmass = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int base = 0; base < V; base += SNT) {
            const int j = base + tid;
            bool valid = j < V;
            unsigned k = 0;
            if (valid) { k = row_key<LDS>(row, skey, j); valid = k >= thr && (k & mask) == prefix; }
            hist_add<MASS>(hist, valid, (int)((k >> shift) & 255u), (MASS && valid) ? weight_fix(k, ymax) : 0ull, lane);
        }
        __syncthreads();
        if (wid == 0) find_bucket(hist, target - above, MASS && shift == 24, top_p, so, lane);
        __syncthreads();
        const int bucket = so->bucket;
        if (MASS && shift == 24) target = so->target;
        if (bucket < 0) { __syncthreads(); return false; }
        above += so->above; bmass = so->bmass;
        prefix |= (unsigned)bucket << shift; mask |= 255u << shift;
        __syncthreads();
    }
    *K = prefix; *above_out = above; *bmass_out = bmass; *target_out = target;
    return true;
}

template <bool LDS>
__global__ __launch_bounds__(SNT) void sample_advance_kernel(const float* __restrict__ logits, int V, SampleArgs sa, GreedyState st,
                                                             GreedyEmbed emb, int advance) {
    extern __shared__ unsigned skey[];                 // LDS: the row's keys
    __shared__ u64 hist[256];
    __shared__ u64 seg[SNW];
    __shared__ SelectOut so;
    __shared__ int s_res, s_next, s_pos;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int nw = (V + 31) >> 5;
    const int do_sample = sa.ipar[0], top_k = sa.ipar[1];
    const float tau = sa.fpar[0], top_p = sa.fpar[1], rep = sa.fpar[2];
    SampleRow row;
    row.x = logits + (long long)b * V; row.seen = sa.seen ? sa.seen + (long long)b * nw : nullptr; row.r = rep; row.tau = tau;
    row.pen = row.seen != nullptr && rep != 1.f; row.temp = do_sample != 0 && tau != 1.f;

    // keys, the largest key and its lowest index
    u64 best = 0;
#pragma unroll 4
    for (int j = tid; j < V; j += SNT) {
        const unsigned k = FK::make(row.y(j));
        if (LDS) skey[j] = k;
        const u64 pack = ((u64)k << 32) | (0xffffffffu - (unsigned)j);
        best = pack > best ? pack : best;
    }
    best = wave_max64(best);
    if (lane == 0) seg[wid] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < SNW; ++w) best = seg[w] > best ? seg[w] : best;
    __syncthreads();
    const unsigned maxkey = (unsigned)(best >> 32);
    int tok = (int)(0xffffffffu - (unsigned)best);
    const float ymax = FK::value(maxkey);

    // the draw's uniform (every thread: the inputs are uniform)
    const int step = advance ? st.gen_len[b] : sa.step[b];
    const uint4 ph = philox4x32_10(make_uint4((unsigned)step, (unsigned)sa.stream[b], 0u, R4D_SAMPLE_PHILOX_SITE),
                                   make_uint2((unsigned)sa.ipar[2], (unsigned)sa.ipar[3]));
    const unsigned u24 = ph.x >> 8;

    unsigned thr = 0, Kc = 0;                          // kept: key >= thr and (key > Kc or (key == Kc and j <= jcut))
    int jcut = 0x7fffffff;
    const bool simple = !do_sample || !(fabsf(ymax) < INFINITY);      // argmax, or a row whose maximum is +-inf: the kept set is `tok`
    if (!simple) {
        const int L = (((V + SNW - 1) / SNW) + 63) / 64 * 64;
        u64 above = 0, bmass = 0, target = 0;
        if (top_k > 0) {
            const int kk = min(max(top_k, 1), V);
            if (kk < V) {
                radix_select<LDS, false>(row, skey, V, 0u, (u64)(kk - 1), 0.f, ymax, hist, &so, &thr, &above, &bmass, &target);
            }
        }
        if (top_p < 1.f && radix_select<LDS, true>(row, skey, V, thr, 0ull, top_p, ymax, hist, &so, &Kc, &above, &bmass, &target)) {
            const u64 qs = weight_fix(Kc, ymax);
            if (qs > 0) {
                const u64 n_keep = (target - above) / qs + 1, cnt = bmass / qs;       // of the keys == Kc, in index order
                if (n_keep < cnt) {
                    auto is_tie = [&](int j) -> u64 { return row_key<LDS>(row, skey, j) == Kc ? 1ull : 0ull; };
                    seg_sums(V, L, is_tie, seg);
                    jcut = seg_find(V, L, is_tie, n_keep - 1, seg, &s_res);
                    __syncthreads();
                }
            }
        }
        auto kept_w = [&](int j) -> u64 {
            const unsigned k = row_key<LDS>(row, skey, j);
            return (k >= thr && (k > Kc || (k == Kc && j <= jcut))) ? weight_fix(k, ymax) : 0ull;
        };
        const u64 Z = seg_sums(V, L, kept_w, seg);
        const u64 T = (Z >> 24) * u24 + (((Z & 0xffffffull) * u24) >> 24);            // floor(Z * u24 / 2^24) < Z
        const int j = seg_find(V, L, kept_w, T, seg, &s_res);
        if (j >= 0) tok = j;
    }
    if (sa.out_keep) {
        unsigned* keep = sa.out_keep + (long long)b * nw;
        for (int base = 0; base < V; base += SNT) {
            const int j = base + tid;
            bool in = false;
            if (j < V) {
                if (simple) in = j == tok;
                else { const unsigned k = row_key<LDS>(row, skey, j); in = k >= thr && (k > Kc || (k == Kc && j <= jcut)); }
            }
            const u64 m = __ballot(in);
            if ((lane & 31) == 0 && (j >> 5) < nw) keep[j >> 5] = (unsigned)(lane ? m >> 32 : m);
        }
    }
    __syncthreads();                                   // every read of the seen words is behind us
    if (tid == 0) {
        if (sa.out_u) sa.out_u[b] = (float)u24 * 5.9604644775390625e-8f;
        if (row.seen && (!advance || st.active[b])) sa.seen[(long long)b * nw + (tok >> 5)] |= 1u << (tok & 31);   // the row is this workgroup's alone
        if (!advance) sa.out_token[b] = tok;
    }
    if (advance) advance_tail(b, tok, st, emb, &s_next, &s_pos);
}

// the LDS kernel's dynamic-LDS limit, on the CURRENT device: set at every call (a host-side attribute, no launch) -- a per-process
// flag would leave a second GPU of the process without it, and need a lock
int sample_advance_prepare() {
    R4D_HIP(hipFuncSetAttribute((const void*)sample_advance_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                SAMPLE_LDS_COLS * (int)sizeof(unsigned)));
    return R4D_OK;
}

int launch_sample_advance(const float* logits, int B, int V, const SampleArgs& sa, const GreedyState* st, hipStream_t s,
                          const GreedyEmbed* embed) {
    R4D_REQUIRE(logits && sa.stream && sa.fpar && sa.ipar, "sample advance: null pointer");
    R4D_REQUIRE(V >= 1, "sample advance: V=%d", V);
    GreedyState g;
    memset(&g, 0, sizeof(g));
    if (st) {
        g = *st;
        R4D_REQUIRE(g.next && g.lens && g.pos && g.active && g.gen_len && g.out_tokens && g.params, "sample advance: null pointer");
        R4D_REQUIRE(g.out_cap >= 1 && g.t_cap >= 1, "sample advance: out_cap=%d t_cap=%d", g.out_cap, g.t_cap);
    } else {
        R4D_REQUIRE(sa.step && sa.out_token, "sample advance: null pointer");
    }
    if (B <= 0) return R4D_OK;
    GreedyEmbed e;
    memset(&e, 0, sizeof(e));
    if (embed) {
        e = *embed;
        R4D_REQUIRE(st && e.wte && e.wpe && e.x_out && e.d >= 1, "sample advance: bad embedding arguments");
    }
    const bool lds = V <= SAMPLE_LDS_COLS;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (s) (void)hipStreamIsCapturing(s, &cap);
    if (lds && cap == hipStreamCaptureStatusNone) {      // (a capturing caller has prepared: encoder.hip, capture_step)
        const int rc = sample_advance_prepare();
        if (rc) return rc;
    }
    ProfScope prof(PK_SAMPLE_ADVANCE, 4.0 * B * (double)V, s);
    if (lds) {
        R4D_BRANCH(SAMPLE_LDS);
        hipLaunchKernelGGL(sample_advance_kernel<true>, dim3(B), dim3(SNT), (size_t)V * sizeof(unsigned), s, logits, V, sa, g, e, st ? 1 : 0);
    } else {
        R4D_BRANCH(SAMPLE_GLOBAL);
        hipLaunchKernelGGL(sample_advance_kernel<false>, dim3(B), dim3(SNT), 0, s, logits, V, sa, g, e, st ? 1 : 0);
    }
    R4D_CHECK_LAUNCH("sample_advance");
    return R4D_OK;
}

}  // namespace r4d

using namespace r4d;

extern "C" int r4d_sample_logits_f32(const float* logits_d, int32_t B, int32_t V, uint32_t* seen_d, const int32_t* step_d,
                                     const int32_t* stream_d, const float* fparams_d, const int32_t* iparams_d, int64_t* out_token_d,
                                     uint32_t* out_keep_d, float* out_u_d, void* stream) {
    R4D_REQUIRE(B >= 0, "sample_logits: B=%d", B);
    const SampleArgs sa{seen_d, step_d, stream_d, fparams_d, iparams_d, out_token_d, out_keep_d, out_u_d};
    return launch_sample_advance(logits_d, B, V, sa, nullptr, (hipStream_t)stream);
}
