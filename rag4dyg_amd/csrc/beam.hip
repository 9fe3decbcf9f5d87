// Greedy beam search on the device (include/r4d.h, "Beam search"): the choice of the next n beams of every prompt in the greedy
// bookkeeping kernel's place in the decode step, and the reordering of the key/value cache that goes with it.  Three kernels:
//
//   beam_rows_kernel     one workgroup of 16 wavefronts per ROW (one beam of one prompt): repetition penalty through the seen bitmap,
//                        m = max, lse = logf(sum expf(x - m)), score = ((x - m) - lse) + beam_score in fp32, and the row's 2n best
//                        (score descending, id ascending) by a radix select on the order-preserving keys, 8 bits a level, with the
//                        sampler's histogram helpers (radix_select.h).  The row is never sorted; only its <= 32 winners are ranked.
//                        The sum behind lse is taken in an order the workgroup's shape fixes (a strided partial per thread, the
//                        butterfly of a wavefront, sixteen wavefront sums in order), so a row's scores depend on the row alone.
//   beam_advance_kernel  one workgroup per PROMPT: the n sorted lists merged into the prompt's 2n best (score descending, flat index
//                        beam * V + id ascending), then the reference's walk over them (modeling_utils.py:1032-1075) with its
//                        BeamHypotheses (:1205-1252) kept in device memory, the in-place reordering of the prompt's rows of
//                        out_tokens and seen, and the two jobs for the decode step that advance_tail.h shares.
//   kv_reorder_kernel    row b n + i of a group receives the K | V lines of row src_row[b n + i], in place: a thread owns one 16-byte
//                        piece of one (layer, group, position) across the group's n rows, loads all n, then stores.
// Rows of up to SAMPLE_LDS_COLS columns keep their keys in LDS; longer rows are re-read (and re-penalised) on every pass.
#include <string.h>
#include "common.h"
#include "advance_tail.h"
#include "radix_select.h"

namespace r4d {

constexpr int BNT = 256;                               // beam_advance_kernel, kv_reorder_kernel

// the row as the beam step sees it (each operation an IEEE fp32 operation of its own; NaN counts as -inf, before and after)
struct BeamRow {
    const float* __restrict__ x; const unsigned* seen; float r, m, lse, bs; bool pen;
    __device__ __forceinline__ float y(int j) const {
        float v = x[j];
        if (pen && ((seen[j >> 5] >> (j & 31)) & 1u)) v = v < 0.f ? v * r : v / r;
        return v;
    }
    __device__ __forceinline__ unsigned ykey(int j) const { return FK::make(y(j)); }
    __device__ __forceinline__ unsigned skey_of(unsigned yk) const { return FK::make(((FK::value(yk) - m) - lse) + bs); }
};
template <bool LDS> __device__ __forceinline__ unsigned beam_key(const BeamRow& row, const unsigned* skey, int j) {
    return LDS ? skey[j] : row.skey_of(row.ykey(j));
}

__device__ __forceinline__ float wave_sum_f32(float v) {       // a butterfly: a + b == b + a, so every lane ends with the same bits
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)v, o); v = t > v ? t : v; }
    return v;
}

template <bool LDS>
__global__ __launch_bounds__(SNT) void beam_rows_kernel(const float* __restrict__ logits, int V, int n, const float* __restrict__ beam_scores,
                                                        const unsigned* __restrict__ seen, const float* __restrict__ fpar,
                                                        float* __restrict__ cand_score, int* __restrict__ cand_id) {
    extern __shared__ unsigned skey[];                 // LDS: the row's keys (of the penalised logits, then of the scores)
    __shared__ u64 hist[256];
    __shared__ u64 seg[SNW];
    __shared__ float fseg[SNW];
    __shared__ unsigned useg[SNW];
    __shared__ SelectOut so;
    __shared__ u64 cand[2 * R4D_BEAM_MAX];
    __shared__ int s_res, s_cnt;
    const int row_i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int nw = (V + 31) >> 5, two_n = 2 * n, kk = min(two_n, V);
    BeamRow row;
    row.x = logits + (long long)row_i * V; row.seen = seen ? seen + (long long)row_i * nw : nullptr; row.r = fpar[1];
    row.pen = row.seen != nullptr && row.r != 1.f; row.bs = beam_scores[row_i]; row.m = 0.f; row.lse = 0.f;

    // keys of the penalised row and the largest of them
    unsigned mk = 0;
#pragma unroll 4
    for (int j = tid; j < V; j += SNT) {
        const unsigned k = row.ykey(j);
        if (LDS) skey[j] = k;
        mk = k > mk ? k : mk;
    }
    mk = wave_max_u32(mk);
    if (lane == 0) useg[wid] = mk;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < SNW; ++w) mk = useg[w] > mk ? useg[w] : mk;
    row.m = FK::value(mk);

    // lse, in the order the workgroup's shape fixes
    float acc = 0.f;
    for (int j = tid; j < V; j += SNT) acc += expf(FK::value(LDS ? skey[j] : row.ykey(j)) - row.m);
    acc = wave_sum_f32(acc);
    if (lane == 0) fseg[wid] = acc;
    __syncthreads();
    float total = fseg[0];
#pragma unroll
    for (int w = 1; w < SNW; ++w) total += fseg[w];
    row.lse = logf(total);
    if (LDS) {
        for (int j = tid; j < V; j += SNT) skey[j] = row.skey_of(skey[j]);     // (each thread rewrites the entries it wrote)
        __syncthreads();
    }

    // the key of rank kk - 1 (ties counted) and the number of keys above it
    unsigned K = 0;                                    // kk == V: every key is above key 0
    int jcut = 0x7fffffff;
    if (kk < V) {
        unsigned prefix = 0, mask = 0;
        u64 above = 0, ties = 0;
        bool ok = true;
        for (int shift = 24; shift >= 0 && ok; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int base = 0; base < V; base += SNT) {
                const int j = base + tid;
                bool valid = j < V;
                unsigned k = 0;
                if (valid) { k = beam_key<LDS>(row, skey, j); valid = (k & mask) == prefix; }
                hist_add<false>(hist, valid, (int)((k >> shift) & 255u), 0ull, lane);
            }
            __syncthreads();
            if (wid == 0) find_bucket(hist, (u64)(kk - 1) - above, false, 0.f, &so, lane);
            __syncthreads();
            const int bucket = so.bucket;
            if (bucket < 0) ok = false;                // (cannot happen: the keys that match the prefix outnumber the target)
            else { above += so.above; ties = so.bmass; prefix |= (unsigned)bucket << shift; mask |= 255u << shift; }
            __syncthreads();
        }
        if (ok) {
            K = prefix;
            const u64 need = (u64)kk - above;          // of the keys == K, the lowest ids
            if (need < ties) {
                const int L = (((V + SNW - 1) / SNW) + 63) / 64 * 64;
                auto is_tie = [&](int j) -> u64 { return beam_key<LDS>(row, skey, j) == K ? 1ull : 0ull; };
                seg_sums(V, L, is_tie, seg);
                jcut = seg_find(V, L, is_tie, need - 1, seg, &s_res);
                __syncthreads();
            }
        }
    }

    // the winners, then their ranks among themselves
    for (int j = tid; j < V; j += SNT) {
        const unsigned k = beam_key<LDS>(row, skey, j);
        if (k > K || (k == K && K != 0u && j <= jcut)) {
            const int slot = atomicAdd(&s_cnt, 1);
            if (slot < 2 * R4D_BEAM_MAX) cand[slot] = ((u64)k << 32) | (0xffffffffu - (unsigned)j);
        }
    }
    __syncthreads();
    const int got = min(s_cnt, kk);
    if (tid < two_n) {
        float* os = cand_score + (long long)row_i * two_n;
        int* oi = cand_id + (long long)row_i * two_n;
        if (tid < got) {
            const u64 me = cand[tid];
            int rank = 0;
            for (int i = 0; i < got; ++i) rank += cand[i] > me ? 1 : 0;
            os[rank] = FK::value((unsigned)(me >> 32));
            oi[rank] = (int)(0xffffffffu - (unsigned)me);
        } else {                                       // V < 2n (or a select that failed): the list's unused tail
            os[tid] = -INFINITY;
            oi[tid] = -1;
        }
    }
}

// hypotheses of one prompt, in LDS while thread 0 walks the candidates
struct HypAdd { int slot, src; };

__global__ __launch_bounds__(BNT) void beam_advance_kernel(int V, BeamArgs ba, GreedyState st, GreedyEmbed emb, int advance) {
    __shared__ u64 pk[2 * R4D_BEAM_MAX * R4D_BEAM_MAX];
    __shared__ float m_score[2 * R4D_BEAM_MAX];
    __shared__ int m_flat[2 * R4D_BEAM_MAX];
    __shared__ double h_score[R4D_BEAM_MAX];
    __shared__ int h_seq[R4D_BEAM_MAX];
    __shared__ HypAdd adds[2 * R4D_BEAM_MAX];
    __shared__ int n_src[R4D_BEAM_MAX], n_tok[R4D_BEAM_MAX], n_pos[R4D_BEAM_MAX];
    __shared__ float n_sc[R4D_BEAM_MAX];
    __shared__ int s_nadd, s_state, s_g, s_len, s_act;
    const int b = blockIdx.x, tid = threadIdx.x, n = ba.n, two_n = 2 * n, L = min(two_n, V), N = n * L, row0 = b * n;
    if (advance) advance_clear_tickets(b, emb);
    const bool was_active = advance ? st.active[row0] != 0 : true;        // (uniform: every thread reads the same word)

    // merge: the rank of every candidate among the prompt's n L (all packs differ: the flat index is part of them)
    if (was_active) {
        for (int c = tid; c < N; c += BNT) {
            const int beam = c / L, i = c - beam * L;
            const int id = ba.cand_id[(long long)(row0 + beam) * two_n + i];
            const unsigned k = FK::make(ba.cand_score[(long long)(row0 + beam) * two_n + i]);
            pk[c] = ((u64)k << 32) | (0xffffffffu - (unsigned)(beam * V + id));
        }
        __syncthreads();
        for (int c = tid; c < N; c += BNT) {
            const u64 me = pk[c];
            const int beam = c / L, i = c - beam * L;
            int rank = i;                              // every list is sorted: its own place, then the heads of the others
            for (int ob = 0; ob < n; ++ob) {
                if (ob == beam) continue;
                const u64* lst = pk + ob * L;
                for (int o = 0; o < L && lst[o] > me; ++o) ++rank;
            }
            if (rank < two_n) {
                const float sc = FK::value((unsigned)(me >> 32));
                const int flat = (int)(0xffffffffu - (unsigned)me);
                m_score[rank] = sc; m_flat[rank] = flat;
                if (!advance) { ba.out_score[(long long)b * two_n + rank] = sc; ba.out_flat[(long long)b * two_n + rank] = flat; }
            }
        }
    }
    if (!advance) return;
    __syncthreads();

    // the reference's walk, by thread 0
    if (tid == 0) {
        const int g = st.gen_len[row0], len = st.lens[row0];
        int state = 0, nadd = 0, act = 0;              // state 0: inactive on entry, 1: done at this step, 2: stepped
        if (was_active) {
            const int max_gen = st.params[0], len_limit = min(st.params[1], st.t_cap), n_eos = min(st.params[2], 4), T = st.params[7];
            const double lp = (double)ba.fpar[0];
            int cnt = ba.hyp_count[b], added = ba.hyp_added[b];
            double worst = ba.worst[b];
            for (int i = 0; i < cnt; ++i) { h_score[i] = ba.hyp_score[row0 + i]; h_seq[i] = ba.hyp_seq[row0 + i]; }
            const bool done = cnt >= n && worst >= (double)m_score[0] / pow((double)(T + max_gen - 1), lp);
            if (done) {
                state = 1;
                ba.done[b] = 1;
            } else {
                state = 2;
                const int cur_len = T + g;
                const double div = pow((double)cur_len, lp);
                int k = 0;
                for (int c = 0; c < two_n && k < n; ++c) {
                    const float s = m_score[c];
                    const int flat = m_flat[c], beam = flat / V, tok = flat - beam * V;
                    bool eos = false;
                    for (int e = 0; e < n_eos; ++e) eos |= tok == st.params[3 + e];
                    if (!eos) { n_src[k] = beam; n_tok[k] = tok; n_sc[k] = s; ++k; continue; }
                    const double score = (double)s / div;
                    if (cnt < n) {
                        h_score[cnt] = score; h_seq[cnt] = added++;
                        adds[nadd++] = HypAdd{cnt, beam};
                        ++cnt;
                        worst = score < worst ? score : worst;
                    } else if (score > worst) {        // the lowest (score, list index) leaves; worst = the lowest that stays
                        int lo = 0;
                        for (int i = 1; i < n; ++i)
                            if (h_score[i] < h_score[lo] || (h_score[i] == h_score[lo] && h_seq[i] < h_seq[lo])) lo = i;
                        h_score[lo] = score; h_seq[lo] = added++;
                        adds[nadd++] = HypAdd{lo, beam};
                        worst = h_score[0];
                        for (int i = 1; i < n; ++i) worst = h_score[i] < worst ? h_score[i] : worst;
                    }
                }
                if (k < n) ba.status[b] |= 1;         // the reference asserts "Beam should always be full"
                for (; k < n; ++k) { n_src[k] = k; n_tok[k] = 0; n_sc[k] = -INFINITY; }
                for (int i = 0; i < nadd; ++i) {
                    const int slot = adds[i].slot;
                    ba.hyp_score[row0 + slot] = h_score[slot]; ba.hyp_seq[row0 + slot] = h_seq[slot]; ba.hyp_len[row0 + slot] = g;
                }
                ba.hyp_count[b] = cnt; ba.hyp_added[b] = added; ba.worst[b] = worst;
                act = !(g + 1 >= max_gen || g + 1 >= st.out_cap || len + 1 >= len_limit);      // the cache row written next is `len`
            }
        }
        ba.group_active[b] = state == 2;
        ba.lo[b] = st.params[7];
        ba.hi[b] = state == 2 ? len : st.params[7];
        s_nadd = nadd; s_state = state; s_g = g; s_len = len; s_act = act;
    }
    __syncthreads();
    const int state = s_state, g = s_g, len = s_len, act = s_act, gcopy = min(g, st.out_cap);
    if (state == 2) {
        // finished hypotheses: the source beam's ids so far (a thread owns a column here and in the reordering below)
        for (int r = 0; r < s_nadd; ++r) {
            const int* src = st.out_tokens + (long long)(row0 + adds[r].src) * st.out_cap;
            int* dst = ba.hyp_ids + (long long)(row0 + adds[r].slot) * st.out_cap;
            for (int c = tid; c < gcopy; c += BNT) dst[c] = src[c];
        }
        for (int c = tid; c < gcopy; c += BNT) {
            int v[R4D_BEAM_MAX];
#pragma unroll
            for (int i = 0; i < R4D_BEAM_MAX; ++i) if (i < n) v[i] = st.out_tokens[(long long)(row0 + n_src[i]) * st.out_cap + c];
#pragma unroll
            for (int i = 0; i < R4D_BEAM_MAX; ++i) if (i < n) st.out_tokens[(long long)(row0 + i) * st.out_cap + c] = v[i];
        }
        if (ba.seen) {
            const int nw = (V + 31) >> 5;
            for (int w = tid; w < nw; w += BNT) {
                unsigned v[R4D_BEAM_MAX];
#pragma unroll
                for (int i = 0; i < R4D_BEAM_MAX; ++i) if (i < n) v[i] = ba.seen[(long long)(row0 + n_src[i]) * nw + w];
#pragma unroll
                for (int i = 0; i < R4D_BEAM_MAX; ++i)
                    if (i < n) ba.seen[(long long)(row0 + i) * nw + w] = v[i] | ((n_tok[i] >> 5) == w ? 1u << (n_tok[i] & 31) : 0u);
            }
        }
    }
    if (tid < n) {
        const int row = row0 + tid;
        int p = 0;
        if (state == 2) {
            if (g < st.out_cap) st.out_tokens[(long long)row * st.out_cap + g] = n_tok[tid];
            ba.beam_scores[row] = n_sc[tid];
            ba.beam_idx[row] = row0 + n_src[tid];
            st.next[row] = n_tok[tid];
            st.gen_len[row] = g + 1;
            st.active[row] = act;
            st.lens[row] = len + act;
            p = act ? len : 0;                         // finished rows rewrite their position 0: never read again
        } else {
            ba.beam_idx[row] = row;
            n_tok[tid] = (int)st.next[row];
            if (state == 1) st.active[row] = 0;
        }
        st.pos[row] = p;
        n_pos[tid] = p;
    }
    if (!emb.x_out) return;                            // (uniform per launch)
    __syncthreads();
    for (int i = 0; i < n; ++i) advance_embed_row(row0 + i, n_tok[i], n_pos[i], st.t_cap, emb);
}

__global__ __launch_bounds__(BNT) void kv_reorder_kernel(float* __restrict__ kv, const int* __restrict__ src_row, const int* __restrict__ lo,
                                                         const int* __restrict__ hi, const int* __restrict__ active, int R, int n,
                                                         int t_cap, int d2) {
    const int p = blockIdx.x, b = blockIdx.y, l = blockIdx.z, row0 = b * n;
    if (active && !active[b]) return;
    if (p < lo[b] || p >= hi[b]) return;
    int src[R4D_BEAM_MAX];
    unsigned bad = 0, moved = 0;
#pragma unroll
    for (int i = 0; i < R4D_BEAM_MAX; ++i) {
        src[i] = row0 + i;
        if (i < n) {
            const int s = src_row[row0 + i];
            if (s < row0 || s >= row0 + n) bad |= 1u << i;            // outside the group: the row is poisoned, nothing is read there
            else { src[i] = s; if (s != row0 + i) moved |= 1u << i; }
        }
    }
    if (!(bad | moved)) return;
    const int pieces = d2 >> 2;
    const float qn = __builtin_nanf("");
    for (int c = threadIdx.x; c < pieces; c += BNT) {
        float4 v[R4D_BEAM_MAX];
#pragma unroll
        for (int i = 0; i < R4D_BEAM_MAX; ++i)
            if (i < n) v[i] = *reinterpret_cast<const float4*>(kv + (((size_t)l * R + src[i]) * t_cap + p) * d2 + 4 * (size_t)c);
#pragma unroll
        for (int i = 0; i < R4D_BEAM_MAX; ++i)
            if (i < n && ((bad | moved) >> i & 1u))
                *reinterpret_cast<float4*>(kv + (((size_t)l * R + row0 + i) * t_cap + p) * d2 + 4 * (size_t)c) =
                    (bad >> i & 1u) ? make_float4(qn, qn, qn, qn) : v[i];
    }
}

int beam_rows_prepare() {
    R4D_HIP(hipFuncSetAttribute((const void*)beam_rows_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                SAMPLE_LDS_COLS * (int)sizeof(unsigned)));
    return R4D_OK;
}

static bool capturing(hipStream_t s) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (s) (void)hipStreamIsCapturing(s, &cap);
    return cap != hipStreamCaptureStatusNone;
}

int launch_beam_rows(const float* logits, int R, int V, const BeamArgs& ba, hipStream_t s) {
    R4D_REQUIRE(logits && ba.beam_scores && ba.fpar && ba.cand_score && ba.cand_id, "beam rows: null pointer");
    R4D_REQUIRE(ba.n >= 2 && ba.n <= R4D_BEAM_MAX && V >= 2 && R >= 1 && R % ba.n == 0, "beam rows: n=%d V=%d rows=%d", ba.n, V, R);
    R4D_REQUIRE((long long)ba.n * V < (1LL << 31), "beam rows: n V = %lld does not fit the flat index", (long long)ba.n * V);
    const bool lds = V <= SAMPLE_LDS_COLS;
    if (lds && !capturing(s)) {                        // (a capturing caller has prepared: encoder.hip, capture_step)
        const int rc = beam_rows_prepare();
        if (rc) return rc;
    }
    ProfScope prof(PK_BEAM_ROWS, 4.0 * R * (double)V, s);
    if (lds) {
        R4D_BRANCH(BEAM_LDS);
        hipLaunchKernelGGL(beam_rows_kernel<true>, dim3(R), dim3(SNT), (size_t)V * sizeof(unsigned), s, logits, V, ba.n, ba.beam_scores, ba.seen,
                           ba.fpar, ba.cand_score, ba.cand_id);
    } else {
        R4D_BRANCH(BEAM_GLOBAL);
        hipLaunchKernelGGL(beam_rows_kernel<false>, dim3(R), dim3(SNT), 0, s, logits, V, ba.n, ba.beam_scores, ba.seen, ba.fpar, ba.cand_score,
                           ba.cand_id);
    }
    R4D_CHECK_LAUNCH("beam_rows");
    return R4D_OK;
}

int launch_beam_advance(int B0, int V, const BeamArgs& ba, const GreedyState* st, const GreedyEmbed* embed, hipStream_t s) {
    R4D_REQUIRE(ba.cand_score && ba.cand_id && ba.n >= 2 && ba.n <= R4D_BEAM_MAX && V >= 2, "beam advance: bad arguments");
    GreedyState g;
    GreedyEmbed e;
    memset(&g, 0, sizeof(g));
    memset(&e, 0, sizeof(e));
    if (st) {
        g = *st;
        R4D_REQUIRE(g.next && g.lens && g.pos && g.active && g.gen_len && g.out_tokens && g.params, "beam advance: null pointer");
        R4D_REQUIRE(g.out_cap >= 1 && g.t_cap >= 1, "beam advance: out_cap=%d t_cap=%d", g.out_cap, g.t_cap);
        R4D_REQUIRE(ba.fpar && ba.beam_scores && ba.beam_idx && ba.lo && ba.hi && ba.group_active && ba.done && ba.hyp_count && ba.hyp_added &&
                    ba.status && ba.worst && ba.hyp_score && ba.hyp_len && ba.hyp_seq && ba.hyp_ids, "beam advance: null pointer");
        if (embed) {
            e = *embed;
            R4D_REQUIRE(e.wte && e.wpe && e.x_out && e.d >= 1, "beam advance: bad embedding arguments");
        }
    } else {
        R4D_REQUIRE(ba.out_score && ba.out_flat, "beam advance: null pointer");
    }
    if (B0 <= 0) return R4D_OK;
    ProfScope prof(PK_BEAM_ADVANCE, 8.0 * B0 * ba.n * 2.0 * ba.n, s);
    hipLaunchKernelGGL(beam_advance_kernel, dim3(B0), dim3(BNT), 0, s, V, ba, g, e, st ? 1 : 0);
    R4D_CHECK_LAUNCH("beam_advance");
    return R4D_OK;
}

int launch_kv_reorder(float* kv, const int* src_row, const int* lo, const int* hi, const int* active, int n_layer, int B0, int n, int t_cap,
                      int d, hipStream_t s) {
    R4D_REQUIRE(kv && src_row && lo && hi, "kv reorder: null pointer");
    R4D_REQUIRE(n_layer >= 1 && n_layer <= 65535 && B0 >= 0 && B0 <= 65535 && n >= 1 && n <= R4D_BEAM_MAX && t_cap >= 1 && d >= 2 && d % 2 == 0,
                "kv reorder: n_layer=%d B0=%d n=%d t_cap=%d d=%d", n_layer, B0, n, t_cap, d);
    if (B0 == 0) return R4D_OK;
    ProfScope prof(PK_KV_REORDER, 0.0, s);            // (the bytes moved depend on ranges only the device knows: time alone)
    // (the range is known on the device only, so the grid covers the cache: below some 64 generated positions the workgroups that
    // leave at once, not the copy, set the launch's time -- profiles/beam_search.md)
    hipLaunchKernelGGL(kv_reorder_kernel, dim3(t_cap, B0, n_layer), dim3(BNT), 0, s, kv, src_row, lo, hi, active, B0 * n, n, t_cap, 2 * d);
    R4D_CHECK_LAUNCH("kv_reorder");
    return R4D_OK;
}

}  // namespace r4d

using namespace r4d;

extern "C" int r4d_beam_select_f32(const float* logits_d, const float* beam_scores_d, const uint32_t* seen_d, const float* fparams_d,
                                   int32_t B0, int32_t n_beams, int32_t V, float* cand_scores_d, int32_t* cand_ids_d, float* out_scores_d,
                                   int32_t* out_index_d, void* stream) {
    R4D_REQUIRE(B0 >= 0 && n_beams >= 2 && n_beams <= R4D_BEAM_MAX, "beam_select: B0=%d n_beams=%d", B0, n_beams);
    R4D_REQUIRE(out_scores_d && out_index_d, "beam_select: null pointer");
    if (B0 == 0) return R4D_OK;
    BeamArgs ba;
    memset(&ba, 0, sizeof(ba));
    ba.n = n_beams; ba.seen = const_cast<uint32_t*>(seen_d); ba.fpar = fparams_d; ba.beam_scores = const_cast<float*>(beam_scores_d);
    ba.cand_score = cand_scores_d; ba.cand_id = cand_ids_d; ba.out_score = out_scores_d; ba.out_flat = out_index_d;
    const int rc = launch_beam_rows(logits_d, B0 * n_beams, V, ba, (hipStream_t)stream);
    if (rc) return rc;
    return launch_beam_advance(B0, V, ba, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int r4d_kv_cache_reorder_f32(float* kv_cache_d, const int32_t* src_row_d, const int32_t* lo_d, const int32_t* hi_d,
                                        const int32_t* active_d, int32_t n_layer, int32_t B0, int32_t n, int32_t t_cap, int32_t d,
                                        void* stream) {
    return launch_kv_reorder(kv_cache_d, src_row_d, lo_d, hi_d, active_d, n_layer, B0, n, t_cap, d, (hipStream_t)stream);
}
