// The tail the per-sequence choice kernels share (encoder_ops.hip: greedy_advance_kernel, sampling.hip: sample_advance_kernel,
// beam.hip: beam_advance_kernel): bookkeeping and stop rules of the reference's decode loops for the token `bi` that thread 0 holds,
// then -- with `emb.x_out` -- the first job of the decode step that follows (the chosen token's un-normalised input row) and the
// clearing of the step's split-K ticket counters.  ONE definition, so that a sampled step and a greedy step stop, count and embed
// alike; the beam step has bookkeeping of its own and shares the two jobs for the decode step.
#pragma once
#include "common.h"

namespace r4d {

// the step's split-K ticket counters, cleared by the workgroup of sequence 0 (every thread calls)
__device__ __forceinline__ void advance_clear_tickets(int b, const GreedyEmbed& emb) {
    if (b == 0)
        for (int i = threadIdx.x; i < emb.n_zero; i += blockDim.x) emb.zero_words[i] = 0u;
}

// x_out[row, :] = wte[id] + wpe[p], by every thread of the workgroup
__device__ __forceinline__ void advance_embed_row(int row, int id, int p, int t_cap, const GreedyEmbed& emb) {
    const bool bad = p < 0 || p >= emb.n_positions || p >= t_cap || id < 0 || id >= emb.vocab;   // as embed_pos_ln_kernel: poison, never fault
    const float* src = emb.wte + (long long)(bad ? 0 : id) * emb.d;
    const float* pe = emb.wpe + (long long)(bad ? 0 : p) * emb.d;
    for (int c = threadIdx.x; c < emb.d; c += blockDim.x) emb.x_out[(long long)row * emb.d + c] = bad ? __builtin_nanf("") : src[c] + pe[c];
}

// called by every thread of the workgroup of sequence b (any workgroup size); s_next / s_pos: two ints of the caller's LDS
__device__ __forceinline__ void advance_tail(int b, int bi, const GreedyState& st, const GreedyEmbed& emb, int* s_next, int* s_pos) {
    const int tid = threadIdx.x;
    advance_clear_tickets(b, emb);
    if (tid == 0) {
        int a = st.active[b];
        const int len = st.lens[b];
        if (a) {
            int g = st.gen_len[b];
            if (g < st.out_cap) st.out_tokens[(long long)b * st.out_cap + g] = bi;
            ++g;
            st.gen_len[b] = g;
            const int max_gen = st.params[0], len_limit = min(st.params[1], st.t_cap), n_eos = min(st.params[2], 4);
            bool stop = g >= max_gen || g >= st.out_cap || len + 1 >= len_limit;      // the cache row written next is `len`
            for (int e = 0; e < n_eos; ++e) stop |= bi == st.params[3 + e];
            if (stop) a = 0;
            st.active[b] = a;
        }
        st.next[b] = bi;
        st.pos[b] = a ? len : 0;                 // finished sequences rewrite their row 0: harmless, they are never read again
        st.lens[b] = len + a;
        *s_next = bi; *s_pos = a ? len : 0;
    }
    if (!emb.x_out) return;                      // (uniform per launch)
    __syncthreads();
    advance_embed_row(b, *s_next, *s_pos, st.t_cap, emb);
}

}  // namespace r4d
