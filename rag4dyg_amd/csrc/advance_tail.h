// The tail the two per-sequence choice kernels share (encoder_ops.hip: greedy_advance_kernel, sampling.hip: sample_advance_kernel):
// bookkeeping and stop rules of the reference's decode loops for the token `bi` that thread 0 holds, then -- with `emb.x_out` --
// the first job of the decode step that follows (the chosen token's un-normalised input row) and the clearing of the step's
// split-K ticket counters.  ONE definition, so that a sampled step and a greedy step stop, count and embed alike.
#pragma once
#include "common.h"

namespace r4d {

// called by every thread of the workgroup of sequence b (any workgroup size); s_next / s_pos: two ints of the caller's LDS
__device__ __forceinline__ void advance_tail(int b, int bi, const GreedyState& st, const GreedyEmbed& emb, int* s_next, int* s_pos) {
    const int tid = threadIdx.x, nt = blockDim.x;
    if (b == 0)
        for (int i = tid; i < emb.n_zero; i += nt) emb.zero_words[i] = 0u;
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
    const int id = *s_next, p = *s_pos;
    const bool bad = p < 0 || p >= emb.n_positions || p >= st.t_cap || id < 0 || id >= emb.vocab;   // as embed_pos_ln_kernel: poison, never fault
    const float* src = emb.wte + (long long)(bad ? 0 : id) * emb.d;
    const float* pe = emb.wpe + (long long)(bad ? 0 : p) * emb.d;
    for (int c = tid; c < emb.d; c += nt) emb.x_out[(long long)b * emb.d + c] = bad ? __builtin_nanf("") : src[c] + pe[c];
}

}  // namespace r4d
