// RAG GENERATOR TRAINING on gfx950 (train/train_generator.py, utils/model.py:105-224): one step on a SPLICED input -- the
// fusion rows of the retrieved neighbourhood placed after position 2 of every sequence --, plus the gather / scatter kernels of
// the one-layer graph-pooling fusion.
//
//   splice_embed_ln4_kernel   x_in[b, t] = (aug_ids[b, t] == -100 ? fused[b, t - 2] : wte[aug_ids[b, t]]) + wpe[t]; ln_1 of it
//   r4d_rag_train_step_f32    training forward (train.hip) -> LM head, CE on aug_ids, dh, dW_head (lm_head.hip: head_train_step)
//                             -> backward (frozen: data gradients only) -> d_fused = gradient of the spliced rows
//   weighted_bag_kernel       P[q] = sum_{j in span q} c_j wte[nodes_j]   (mean over nodes of A_norm X = c^T X per query)
//   scatter_fix_kernel        out[ids[k]] = sum_k w_k src[row_of[k]]      (64-bit fixed point, as the embedding backward)
//
// One int64 array aug_ids [B, Ta] (-100 at the fused positions) is the splice, the CE labels (ignore_index -100: lm_ce skips it) and
// the wte scatter (embedding_bwd_kernel skips negative ids).  Every sum runs in a fixed order or through the fixed-point table:
// no float atomics, the same bits on every launch.
#include <string.h>
#include "common.h"

namespace r4d {

__device__ __forceinline__ float rag_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one wave per row, 16-byte lanes (d % 64 == 0: lanes past d / 4 idle); the sums in embed_ln4_groups_kernel's order
template <int NQ>
__global__ __launch_bounds__(256) void splice_embed_ln4_kernel(const int64_t* __restrict__ ids, const float* __restrict__ fused, int r,
                                                               const float* __restrict__ wte, const float* __restrict__ wpe, int vocab,
                                                               long long rows, int T, int d, const float* __restrict__ w,
                                                               const float* __restrict__ b, float eps, float* __restrict__ x_out,
                                                               float* __restrict__ y_out) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long long seq = row / T;
    const int t = (int)(row - seq * T), j = t - 2;
    const long long id = ids[row];
    const bool fz = id == -100 && j >= 0 && j < r;
    const bool bad = !fz && (id < 0 || id >= vocab);             // a stray id: poison the row, never fault
    const float* src = fz ? fused + (seq * r + j) * (long long)d : wte + (bad ? 0 : id) * (long long)d;
    const int n4 = d >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    const float4* p4 = reinterpret_cast<const float4*>(wpe + (long long)t * d);
    float4* xr = reinterpret_cast<float4*>(x_out + row * d);
    float4 v[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int c = lane + 64 * i;
        if (c < n4) {
            const float4 e = s4[c], q = p4[c];
            const float nan = __builtin_nanf("");
            v[i] = bad ? make_float4(nan, nan, nan, nan) : make_float4(e.x + q.x, e.y + q.y, e.z + q.z, e.w + q.w);
            xr[c] = v[i];
        }
    }
    float s_ = 0.f;
#pragma unroll
    for (int i = 0; i < NQ; ++i) s_ += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    const float mean = rag_wave_sum(s_) / (float)d;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NQ; ++i)
        if (lane + 64 * i < n4) {
            const float a0 = v[i].x - mean, a1 = v[i].y - mean, a2 = v[i].z - mean, a3 = v[i].w - mean;
            q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
        }
    const float rstd = rsqrtf(rag_wave_sum(q) / (float)d + eps);
    float4* yr = reinterpret_cast<float4*>(y_out + row * d);
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int c = lane + 64 * i;
        if (c < n4) {
            const float4 ww = reinterpret_cast<const float4*>(w)[c], bb = reinterpret_cast<const float4*>(b)[c];
            yr[c] = make_float4((v[i].x - mean) * rstd * ww.x + bb.x, (v[i].y - mean) * rstd * ww.y + bb.y,
                                (v[i].z - mean) * rstd * ww.z + bb.z, (v[i].w - mean) * rstd * ww.w + bb.w);
        }
    }
}

int launch_splice_embed_ln(const int64_t* aug_ids, const float* fused, int r, const float* wte, const float* wpe, int vocab, int B,
                           int T, int d, const float* w, const float* b, float eps, float* x_out, float* y_out, hipStream_t s) {
    R4D_REQUIRE(aug_ids && fused && r >= 1 && r + 2 <= T && d % 64 == 0 && d <= 2048, "splice embed: r=%d T=%d d=%d", r, T, d);
    const uintptr_t align = (uintptr_t)fused | (uintptr_t)wte | (uintptr_t)wpe | (uintptr_t)w | (uintptr_t)b | (uintptr_t)x_out |
                            (uintptr_t)y_out;
    R4D_REQUIRE((align & 15) == 0, "splice embed: every pointer must be 16-byte aligned");
    const long long rows = (long long)B * T;
    ProfScope prof(PK_SPLICE_EMBED, 12.0 * rows * d + 8.0 * rows, s);
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (d <= 256) hipLaunchKernelGGL(splice_embed_ln4_kernel<1>, grid, dim3(256), 0, s, aug_ids, fused, r, wte, wpe, vocab, rows, T, d, w, b, eps, x_out, y_out);
    else if (d <= 512) hipLaunchKernelGGL(splice_embed_ln4_kernel<2>, grid, dim3(256), 0, s, aug_ids, fused, r, wte, wpe, vocab, rows, T, d, w, b, eps, x_out, y_out);
    else if (d <= 1024) hipLaunchKernelGGL(splice_embed_ln4_kernel<4>, grid, dim3(256), 0, s, aug_ids, fused, r, wte, wpe, vocab, rows, T, d, w, b, eps, x_out, y_out);
    else hipLaunchKernelGGL(splice_embed_ln4_kernel<8>, grid, dim3(256), 0, s, aug_ids, fused, r, wte, wpe, vocab, rows, T, d, w, b, eps, x_out, y_out);
    R4D_CHECK_LAUNCH("splice_embed_ln");
    return R4D_OK;
}

// workgroup (bag q, 256 columns): wave v sums the span's entries v, v + 4, ... in order, then (w0 + w1) + (w2 + w3)
__global__ __launch_bounds__(256) void weighted_bag_kernel(const float* __restrict__ table, int vocab, int d, const int64_t* __restrict__ ids,
                                                           const float* __restrict__ wts, const int32_t* __restrict__ offs,
                                                           float* __restrict__ out) {
    __shared__ float4 part[4][64];
    const int q = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane, n4 = d >> 2;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < n4) {
        const int j1 = offs[q + 1];
        for (int j = offs[q] + wv; j < j1; j += 4) {
            const long long id = ids[j];
            const float cw = wts[j];
            if (id < 0 || id >= vocab) {                             // a stray node id: poison the bag, never fault
                const float nan = __builtin_nanf("");
                acc = make_float4(nan, nan, nan, nan);
                continue;
            }
            const float4 x = reinterpret_cast<const float4*>(table + id * (long long)d)[c];
            acc.x = fmaf(cw, x.x, acc.x); acc.y = fmaf(cw, x.y, acc.y); acc.z = fmaf(cw, x.z, acc.z); acc.w = fmaf(cw, x.w, acc.w);
        }
    }
    part[wv][lane] = acc;
    __syncthreads();
    if (wv == 0 && c < n4) {
        const float4 a = part[0][lane], b = part[1][lane], e = part[2][lane], f = part[3][lane];
        reinterpret_cast<float4*>(out + (long long)q * d)[c] =
            make_float4((a.x + b.x) + (e.x + f.x), (a.y + b.y) + (e.y + f.y), (a.z + b.z) + (e.z + f.z), (a.w + b.w) + (e.w + f.w));
    }
}

__device__ __forceinline__ float scatter_term(const float* src, const int32_t* row_of, const float* wts, long long k, int d, int c) {
    const long long r = row_of ? (long long)row_of[k] : k;
    const float v = src[r * d + c];
    return wts ? wts[k] * v : v;
}
// max |term| over every contribution (the bit pattern of a non-negative float, NaN counted as Inf) into *max_bits (zeroed by the caller)
__global__ __launch_bounds__(256) void scatter_absmax_kernel(const float* __restrict__ src, const int32_t* __restrict__ row_of,
                                                             const float* __restrict__ wts, long long n, int d, unsigned* __restrict__ max_bits) {
    unsigned m = 0u;
    const long long tot = n * d;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < tot; i += (long long)gridDim.x * 256) {
        const float v = fabsf(scatter_term(src, row_of, wts, i / d, d, (int)(i % d)));
        const unsigned bits = (v <= 3.402823466e38f) ? __float_as_uint(v) : 0x7f800000u;
        m = bits > m ? bits : m;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned other = (unsigned)__shfl_xor((int)m, o, 64);
        m = other > m ? other : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(max_bits, m);
}
// one wave per contribution; acc: [vocab * d] sums, the poison word, the max word (train_ops.hip: embedding_bwd_kernel's layout)
__global__ __launch_bounds__(256) void scatter_fix_kernel(const float* __restrict__ src, const int32_t* __restrict__ row_of,
                                                          const float* __restrict__ wts, const int64_t* __restrict__ ids, long long n, int d,
                                                          int vocab, unsigned long long* __restrict__ acc, int lg_rows) {
    const long long k = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n) return;
    const int lane = threadIdx.x & 63;
    const long long tab = (long long)vocab * d;
    const unsigned mb = (unsigned)acc[tab + 1];
    if (mb >= 0x7f800000u) {                                     // a NaN / Inf contribution: the whole output becomes NaN
        if (k == 0 && lane == 0) atomicOr(acc + tab, 1ull);
        return;
    }
    const long long id = ids[k];
    if (id < 0 || id >= vocab) return;
    const int S = emb_scale_exp(mb, lg_rows);
    for (int c = lane; c < d; c += 64) {
        const long long q = __double2ll_rn(ldexp((double)scatter_term(src, row_of, wts, k, d, c), S));
        atomicAdd(acc + id * d + c, (unsigned long long)q);
    }
}

}  // namespace r4d

using namespace r4d;

extern "C" {

size_t r4d_rag_train_workspace_bytes(const r4d_gpt2_config* cfg, int32_t B, int32_t Ta, int32_t ldV) {
    if (!cfg || B <= 0 || Ta <= 0 || ldV <= 0 || cfg->n_embd <= 0) return 0;
    const TrainModes md = train_modes();
    if (!train_modes_ok(md)) return 0;                            // train-attention-fused without train-attention-bf16
    return lm_layout(cfg, B, Ta, ldV, md).total * sizeof(float) + 256;
}

int r4d_rag_train_step_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_gpt2_grads* grads, const r4d_lm_head* head,
                           int32_t head_mode, float* head_grad_d, const int64_t* aug_ids_d, const float* fused_d, int32_t B, int32_t Ta,
                           int32_t r, float grad_scale, float* loss_d, float* d_fused_d, float* hidden_out_d,
                           const r4d_train_dropout* dropout, void* workspace_d, size_t workspace_bytes, void* stream) {
    R4D_REQUIRE(cfg && w && head && head->wte_pad && aug_ids_d && fused_d && loss_d, "rag train step: null pointer");
    R4D_REQUIRE(head_mode == R4D_HEAD_GRAD_UNTIED || head_mode == R4D_HEAD_GRAD_TIED || head_mode == R4D_HEAD_GRAD_NONE,
                "rag train step: head_mode %d", head_mode);
    const bool backward = grads || d_fused_d;                      // every gradient output NULL: forward and loss only
    R4D_REQUIRE(!backward || head_mode != R4D_HEAD_GRAD_UNTIED || head_grad_d, "rag train step: the untied head needs head_grad_d");
    R4D_REQUIRE(!backward || head_mode != R4D_HEAD_GRAD_TIED || (grads && grads->wte), "rag train step: the tied head adds into grads->wte");
    R4D_REQUIRE(!grads || (grads->wte && grads->wpe && grads->ln_f_w && grads->ln_f_b && grads->layers), "rag train step: null gradient");
    R4D_REQUIRE(B >= 1 && r >= 1 && Ta >= r + 3 && head->ldV % 128 == 0 && head->ldV >= cfg->vocab,
                "rag train step: B=%d Ta=%d r=%d ldV=%d (V=%d)", B, Ta, r, head->ldV, cfg->vocab);
    const SpliceIn sp{fused_d, r};
    return head_train_step("rag train step", cfg, w, grads, head, head_mode, head_grad_d, aug_ids_d, &sp, B, Ta, grad_scale, loss_d,
                           d_fused_d, hidden_out_d, dropout, workspace_d, workspace_bytes, train_modes(), (hipStream_t)stream);
}

int r4d_weighted_bag_f32(const float* table_d, int32_t vocab, int32_t d, const int64_t* ids_d, const float* weights_d,
                         const int32_t* offsets_d, int32_t n_bags, float* out_d, void* stream) {
    R4D_REQUIRE(table_d && ids_d && weights_d && offsets_d && out_d && vocab >= 1 && n_bags >= 1 && d % 4 == 0 &&
                d >= 4, "weighted_bag: bad arguments");
    R4D_REQUIRE((((uintptr_t)table_d | (uintptr_t)out_d) & 15) == 0, "weighted_bag: table and out must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(PK_WEIGHTED_BAG, 4.0 * n_bags * d, s);        // output bytes (the gathered rows depend on the spans)
    hipLaunchKernelGGL(weighted_bag_kernel, dim3((unsigned)n_bags, (unsigned)cdiv(d / 4, 64)), dim3(256), 0, s, table_d, vocab, d, ids_d,
                       weights_d, offsets_d, out_d);
    R4D_CHECK_LAUNCH("weighted_bag");
    return R4D_OK;
}

size_t r4d_embedding_scatter_workspace_bytes(int32_t vocab, int32_t d) {
    if (vocab <= 0 || d <= 0) return 0;
    return ((size_t)vocab * d + 2) * sizeof(unsigned long long);
}

int r4d_embedding_scatter_f32(const float* src_d, const int32_t* row_of_d, const float* weights_d, const int64_t* ids_d, int32_t n,
                              int32_t d, int32_t vocab, float* out_d, void* workspace_d, size_t workspace_bytes, void* stream) {
    R4D_REQUIRE(src_d && ids_d && out_d && n >= 1 && d >= 1 && vocab >= 1, "embedding_scatter: bad arguments");
    if (!workspace_d || workspace_bytes < r4d_embedding_scatter_workspace_bytes(vocab, d)) {
        set_error("embedding_scatter: workspace too small");
        return R4D_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* acc = (unsigned long long*)workspace_d;
    const long long tab = (long long)vocab * d;
    R4D_HIP(hipMemsetAsync(acc, 0, ((size_t)tab + 2) * sizeof(unsigned long long), s));
    ProfScope prof(PK_EMB_SCATTER, 4.0 * n * d + 16.0 * tab, s);  // bytes: the terms, the table cleared / summed / converted
    const long long tot = (long long)n * d;
    const unsigned grid = (unsigned)((tot + 256 * 16 - 1) / (256 * 16) < 2048 ? (tot + 256 * 16 - 1) / (256 * 16) : 2048);
    hipLaunchKernelGGL(scatter_absmax_kernel, dim3(grid), dim3(256), 0, s, src_d, row_of_d, weights_d, (long long)n, d,
                       reinterpret_cast<unsigned*>(acc + tab + 1));
    R4D_CHECK_LAUNCH("scatter_absmax");
    hipLaunchKernelGGL(scatter_fix_kernel, dim3((unsigned)(((long long)n + 3) / 4)), dim3(256), 0, s, src_d, row_of_d, weights_d, ids_d,
                       (long long)n, d, vocab, acc, emb_lg_rows(n));
    R4D_CHECK_LAUNCH("scatter_fix");
    return launch_embedding_fix_to_f32(acc, tab, n, out_d, s);
}

}  // extern "C"
