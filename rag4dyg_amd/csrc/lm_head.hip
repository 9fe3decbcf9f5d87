// SimpleDyG LM TRAINING head on gfx950: the logits of every position against the tied token table, the shifted cross entropy of
// models/modeling_gpt2.py:604-615 (labels == inputs) and its gradient -- what torch autograd does for the reference when
// main_SimpleDyG.py:236 calls loss.backward() on GPT2LMHeadModel's loss.
//
//   logits   [N, ldV] = h_lnf . wte_pad^T          the forward GEMM family of the mode (f16x2 / bf16x3 / exact f32), conv1d
//   loss, dlogits (in place)                       lm_ce_kernel: one workgroup per row, the row read once into LDS, written once
//   dh       [N, d]   = dlogits . wte_pad          bf16x3 like every data gradient (train.hip: bwd_data)
//   dwte_head [ldV, d] = dlogits^T . h_lnf         the weight-gradient GEMM (launch_gemm_f32_tn: gemm_s3tn in the split modes)
//   grads->wte = embedding scatter (fixed point, train_ops.hip) + dwte_head[0:V]    in that order
//
// V is padded to ldV (a multiple of 128) with ZERO rows of wte_pad: every GEMM family then sees its aligned shape (K % 32 for the
// planes of dh, I % 128 for gemm_s3tn) and the pad columns of the logits are exact zeros that the CE kernel also writes as
// zero gradient, so the pad contributes nothing anywhere.  Every sum runs in a fixed order (wave butterflies, then sequential
// over waves / threads; no float atomics): the same bits on every launch and rank, like losses.hip.
#include <math.h>
#include <string.h>
#include "common.h"

namespace r4d {

constexpr int CE_THREADS = 512;
constexpr int CE_MAX_LDV = 15872;          // the row lives in LDS: 62 KB (+ the reduction words) of the 64 KB a workgroup gets

__device__ __forceinline__ float ce_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float ce_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// label of row r = (b, t): src[b, t + 1] = src[r + 1] (same sequence while t < T - 1); -1 when the row counts not
__device__ __forceinline__ int ce_label(const int64_t* __restrict__ src, int r, int T, int V) {
    if (r % T == T - 1) return -1;
    const long long l = src[(long long)r + 1];
    return (l >= 0 && l < V) ? (int)l : -1;
}

// one workgroup: the number of counted rows (integers, so the order does not matter); a label outside [0, V) that is not the
// ignore_index -100 raises R4D_RANGE_BAD_LABEL in the range-guard word when one is registered (torch would raise on it)
__global__ __launch_bounds__(1024) void lm_ce_count_kernel(const int64_t* __restrict__ src, int N, int T, int V, int* __restrict__ count,
                                                           unsigned* __restrict__ range_flag) {
    __shared__ int part[16];
    const int tid = threadIdx.x;
    int c = 0;
    bool bad = false;
    for (int r = tid; r < N; r += 1024) {
        c += ce_label(src, r, T, V) >= 0;
        if (r % T != T - 1) {
            const long long l = src[(long long)r + 1];
            bad |= l != -100 && (l < 0 || l >= V);
        }
    }
    if (bad && range_flag) atomicOr(range_flag, R4D_RANGE_BAD_LABEL);
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((tid & 63) == 0) part[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int w = 0; w < 16; ++w) s += part[w];
        *count = s;
    }
}

// one workgroup per row: the row is read ONCE (16-byte loads into LDS), max and sum of exponentials in fp32, the gradient
// written ONCE over the logits; terms[r] = log-sum-exp - logit[label] (0 for an uncounted row)
__global__ __launch_bounds__(CE_THREADS) void lm_ce_kernel(float* __restrict__ logits, int V, int ldV, const int64_t* __restrict__ src,
                                                           int T, float gscale, const int* __restrict__ count, float* __restrict__ terms) {
    extern __shared__ float4 row4[];
    __shared__ float red[CE_THREADS / 64];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float4* g4 = reinterpret_cast<float4*>(logits + (size_t)r * ldV);
    const int n4 = ldV >> 2;
    const int lab = ce_label(src, r, T, V);
    if (lab < 0) {                                                  // no label: exact zero gradient, nothing read
        for (int i = tid; i < n4; i += CE_THREADS) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid == 0) terms[r] = 0.f;
        return;
    }
    float mx = -INFINITY;
    for (int i = tid; i < n4; i += CE_THREADS) {
        const float4 v = g4[i];
        row4[i] = v;
        const int c = 4 * i;
        if (c < V) mx = fmaxf(mx, v.x);
        if (c + 1 < V) mx = fmaxf(mx, v.y);
        if (c + 2 < V) mx = fmaxf(mx, v.z);
        if (c + 3 < V) mx = fmaxf(mx, v.w);
    }
    mx = ce_wave_max(mx);
    if (lane == 0) red[wv] = mx;
    __syncthreads();
    mx = red[0];
    for (int w = 1; w < CE_THREADS / 64; ++w) mx = fmaxf(mx, red[w]);
    __syncthreads();                                                // red is reused below
    float se = 0.f;
    for (int i = tid; i < n4; i += CE_THREADS) {
        const float4 v = row4[i];
        const int c = 4 * i;
        if (c < V) se += expf(v.x - mx);
        if (c + 1 < V) se += expf(v.y - mx);
        if (c + 2 < V) se += expf(v.z - mx);
        if (c + 3 < V) se += expf(v.w - mx);
    }
    se = ce_wave_sum(se);
    if (lane == 0) red[wv] = se;
    __syncthreads();
    se = red[0];
    for (int w = 1; w < CE_THREADS / 64; ++w) se += red[w];
    // softmax as exp(x - max) / sum and the term as log(sum) - (x_label - max): every quantity stays O(1) (losses.hip)
    const float scale = gscale / (float)(*count);
    const float inv_se = 1.f / se;
    for (int i = tid; i < n4; i += CE_THREADS) {
        const float4 v = row4[i];
        const int c = 4 * i;
        float4 o;
        o.x = c < V ? (expf(v.x - mx) * inv_se - (c == lab ? 1.f : 0.f)) * scale : 0.f;
        o.y = c + 1 < V ? (expf(v.y - mx) * inv_se - (c + 1 == lab ? 1.f : 0.f)) * scale : 0.f;
        o.z = c + 2 < V ? (expf(v.z - mx) * inv_se - (c + 2 == lab ? 1.f : 0.f)) * scale : 0.f;
        o.w = c + 3 < V ? (expf(v.w - mx) * inv_se - (c + 3 == lab ? 1.f : 0.f)) * scale : 0.f;
        g4[i] = o;
    }
    if (tid == 0) terms[r] = logf(se) - (reinterpret_cast<const float*>(row4)[lab] - mx);
}

// second stage: thread t sums rows t, t + 1024, ... in order, then a fixed tree over the threads; loss = sum / count
__global__ __launch_bounds__(1024) void lm_ce_reduce_kernel(const float* __restrict__ terms, int N, const int* __restrict__ count,
                                                            float* __restrict__ loss) {
    __shared__ float buf[1024];
    const int tid = threadIdx.x;
    float s = 0.f;
    for (int r = tid; r < N; r += 1024) s += terms[r];
    buf[tid] = s;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) buf[tid] += buf[tid + o];
        __syncthreads();
    }
    if (tid == 0) loss[0] = buf[0] / (float)(*count);             // 0 / 0 = NaN when nothing counts, as torch
}

// y[i] += x[i], i < n (n % 4 == 0, 16-byte aligned)
__global__ __launch_bounds__(256) void add_inplace_kernel(float4* __restrict__ y, const float4* __restrict__ x, long long n4) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) {
        float4 a = y[i];
        const float4 b = x[i];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        y[i] = a;
    }
}

static inline size_t up64(size_t n) { return (n + 63) / 64 * 64; }
static size_t ce_ws_floats(int N) { return up64((size_t)N) + 64; }

static int lm_ce(float* logits, int N, int V, int ldV, const int64_t* src, int T, float gscale, float* loss, float* ws, hipStream_t s) {
    int* count = reinterpret_cast<int*>(ws + up64((size_t)N));
    hipLaunchKernelGGL(lm_ce_count_kernel, dim3(1), dim3(1024), 0, s, src, N, T, V, count, g_range_flag);
    R4D_CHECK_LAUNCH("lm_ce_count");
    {
        ProfScope prof(PK_LM_CE, 2.0 * N * (double)V * 4.0, s);
        hipLaunchKernelGGL(lm_ce_kernel, dim3(N), dim3(CE_THREADS), (size_t)ldV * sizeof(float), s, logits, V, ldV, src, T, gscale,
                           count, ws);
        R4D_CHECK_LAUNCH("lm_ce");
    }
    hipLaunchKernelGGL(lm_ce_reduce_kernel, dim3(1), dim3(1024), 0, s, ws, N, count, loss);
    R4D_CHECK_LAUNCH("lm_ce_reduce");
    return R4D_OK;
}

int check_ce(int N, int V, int ldV, int T) {
    R4D_REQUIRE(N >= 1 && T >= 1 && N % T == 0, "lm_ce: N=%d is not a multiple of T=%d", N, T);
    R4D_REQUIRE(V >= 1 && ldV >= V && ldV % 4 == 0 && ldV <= CE_MAX_LDV, "lm_ce: V=%d ldV=%d (V <= ldV <= %d, ldV %% 4 == 0)", V, ldV,
                CE_MAX_LDV);
    return R4D_OK;
}

LMLayout lm_layout(const r4d_gpt2_config* cfg, int B, int T, int ldV) {
    LMLayout t;
    const size_t N = (size_t)B * T, d = cfg->n_embd;
    size_t off = 0;
    auto take = [&](size_t n) { const size_t o = off; off += up64(n); return o; };
    t.train = take(gpt2_train_workspace_floats(cfg, 1, &B, &T));
    t.h = take(N * d); t.logits = take(N * ldV); t.dh = take(N * d); t.dwte = take((size_t)ldV * d);
    t.tn = take(gemm_tn_scratch_floats(ldV, (int)d, (int)N)); t.ce = take(ce_ws_floats((int)N));
    t.total = off;
    return t;
}

int launch_add_inplace(float* y, const float* x, long long n, hipStream_t s) {
    const long long n4 = n / 4;
    hipLaunchKernelGGL(add_inplace_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<float4*>(y),
                       reinterpret_cast<const float4*>(x), n4);
    R4D_CHECK_LAUNCH("lm_wte_add");
    return R4D_OK;
}

// The head of both training steps (the LM step below, the RAG step of rag_train.hip): logits on the mode's forward GEMM family,
// the cross entropy, then dh = dlogits . wte_pad (bf16x3 like every data gradient) and dwte = dlogits^T . h
int lm_head_train(const float* h, int N, int V, int d, const r4d_lm_head* head, const int64_t* src, int T, float gscale, float* loss,
                  float* logits, float* dh, float* dwte, float* tn_scratch, float* ce_ws, hipStream_t s) {
    const int ldV = head->ldV;
    int rc;
    // logits = h . wte_pad^T: wte_pad [ldV, d] IS the k-contiguous [N, K] operand (planes when the mode has them)
    if ((rc = conv1d(h, nullptr, head->wte_pad, nullptr, nullptr, N, d, ldV, EPI_NONE, logits, s, nullptr, false, head->w3, head->h2)))
        return rc;
    if ((rc = lm_ce(logits, N, V, ldV, src, T, gscale, loss, ce_ws, s))) return rc;
    // dh = dlogits . wte_pad  (K = ldV: the pad columns of dlogits are zero)
    if (dh && head->w3t && g_gemm_split3 && gemm_s3_supported(N, ldV, d)) {
        S3Args a;
        memset(&a, 0, sizeof(a));
        a.A = logits; a.planes = head->w3t; a.C = dh; a.M = N; a.N = d; a.K = ldV; a.lda = ldV; a.ldc = d; a.ldr = d;
        a.epilogue = EPI_NONE;
        if ((rc = launch_gemm_s3(a, s))) return rc;
    } else if (dh) {
        GemmArgs g;
        memset(&g, 0, sizeof(g));
        g.A = logits; g.B = head->wte_pad; g.C = dh;
        g.M = N; g.N = d; g.K = ldV; g.lda = ldV; g.ldb = d; g.ldc = d;
        g.b_trans = 0; g.b_rows = ldV; g.nbatch = 1; g.nb1 = 1; g.epilogue = EPI_NONE; g.scale_div = 1.f; g.causal = CAUSAL_NONE;
        if ((rc = launch_gemm_f32(g, s))) return rc;
    }
    // dwte [ldV, d] = dlogits^T . h
    return dwte ? launch_gemm_f32_tn(logits, h, dwte, ldV, d, N, ldV, d, tn_scratch, s) : R4D_OK;
}

}  // namespace r4d

using namespace r4d;

extern "C" {

int r4d_gpt2_train_forward_hidden_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, int32_t n_groups,
                                      const int64_t* const* ids_d, const int32_t* Bs, const int32_t* Ts, float* out_hidden_d,
                                      const r4d_train_dropout* dropout, void* workspace_d, size_t workspace_bytes, void* stream) {
    R4D_REQUIRE(out_hidden_d, "gpt2 train: null pointer");
    return gpt2_train_forward(cfg, w, n_groups, ids_d, Bs, Ts, nullptr, out_hidden_d, dropout, workspace_d, workspace_bytes,
                              (hipStream_t)stream);
}

int r4d_gpt2_train_backward_hidden_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_gpt2_grads* grads,
                                       int32_t n_groups, const int64_t* const* ids_d, const int32_t* Bs, const int32_t* Ts,
                                       const float* d_hidden_d, const r4d_train_dropout* dropout,
                                       void* workspace_d, size_t workspace_bytes, void* stream) {
    R4D_REQUIRE(d_hidden_d, "gpt2 train backward: null pointer");
    return gpt2_train_backward(cfg, w, grads, n_groups, ids_d, Bs, Ts, nullptr, d_hidden_d, dropout, workspace_d, workspace_bytes,
                               (hipStream_t)stream);
}

size_t r4d_lm_ce_workspace_bytes(int32_t N) { return N > 0 ? ce_ws_floats(N) * sizeof(float) : 0; }

int r4d_lm_ce_f32(float* logits_d, int32_t N, int32_t V, int32_t ldV, const int64_t* ids_d, const int64_t* labels_d, int32_t T,
                  float grad_scale, float* loss_d, void* workspace_d, size_t workspace_bytes, void* stream) {
    int rc = check_ce(N, V, ldV, T);
    if (rc) return rc;
    const int64_t* src = labels_d ? labels_d : ids_d;
    R4D_REQUIRE(logits_d && src && loss_d && ((uintptr_t)logits_d % 16) == 0, "lm_ce: null or misaligned pointer");
    if (!workspace_d || workspace_bytes < r4d_lm_ce_workspace_bytes(N)) {
        set_error("lm_ce: workspace too small");
        return R4D_ERR_WORKSPACE;
    }
    return lm_ce(logits_d, N, V, ldV, src, T, grad_scale, loss_d, (float*)workspace_d, (hipStream_t)stream);
}

size_t r4d_gpt2_lm_train_workspace_bytes(const r4d_gpt2_config* cfg, int32_t B, int32_t T, int32_t ldV) {
    if (!cfg || B <= 0 || T <= 0 || ldV <= 0 || cfg->n_embd <= 0) return 0;
    return lm_layout(cfg, B, T, ldV).total * sizeof(float) + 256;
}

int r4d_gpt2_lm_train_step_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_gpt2_grads* grads,
                               const r4d_lm_head* head, const int64_t* ids_d, int32_t B, int32_t T, float grad_scale, float* loss_d,
                               const r4d_train_dropout* dropout, void* workspace_d, size_t workspace_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    R4D_REQUIRE(cfg && w && grads && grads->wte && head && head->wte_pad && ids_d && loss_d, "lm train step: null pointer");
    const int V = cfg->vocab, ldV = head->ldV, d = cfg->n_embd;
    R4D_REQUIRE(B >= 1 && T >= 1 && ldV % 128 == 0 && ldV >= V, "lm train step: B=%d T=%d ldV=%d (a multiple of 128 >= V=%d)", B, T,
                ldV, V);
    int rc = check_ce(B * T, V, ldV, T);
    if (rc) return rc;
    const LMLayout t = lm_layout(cfg, B, T, ldV);
    if (!workspace_d || workspace_bytes < t.total * sizeof(float)) {
        set_error("lm train step: workspace %zu bytes < required %zu", workspace_bytes, t.total * sizeof(float));
        return R4D_ERR_WORKSPACE;
    }
    float* ws = (float*)workspace_d;
    const int N = B * T;
    float *h = ws + t.h, *logits = ws + t.logits, *dh = ws + t.dh, *dwte = ws + t.dwte;
    const size_t train_bytes = (t.h - t.train) * sizeof(float);
    const int64_t* const ids[1] = {ids_d};
    if ((rc = gpt2_train_forward(cfg, w, 1, ids, &B, &T, nullptr, h, dropout, ws + t.train, train_bytes, s))) return rc;
    if ((rc = lm_head_train(h, N, V, d, head, ids_d, T, grad_scale, loss_d, logits, dh, dwte, ws + t.tn, ws + t.ce, s))) return rc;
    if ((rc = gpt2_train_backward(cfg, w, grads, 1, ids, &B, &T, nullptr, dh, dropout, ws + t.train, train_bytes, s))) return rc;
    // tied weight: the embedding scatter (written by the backward) + the head's part, in this fixed order
    return launch_add_inplace(grads->wte, dwte, (long long)V * d, s);
}

}  // extern "C"
