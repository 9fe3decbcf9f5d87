// SimpleDyG LM TRAINING head on gfx950: the logits of every position against the tied token table, the shifted cross entropy of
// models/modeling_gpt2.py:604-615 (labels == inputs) and its gradient -- what torch autograd does for the reference when
// main_SimpleDyG.py:236 calls loss.backward() on GPT2LMHeadModel's loss.
//
//   logits   [N, ldV] = h_lnf . wte_pad^T          the forward GEMM family of the mode (f16x2 / bf16x3 / exact f32), conv1d
//   loss, dlogits (in place)                       lm_ce_kernel: one workgroup per row, the row read once into LDS, written once
//   dh       [N, d]   = dlogits . wte_pad          bf16x3 like every data gradient (train.hip: data_grad)
//   dwte_head [ldV, d] = dlogits^T . h_lnf         the weight-gradient GEMM (train.hip: weight_grad -- gemm_s3tn in the split modes)
//   grads->wte = embedding scatter (fixed point, train_ops.hip) + dwte_head[0:V]    in that order
//
// V is padded to ldV (a multiple of 128) with ZERO rows of wte_pad: every GEMM family then sees its aligned shape (K % 32 for the
// planes of dh, I % 128 for gemm_s3tn) and the pad columns of the logits are exact zeros that the CE kernel also writes as
// zero gradient, so the pad contributes nothing anywhere.  Every sum runs in a fixed order (wave butterflies, then sequential
// over waves / threads; no float atomics): the same bits on every launch and rank, like losses.hip.
//
// ldV > CE_MAX_LDV (a vocabulary beyond what one LDS row holds): the CHUNKED head (lm_head_train_chunked below).  The rows of
// wte_pad are cut into chunks of CE_CHUNK; the logits exist one chunk [N, Ck] at a time, a first sweep folds every chunk into the
// row's running (max, sum of exponentials, label logit) -- an online softmax -- and a second sweep forms each chunk's logits again
// (the same launch on the same bits), turns them into their gradient and feeds the two gradient GEMMs.  Scratch does not grow
// with V; one extra logits GEMM is the price.
//
// r4d_set_train_head_bf16 (`hb` below, read by the step entries and handed down; NOT fp32-accurate): per chunk
//   logits_k = RN(h) . RN(wte_k)^T        gemm_b1 on plane 0 of the chunk's w3 (conv1d, BF16_TRAIN_HEAD)
//   dh (+)= RN(dlogits_k) . RN(wte_k)     gemm_b1 on plane 0 of the chunk's w3t, K = Ck, the residual epilogue onto dh itself for k > 0
//   dwte[c0 : c0 + Ck] = RN(dlogits_k)^T . RN(h)    gemm_b1tn (I = Ck, J = d, lda = Ck), slices within the room of `tn`
// each product on its own: one whose plane is missing or whose shape the bf16 kernel refuses keeps the route above.  The logits and
// their gradient in memory, the cross entropy, dh, dwte and the tied add stay fp32.  dh in place: the residual epilogue
// (gemm_epilogue_rowmajor.h) loads an accumulator tile's 16 second-buffer values in the thread that then stores those 16 elements
// of C, loads first (interior tiles: the res[] loop ahead of the stores; edge tiles: res[r] ahead of the guarded store; a clamped
// row or column reads an element some other thread writes, and throws it away) -- the bf16x3 route relies on the same text.
#include <math.h>
#include <string.h>
#include "common.h"

namespace r4d {

constexpr int CE_THREADS = 512;
constexpr int CE_MAX_LDV = 15872;          // the row lives in LDS: 62 KB (+ the reduction words) of the 64 KB a workgroup gets
constexpr int CE_CHUNK = 15872;            // vocabulary rows per chunk of the chunked head (a multiple of 128, <= CE_MAX_LDV); 8192 measured 2 % slower: DESIGN.md 7.1
static_assert(CE_CHUNK % 128 == 0 && CE_CHUNK <= CE_MAX_LDV, "a chunk row is staged in LDS like a whole row");
static inline int ce_chunk_rows(int ldV) { return ldV <= CE_MAX_LDV ? ldV : CE_CHUNK; }

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

// ---- the chunked form (ldV > CE_MAX_LDV): the same row, one column range [c0, c0 + cn) at a time
// One workgroup per row.  The range is read ONCE into LDS; its max mc and sum of exponentials sc are folded into the row's running
// pair as m' = max(m, mc), s = s exp(m - m') + sc exp(mc - m') (the range at c0 == 0 starts the pair); the label's logit is kept
// when the label lies in the range.  `last`: terms[r] = log s - (x_label - m) (0 for an uncounted row).  Columns >= V are never
// read as classes; a row without a counted label reads nothing.  x: column c0 of row 0 (the range's first element), ld: row stride.
__global__ __launch_bounds__(CE_THREADS) void lm_ce_stats_kernel(const float* __restrict__ x, size_t ld, int c0, int cn, int V,
                                                                 const int64_t* __restrict__ src, int T, float* __restrict__ m_run,
                                                                 float* __restrict__ s_run, float* __restrict__ x_lab, int last,
                                                                 float* __restrict__ terms) {
    extern __shared__ float4 row4[];
    __shared__ float red[CE_THREADS / 64];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int lab = ce_label(src, r, T, V);
    if (lab < 0) {
        if (last && tid == 0) terms[r] = 0.f;
        return;
    }
    const float4* g4 = reinterpret_cast<const float4*>(x + (size_t)r * ld);
    const int n4 = cn >> 2;
    float mx = -INFINITY;
    for (int i = tid; i < n4; i += CE_THREADS) {
        const float4 v = g4[i];
        row4[i] = v;
        const int c = c0 + 4 * i;
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
        const int c = c0 + 4 * i;
        if (c < V) se += expf(v.x - mx);
        if (c + 1 < V) se += expf(v.y - mx);
        if (c + 2 < V) se += expf(v.z - mx);
        if (c + 3 < V) se += expf(v.w - mx);
    }
    se = ce_wave_sum(se);
    if (lane == 0) red[wv] = se;
    __syncthreads();
    if (tid != 0) return;
    se = red[0];
    for (int w = 1; w < CE_THREADS / 64; ++w) se += red[w];
    float m = mx, sum = se;
    if (c0 > 0) {                                                   // fold into the ranges before this one
        const float m0 = m_run[r];
        m = fmaxf(m0, mx);
        sum = s_run[r] * expf(m0 - m) + se * expf(mx - m);
    }
    m_run[r] = m;
    s_run[r] = sum;
    float xl;
    if (lab >= c0 && lab < c0 + cn) xl = reinterpret_cast<const float*>(row4)[lab - c0];
    else xl = c0 > 0 ? x_lab[r] : 0.f;
    x_lab[r] = xl;
    if (last) terms[r] = logf(sum) - (xl - m);
}

// One workgroup per row: the range's logits are OVERWRITTEN with gscale * (exp(x - m) / s - onehot) / n_counted from the row's
// final (m, s); exact zeros in the columns >= V and in rows without a counted label.
__global__ __launch_bounds__(CE_THREADS) void lm_ce_grad_kernel(float* __restrict__ x, size_t ld, int c0, int cn, int V,
                                                                const int64_t* __restrict__ src, int T, float gscale,
                                                                const int* __restrict__ count, const float* __restrict__ m_run,
                                                                const float* __restrict__ s_run) {
    const int r = blockIdx.x, tid = threadIdx.x;
    float4* g4 = reinterpret_cast<float4*>(x + (size_t)r * ld);
    const int n4 = cn >> 2;
    const int lab = ce_label(src, r, T, V);
    if (lab < 0) {
        for (int i = tid; i < n4; i += CE_THREADS) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const float mx = m_run[r], inv_se = 1.f / s_run[r], scale = gscale / (float)(*count);
    for (int i = tid; i < n4; i += CE_THREADS) {
        const float4 v = g4[i];
        const int c = c0 + 4 * i;
        float4 o;
        o.x = c < V ? (expf(v.x - mx) * inv_se - (c == lab ? 1.f : 0.f)) * scale : 0.f;
        o.y = c + 1 < V ? (expf(v.y - mx) * inv_se - (c + 1 == lab ? 1.f : 0.f)) * scale : 0.f;
        o.z = c + 2 < V ? (expf(v.z - mx) * inv_se - (c + 2 == lab ? 1.f : 0.f)) * scale : 0.f;
        o.w = c + 3 < V ? (expf(v.w - mx) * inv_se - (c + 3 == lab ? 1.f : 0.f)) * scale : 0.f;
        g4[i] = o;
    }
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
// terms [N], the count word; the chunked form adds the rows' running (m, s, x_label)
static size_t ce_ws_floats(int N, bool chunked) { return up64((size_t)N) * (chunked ? 4 : 1) + 64; }
struct CeWs { float* terms; int* count; float* m; float* s; float* xl; };
static CeWs ce_ws(float* ws, int N) {
    const size_t n = up64((size_t)N);
    return {ws, reinterpret_cast<int*>(ws + n), ws + n + 64, ws + 2 * n + 64, ws + 3 * n + 64};
}

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

// the pieces of the chunked form, in the order the callers issue them: count; stats per range (ascending, the range that
// holds column V - 1 with last = true); reduce; grad per range
static int launch_ce_count(const int64_t* src, int N, int T, int V, const CeWs& w, hipStream_t s) {
    hipLaunchKernelGGL(lm_ce_count_kernel, dim3(1), dim3(1024), 0, s, src, N, T, V, w.count, g_range_flag);
    R4D_CHECK_LAUNCH("lm_ce_count");
    return R4D_OK;
}
static int launch_ce_stats(const float* x, size_t ld, int c0, int cn, int N, int V, const int64_t* src, int T, const CeWs& w, bool last,
                           hipStream_t s) {
    const int real = (V - c0 < cn ? V - c0 : cn);
    ProfScope prof(PK_LM_CE, (double)N * real * 4.0, s);
    hipLaunchKernelGGL(lm_ce_stats_kernel, dim3(N), dim3(CE_THREADS), (size_t)cn * sizeof(float), s, x, ld, c0, cn, V, src, T, w.m, w.s,
                       w.xl, last ? 1 : 0, w.terms);
    R4D_CHECK_LAUNCH("lm_ce_stats");
    return R4D_OK;
}
static int launch_ce_reduce(int N, const CeWs& w, float* loss, hipStream_t s) {
    hipLaunchKernelGGL(lm_ce_reduce_kernel, dim3(1), dim3(1024), 0, s, w.terms, N, w.count, loss);
    R4D_CHECK_LAUNCH("lm_ce_reduce");
    return R4D_OK;
}
static int launch_ce_grad(float* x, size_t ld, int c0, int cn, int N, int V, const int64_t* src, int T, float gscale, const CeWs& w,
                          hipStream_t s) {
    ProfScope prof(PK_LM_CE, 2.0 * N * (double)cn * 4.0, s);
    hipLaunchKernelGGL(lm_ce_grad_kernel, dim3(N), dim3(CE_THREADS), 0, s, x, ld, c0, cn, V, src, T, gscale, w.count, w.m, w.s);
    R4D_CHECK_LAUNCH("lm_ce_grad");
    return R4D_OK;
}

// r4d_lm_ce_f32 on a materialised [N, ldV] matrix with ldV > CE_MAX_LDV: the two kernels over the column ranges, row stride ldV
static int lm_ce_chunked(float* logits, int N, int V, int ldV, const int64_t* src, int T, float gscale, float* loss, float* ws,
                         hipStream_t s) {
    const CeWs w = ce_ws(ws, N);
    const int C = CE_CHUNK;
    int rc;
    if ((rc = launch_ce_count(src, N, T, V, w, s))) return rc;
    for (int c0 = 0; c0 < V; c0 += C) {                      // ranges past V hold no class
        const int cn = ldV - c0 < C ? ldV - c0 : C;
        if ((rc = launch_ce_stats(logits + c0, (size_t)ldV, c0, cn, N, V, src, T, w, c0 + C >= V, s))) return rc;
    }
    if ((rc = launch_ce_reduce(N, w, loss, s))) return rc;
    for (int c0 = 0; c0 < ldV; c0 += C) {
        const int cn = ldV - c0 < C ? ldV - c0 : C;
        if ((rc = launch_ce_grad(logits + c0, (size_t)ldV, c0, cn, N, V, src, T, gscale, w, s))) return rc;
    }
    return R4D_OK;
}

static int check_ce(int N, int V, int ldV, int T) {
    R4D_REQUIRE(N >= 1 && T >= 1 && N % T == 0, "lm_ce: N=%d is not a multiple of T=%d", N, T);
    R4D_REQUIRE(V >= 1 && ldV >= V && ldV % 4 == 0, "lm_ce: V=%d ldV=%d (V <= ldV, ldV %% 4 == 0)", V, ldV);
    return R4D_OK;
}

// the weight gradient's slices: room for ONE chunk, the full one or the shorter last one
static size_t head_tn_floats(int N, int d, int ldV) {
    const int C = ce_chunk_rows(ldV), tail = ldV % C;
    size_t tn = gemm_tn_scratch_floats(C, d, N);
    if (tail) { const size_t tn2 = gemm_tn_scratch_floats(tail, d, N); tn = tn2 > tn ? tn2 : tn; }
    return tn;
}

LMLayout lm_layout(const r4d_gpt2_config* cfg, int B, int T, int ldV, TrainModes md) {
    LMLayout t;
    const size_t N = (size_t)B * T, d = cfg->n_embd;
    size_t off = 0;
    auto take = [&](size_t n) { const size_t o = off; off += up64(n); return o; };
    t.train = take(gpt2_train_workspace_floats(cfg, 1, &B, &T, md));
    // ldV > CE_MAX_LDV: the logits slot and the weight-gradient scratch hold ONE chunk (the full one or the shorter last one)
    // (the sizes do not depend on r4d_set_train_head_bf16: gemm_b1tn cuts its slices to the room of `tn`)
    const int C = ce_chunk_rows(ldV);
    const size_t tn = head_tn_floats((int)N, (int)d, ldV);
    t.h = take(N * d); t.logits = take(N * C); t.dh = take(N * d); t.dwte = take((size_t)ldV * d);
    t.tn = take(tn); t.ce = take(ce_ws_floats((int)N, ldV > CE_MAX_LDV));
    t.total = off;
    return t;
}

// y += x (n % 4 == 0, 16-byte aligned)
static int launch_add_inplace(float* y, const float* x, long long n, hipStream_t s) {
    const long long n4 = n / 4;
    hipLaunchKernelGGL(add_inplace_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<float4*>(y),
                       reinterpret_cast<const float4*>(x), n4);
    R4D_CHECK_LAUNCH("lm_wte_add");
    return R4D_OK;
}

// The chunked head (ldV > CE_MAX_LDV).  Chunk k covers the rows [k C, k C + Ck) of wte_pad; `logits` holds ONE chunk [N, Ck].
//   sweep 1, k ascending:  logits_k = h . wte_k^T (the forward GEMM family of the mode), lm_ce_stats
//   loss = reduce(terms);  dh == dwte == NULL (the evaluation loss): done
//   sweep 2, k ascending:  the same GEMM again (deterministic kernels: the same bits), lm_ce_grad, dh (+)= dlogits_k . wte_k through
//                          the residual epilogue (k == 0 has none), dwte[k C : k C + Ck] = dlogits_k^T . h
// The planes are laid chunk by chunk (include/r4d.h: r4d_lm_head), so every GEMM is an ordinary aligned one on a contiguous
// operand; the chunk order is fixed, so dh carries the same bits on every launch.
static int lm_head_train_chunked(const float* h, int N, int V, int d, const r4d_lm_head* head, const int64_t* src, int T, float gscale,
                                 float* loss, float* logits, float* dh, float* dwte, float* tn_scratch, float* ce_ws_, int hb,
                                 hipStream_t s) {
    const int ldV = head->ldV, C = CE_CHUNK;
    R4D_REQUIRE((long long)N * C < (1ll << 31) && (long long)ldV * d < (1ll << 31),
                "lm head: N=%d rows x %d chunk columns or ldV=%d x d=%d reaches 2^31 elements (32-bit index arithmetic)", N, C, ldV, d);
    const CeWs w = ce_ws(ce_ws_, N);
    int rc;
    const Conv1DOpts fwd{nullptr, false, hb ? BF16_TRAIN_HEAD : BF16_OFF};
    const int gb = hb ? TRAIN_BF16_HEAD : TRAIN_BF16_OFF;
    auto chunk_logits = [&](int c0, int cn) { return conv1d(conv1d_w(*head, d, c0, cn), h, nullptr, N, EPI_NONE, logits, s, fwd); };
    if ((rc = launch_ce_count(src, N, T, V, w, s))) return rc;
    for (int c0 = 0; c0 < ldV; c0 += C) {
        const int cn = ldV - c0 < C ? ldV - c0 : C;
        if ((rc = chunk_logits(c0, cn))) return rc;
        if ((rc = launch_ce_stats(logits, (size_t)cn, c0, cn, N, V, src, T, w, c0 + C >= ldV, s))) return rc;
    }
    if ((rc = launch_ce_reduce(N, w, loss, s))) return rc;
    if (!dh && !dwte) return R4D_OK;
    for (int c0 = 0; c0 < ldV; c0 += C) {
        const int cn = ldV - c0 < C ? ldV - c0 : C;
        if ((rc = chunk_logits(c0, cn))) return rc;
        if ((rc = launch_ce_grad(logits, (size_t)cn, c0, cn, N, V, src, T, gscale, w, s))) return rc;
        if (dh && (rc = data_grad(conv1d_w(*head, d, c0, cn), logits, N, dh, c0 ? dh : nullptr, nullptr, s, gb))) return rc;
        if (dwte && (rc = weight_grad(logits, h, dwte + (size_t)c0 * d, nullptr, cn, d, N, cn, d, tn_scratch, nullptr, s, gb))) return rc;
    }
    return R4D_OK;
}

// The head of the training step: logits = h . wte_pad^T on the mode's forward GEMM family, loss and dlogits (in place; label of
// row r: src[r + 1] within a sequence of T rows), then -- when `dh` is given -- dh = dlogits . wte_pad (bf16x3 like every data
// gradient) and -- when `dwte` is given -- dwte [ldV, d] = dlogits^T . h.  `hb` (TrainModes::head_bf16): each of the three on plain
// bf16 operands where its plane and shape allow (the head of this file).  A loss-only call (dh == dwte == NULL) forms its logits by
// the launch the training call uses, so its loss carries the training call's bits.
static int lm_head_train(const float* h, int N, int V, int d, const r4d_lm_head* head, const int64_t* src, int T, float gscale,
                         float* loss, float* logits, float* dh, float* dwte, float* tn_scratch, float* ce_ws, int hb, hipStream_t s) {
    const int ldV = head->ldV;
    if (ldV > CE_MAX_LDV) return lm_head_train_chunked(h, N, V, d, head, src, T, gscale, loss, logits, dh, dwte, tn_scratch, ce_ws, hb, s);
    int rc;
    const int gb = hb ? TRAIN_BF16_HEAD : TRAIN_BF16_OFF;
    // logits = h . wte_pad^T: wte_pad [ldV, d] IS the k-contiguous [N, K] operand (planes when the mode has them)
    const Conv1DW W = conv1d_w(*head, d, 0, ldV);
    if ((rc = conv1d(W, h, nullptr, N, EPI_NONE, logits, s, Conv1DOpts{nullptr, false, hb ? BF16_TRAIN_HEAD : BF16_OFF}))) return rc;
    if ((rc = lm_ce(logits, N, V, ldV, src, T, gscale, loss, ce_ws, s))) return rc;
    // dh = dlogits . wte_pad  (K = ldV: the pad columns of dlogits are zero)
    if (dh && (rc = data_grad(W, logits, N, dh, nullptr, nullptr, s, gb))) return rc;
    // dwte [ldV, d] = dlogits^T . h
    return dwte ? weight_grad(logits, h, dwte, nullptr, ldV, d, N, ldV, d, tn_scratch, nullptr, s, gb) : R4D_OK;
}

// The head alone (r4d_lm_head_train_f32): one chunk of logits, the weight gradient's slices, the cross entropy's words
struct HeadLayout { size_t logits, tn, ce, total; };
static HeadLayout head_layout(int N, int d, int ldV) {
    HeadLayout t;
    size_t off = 0;
    auto take = [&](size_t n) { const size_t o = off; off += up64(n); return o; };
    t.logits = take((size_t)N * ce_chunk_rows(ldV)); t.tn = take(head_tn_floats(N, d, ldV));
    t.ce = take(ce_ws_floats(N, ldV > CE_MAX_LDV));
    t.total = off;
    return t;
}

// One training step through the head, behind the argument checks of its two exports (`who`: the export's name in a message):
// training forward (train.hip) -> lm_head_train on `ids` -> backward -> the head's weight gradient to its place.  The LM step is
// the RAG step without a splice (`sp` == nullptr), with a tied head and no optional output.  No gradient output at all (`grads`
// and `d_fused` NULL): forward and loss only.
int head_train_step(const char* who, const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_gpt2_grads* grads,
                    const r4d_lm_head* head, int head_mode, float* head_grad, const int64_t* ids_d, const SpliceIn* sp, int B, int T,
                    float gscale, float* loss, float* d_fused, float* hidden_out, const r4d_train_dropout* dropout, void* workspace_d,
                    size_t workspace_bytes, TrainModes md, hipStream_t s) {
    const int V = cfg->vocab, ldV = head->ldV, d = cfg->n_embd, N = B * T;
    int rc = check_ce(N, V, ldV, T);
    if (rc) return rc;
    const LMLayout t = lm_layout(cfg, B, T, ldV, md);
    if (!workspace_d || workspace_bytes < t.total * sizeof(float)) {
        set_error("%s: workspace %zu bytes < required %zu", who, workspace_bytes, t.total * sizeof(float));
        return R4D_ERR_WORKSPACE;
    }
    float* ws = (float*)workspace_d;
    float *h = ws + t.h, *logits = ws + t.logits, *dh = ws + t.dh, *dwte = ws + t.dwte;
    const size_t train_bytes = (t.h - t.train) * sizeof(float);
    const int64_t* const ids[1] = {ids_d};
    const bool backward = grads || d_fused;
    const bool head_w = backward && head_mode != R4D_HEAD_GRAD_NONE;
    if ((rc = gpt2_train_forward(cfg, w, 1, ids, &B, &T, nullptr, h, dropout, ws + t.train, train_bytes, md, s, sp))) return rc;
    if (hidden_out) R4D_HIP(hipMemcpyAsync(hidden_out, h, (size_t)N * d * sizeof(float), hipMemcpyDeviceToDevice, s));
    if ((rc = lm_head_train(h, N, V, d, head, ids_d, T, gscale, loss, logits, backward ? dh : nullptr, head_w ? dwte : nullptr,
                            ws + t.tn, ws + t.ce, md.head_bf16, s))) return rc;
    if (!backward) return R4D_OK;
    if ((rc = gpt2_train_backward(cfg, w, grads, 1, ids, &B, &T, nullptr, dh, dropout, ws + t.train, train_bytes, md, s, sp, d_fused)))
        return rc;
    if (head_mode == R4D_HEAD_GRAD_UNTIED)
        R4D_HIP(hipMemcpyAsync(head_grad, dwte, (size_t)V * d * sizeof(float), hipMemcpyDeviceToDevice, s));
    else if (head_mode == R4D_HEAD_GRAD_TIED)                       // tied weight: the token scatter (written by the backward) + the
        return launch_add_inplace(grads->wte, dwte, (long long)V * d, s);   // head's part, in this fixed order
    return R4D_OK;
}

}  // namespace r4d

using namespace r4d;

extern "C" {

int r4d_gpt2_train_forward_hidden_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, int32_t n_groups,
                                      const int64_t* const* ids_d, const int32_t* Bs, const int32_t* Ts, float* out_hidden_d,
                                      const r4d_train_dropout* dropout, void* workspace_d, size_t workspace_bytes, void* stream) {
    R4D_REQUIRE(out_hidden_d, "gpt2 train: null pointer");
    return gpt2_train_forward(cfg, w, n_groups, ids_d, Bs, Ts, nullptr, out_hidden_d, dropout, workspace_d, workspace_bytes,
                              train_modes(), (hipStream_t)stream);
}

int r4d_gpt2_train_backward_hidden_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_gpt2_grads* grads,
                                       int32_t n_groups, const int64_t* const* ids_d, const int32_t* Bs, const int32_t* Ts,
                                       const float* d_hidden_d, const r4d_train_dropout* dropout,
                                       void* workspace_d, size_t workspace_bytes, void* stream) {
    R4D_REQUIRE(d_hidden_d, "gpt2 train backward: null pointer");
    return gpt2_train_backward(cfg, w, grads, n_groups, ids_d, Bs, Ts, nullptr, d_hidden_d, dropout, workspace_d, workspace_bytes,
                               train_modes(), (hipStream_t)stream);
}

size_t r4d_lm_ce_workspace_bytes(int32_t N) { return N > 0 ? ce_ws_floats(N, true) * sizeof(float) : 0; }

int32_t r4d_lm_head_chunk_rows(int32_t ldV) { return ldV > 0 ? ce_chunk_rows(ldV) : 0; }

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
    if (ldV > CE_MAX_LDV) return lm_ce_chunked(logits_d, N, V, ldV, src, T, grad_scale, loss_d, (float*)workspace_d, (hipStream_t)stream);
    return lm_ce(logits_d, N, V, ldV, src, T, grad_scale, loss_d, (float*)workspace_d, (hipStream_t)stream);
}

size_t r4d_gpt2_lm_train_workspace_bytes(const r4d_gpt2_config* cfg, int32_t B, int32_t T, int32_t ldV) {
    if (!cfg || B <= 0 || T <= 0 || ldV <= 0 || cfg->n_embd <= 0) return 0;
    const TrainModes md = train_modes();
    if (!train_modes_ok(md)) return 0;                            // train-attention-fused without train-attention-bf16
    return lm_layout(cfg, B, T, ldV, md).total * sizeof(float) + 256;
}

int r4d_gpt2_lm_train_step_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_gpt2_grads* grads,
                               const r4d_lm_head* head, const int64_t* ids_d, int32_t B, int32_t T, float grad_scale, float* loss_d,
                               const r4d_train_dropout* dropout, void* workspace_d, size_t workspace_bytes, void* stream) {
    R4D_REQUIRE(cfg && w && grads && grads->wte && head && head->wte_pad && ids_d && loss_d, "lm train step: null pointer");
    R4D_REQUIRE(B >= 1 && T >= 1 && head->ldV % 128 == 0 && head->ldV >= cfg->vocab,
                "lm train step: B=%d T=%d ldV=%d (a multiple of 128 >= V=%d)", B, T, head->ldV, cfg->vocab);
    return head_train_step("lm train step", cfg, w, grads, head, R4D_HEAD_GRAD_TIED, nullptr, ids_d, nullptr, B, T, grad_scale, loss_d,
                           nullptr, nullptr, dropout, workspace_d, workspace_bytes, train_modes(), (hipStream_t)stream);
}

size_t r4d_lm_head_train_workspace_bytes(int32_t N, int32_t d, int32_t ldV) {
    if (N <= 0 || d <= 0 || ldV <= 0) return 0;
    return head_layout(N, d, ldV).total * sizeof(float) + 256;
}

int r4d_lm_head_train_f32(const float* h_d, int32_t N, int32_t V, int32_t d, const r4d_lm_head* head, const int64_t* labels_src_d,
                          int32_t T, float grad_scale, float* loss_d, float* dh_d, float* dwte_d, void* workspace_d,
                          size_t workspace_bytes, void* stream) {
    const int head_bf16 = train_modes().head_bf16;                  // r4d_set_train_head_bf16, read here and handed down
    R4D_REQUIRE(h_d && head && head->wte_pad && labels_src_d && loss_d, "lm head train: null pointer");
    R4D_REQUIRE(d >= 4 && d % 4 == 0 && head->ldV % 128 == 0 && head->ldV >= V, "lm head train: d=%d ldV=%d (d %% 4 == 0, ldV a multiple of 128 >= V=%d)",
                d, head->ldV, V);
    const int ldV = head->ldV;
    int rc = check_ce(N, V, ldV, T);
    if (rc) return rc;
    R4D_REQUIRE((long long)N * ce_chunk_rows(ldV) < (1ll << 31) && (long long)ldV * d < (1ll << 31) && (long long)N * d < (1ll << 31),
                "lm head train: N=%d rows x %d chunk columns, ldV=%d x d=%d or N x d reaches 2^31 elements (32-bit index arithmetic)", N,
                ce_chunk_rows(ldV), ldV, d);
    R4D_REQUIRE((((uintptr_t)h_d | (uintptr_t)head->wte_pad | (uintptr_t)head->w3 | (uintptr_t)head->w3t | (uintptr_t)head->h2 |
                  (uintptr_t)dh_d | (uintptr_t)dwte_d | (uintptr_t)workspace_d) & 15) == 0, "lm head train: 16-byte alignment");
    const HeadLayout t = head_layout(N, d, ldV);
    if (!workspace_d || workspace_bytes < t.total * sizeof(float)) {
        set_error("lm head train: workspace %zu bytes < required %zu", workspace_bytes, t.total * sizeof(float));
        return R4D_ERR_WORKSPACE;
    }
    float* ws = (float*)workspace_d;
    return lm_head_train(h_d, N, V, d, head, labels_src_d, T, grad_scale, loss_d, ws + t.logits, dh_d, dwte_d, ws + t.tn, ws + t.ce,
                         head_bf16, (hipStream_t)stream);
}

}  // extern "C"
