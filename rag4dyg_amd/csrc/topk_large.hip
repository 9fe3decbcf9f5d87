// Exact per-row top-k for 64 < k <= 2048 on gfx950, in the canonical order of the build (key descending, list position
// ascending == np.argsort(-x, kind='stable') after the key mapping of topk_key.h).  topk.hip hands a wavefront's lane r the
// r-th winner, so it ends at 64; here a workgroup SELECTS by value and then sorts only what it selected:
//   * a workgroup of 1024 threads owns LG_CHUNK = 16384 consecutive list positions of one row, 16 consecutive ones per thread,
//     as keys in registers (the row is read once, 64 bytes per lane);
//   * the min(k, chunk length)-th largest key comes out of a radix select on the 32-bit key, 8 bits a pass: an LDS histogram
//     (ds atomics, a thread adds a run of equal digits once), a suffix scan of the 256 bins by one wavefront, the next pass
//     over the keys that share the selected prefix.  A pass whose selected bin holds exactly what is still needed ends it;
//   * every key above the selected prefix survives, and of the keys equal to it the `need` lowest positions: a workgroup
//     prefix sum in position order (both counts in one word) gives each survivor its slot;
//   * the survivors -- k at the most -- are sorted by the bitonic network of sort_chunks_kernel on (inverted key, position): all
//     pairs are distinct, the order is unique;
//   * they leave as candidates [rows, nchunks * k] with their global indices, or as the result when the row is one chunk.
// Longer rows repeat the launch over the candidate lists (idx_in) until one chunk is left: 16384 >= 8 k, so every level shrinks
// the list at least 4-fold.  No workgroup waits on another one: a level ends with its launch.
#include "common.h"
#include "topk_key.h"

namespace r4d {

constexpr int LG_E = 16;                        // list positions per thread
constexpr int LG_THREADS = 1024;
constexpr int LG_CHUNK = LG_E * LG_THREADS;     // list positions per workgroup
static_assert(LG_CHUNK >= 8 * TOPK_MAX_K, "a level must shrink its list");

typedef float LgVec4 __attribute__((ext_vector_type(4), aligned(4)));   // rows start at any element (topk.hip: Vec4)

// grid (nchunks, rows), block 1024.  vals [rows, ld], n list positions per row; idx_in (nullable) their global indices, else
// index = position + index_offset.  out_v / out_i [rows, nchunks, k]; sortn = the power of two >= k.
__global__ __launch_bounds__(LG_THREADS) void topk_large_kernel(const float* __restrict__ vals, const long long* __restrict__ idx_in,
                                                                 int n, long long ld, int k, int sortn, long long index_offset,
                                                                 int nchunks, float* __restrict__ out_v, long long* __restrict__ out_i) {
    __shared__ unsigned s_hist[256];
    __shared__ uint32_t s_sk[TOPK_MAX_K];          // survivors: inverted key (ascending == descending value), list position
    __shared__ uint32_t s_sp[TOPK_MAX_K];
    __shared__ unsigned s_wsum[LG_THREADS / 64];
    __shared__ unsigned s_sel[3];                  // selected digit, what is still needed inside it, "the bin is exactly that"
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int chunk = blockIdx.x, row = blockIdx.y;
    const float* v = vals + (long long)row * ld;
    const int col0 = chunk * LG_CHUNK + t * LG_E;
    const int len = min(LG_CHUNK, n - chunk * LG_CHUNK);
    const int kk = min(k, len);                    // a chunk shorter than k gives all it has

    uint32_t c[LG_E];                              // keys of positions [col0, col0 + 16); 0 = beyond the list
#pragma unroll
    for (int j = 0; j < LG_E / 4; ++j) {
        const int c0 = col0 + 4 * j;
        if (c0 + 3 < n) {
            const LgVec4 x = *reinterpret_cast<const LgVec4*>(v + c0);
            c[4 * j] = KeyOf<float>::make(x.x); c[4 * j + 1] = KeyOf<float>::make(x.y);
            c[4 * j + 2] = KeyOf<float>::make(x.z); c[4 * j + 3] = KeyOf<float>::make(x.w);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {          // clamped address, value masked
                const uint32_t key = KeyOf<float>::make(v[min(c0 + e, n - 1)]);
                c[4 * j + e] = (c0 + e < n) ? key : 0u;
            }
        }
    }

    // ---- radix select: prefix P of the kk-th largest key, over the top (32 - shift) bits
    uint32_t P = 0;
    unsigned need = (unsigned)kk;
    int shift = 24;
    for (int s = 24; s >= 0; s -= 8) {
        if (t < 256) s_hist[t] = 0;
        __syncthreads();
        int run_d = 0;
        unsigned run_n = 0;
#pragma unroll
        for (int e = 0; e < LG_E; ++e) {
            const bool in = c[e] != 0 && ((c[e] >> s) >> 8) == P;      // (two shifts: s + 8 is 32 in the first pass)
            const int d = (int)((c[e] >> s) & 255u);
            if (in) {
                if (run_n && d != run_d) { atomicAdd(&s_hist[run_d], run_n); run_n = 0; }
                run_d = d; ++run_n;
            }
        }
        if (run_n) atomicAdd(&s_hist[run_d], run_n);
        __syncthreads();
        if (w == 0) {                               // lane L: bins 255 - 4L .. 252 - 4L, descending digit
            unsigned h[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] = s_hist[255 - (4 * lane + j)];
            const unsigned tot = h[0] + h[1] + h[2] + h[3];
            unsigned incl = tot;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned y = __shfl_up(incl, o);
                if (lane >= o) incl += y;
            }
            unsigned excl = incl - tot;             // keys in the bins above this lane's
#pragma unroll
            for (int j = 0; j < 4; ++j) {           // exactly one bin of the 256 holds the need-th key
                if (excl < need && need <= excl + h[j]) {
                    s_sel[0] = 255u - (unsigned)(4 * lane + j);
                    s_sel[1] = need - excl;
                    s_sel[2] = (h[j] == need - excl) ? 1u : 0u;
                }
                excl += h[j];
            }
        }
        __syncthreads();
        P = (P << 8) | s_sel[0];
        need = s_sel[1];
        shift = s;
        if (s_sel[2]) break;                        // workgroup-uniform: every key with this prefix is taken
    }

    // ---- slots: keys above the prefix first (kk - need of them), then the `need` lowest positions that equal it
    unsigned ngt = 0, neq = 0;
#pragma unroll
    for (int e = 0; e < LG_E; ++e) {
        const uint32_t hi = c[e] >> shift;
        ngt += (c[e] != 0 && hi > P) ? 1u : 0u;
        neq += (c[e] != 0 && hi == P) ? 1u : 0u;
    }
    const unsigned mine = ngt | (neq << 16);        // both counts stay below 2^16 (16384 positions)
    unsigned incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    if (lane == 63) s_wsum[w] = incl;
    __syncthreads();
    unsigned before = incl - mine;
    for (int j = 0; j < w; ++j) before += s_wsum[j];
    unsigned g = before & 0xffffu, q = before >> 16;
    const unsigned eq0 = (unsigned)kk - need;
#pragma unroll
    for (int e = 0; e < LG_E; ++e) {
        const uint32_t hi = c[e] >> shift;
        const bool gt = c[e] != 0 && hi > P, eq = c[e] != 0 && hi == P;
        unsigned slot = 0xffffffffu;
        if (gt) slot = g++;
        if (eq) { if (q < need) slot = eq0 + q; ++q; }
        if (slot < (unsigned)kk) { s_sk[slot] = ~c[e]; s_sp[slot] = (uint32_t)(col0 + e); }
    }
    for (int j = kk + t; j < sortn; j += LG_THREADS) { s_sk[j] = 0xffffffffu; s_sp[j] = 0xffffffffu; }   // above every real pair
    __syncthreads();

    // ---- bitonic network over sortn pairs, ascending in (inverted key, position)
    for (int size = 2; size <= sortn; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (t < (sortn >> 1)) {
                const int l = ((t / stride) * 2 * stride) + (t % stride), r = l + stride;
                const bool asc = (l & size) == 0;
                const uint32_t kl = s_sk[l], kr = s_sk[r], il = s_sp[l], ir = s_sp[r];
                const bool less = (kr < kl) | ((kr == kl) & (ir < il));
                if (less == asc) { s_sk[l] = kr; s_sp[l] = ir; s_sk[r] = kl; s_sp[r] = il; }
            }
            __syncthreads();
        }
    }

    const long long obase = ((long long)row * nchunks + chunk) * k;
    for (int j = t; j < k; j += LG_THREADS) {
        float val = -INFINITY;                      // padding of a chunk shorter than k, as topk.hip pads
        long long gi = 0x7fffffffffffffffLL;
        if (j < kk) {
            const uint32_t pos = s_sp[j];
            val = KeyOf<float>::value(~s_sk[j]);
            gi = idx_in ? idx_in[(long long)row * ld + pos] : (long long)pos + index_offset;
        }
        out_v[obase + j] = val;
        out_i[obase + j] = gi;
    }
}

// Candidate lists of every level but the last, behind the block of ticket counters that r4d_score_topk_f32's scan clears at
// the start of every top-k workspace.  Never below what the k = 64 launch of the same rows asks for, so that a size query
// does not shrink where the route changes.
size_t topk_large_ws_bytes(int rows, int n, int k) {
    size_t total = align_up((size_t)rows * sizeof(unsigned), 256);
    if (k <= TOPK_MAX_K) {
        long long cur = n;
        while (cur > LG_CHUNK) {
            const long long nchunks = (cur + LG_CHUNK - 1) / LG_CHUNK;
            total += align_up((size_t)rows * nchunks * k * 4, 256) + align_up((size_t)rows * nchunks * k * 8, 256);
            cur = nchunks * k;
        }
    }
    const size_t small = topk_ws_bytes<float>(rows, n, 64);
    return total + 256 > small ? total + 256 : small;
}

// the caller (topk_rows) has checked k, rows, n and the workspace size
int topk_large_rows(const float* vals, const long long* idx_in, int rows, int n, long long ld, int k, long long index_offset,
                    float* out_v, long long* out_i, void* ws, hipStream_t s) {
    int sortn = 128;
    while (sortn < k) sortn <<= 1;
    char* wp = (char*)ws + align_up((size_t)rows * sizeof(unsigned), 256);
    if (n <= LG_CHUNK) R4D_BRANCH(TOPKL_ONE); else R4D_BRANCH(TOPKL_MULTI);
    const float* cv = vals;
    const long long* ci = idx_in;
    long long cur = n, cld = ld;
    while (true) {
        const int nchunks = (int)((cur + LG_CHUNK - 1) / LG_CHUNK);
        float* ov = out_v;
        long long* oi = out_i;
        if (nchunks > 1) {
            ov = (float*)wp; wp += align_up((size_t)rows * nchunks * k * 4, 256);
            oi = (long long*)wp; wp += align_up((size_t)rows * nchunks * k * 8, 256);
        }
        {
            ProfScope prof(PK_TOPK, (double)rows * cur * (4 + (ci ? 8 : 0)), s);
            hipLaunchKernelGGL(topk_large_kernel, dim3(nchunks, rows), dim3(LG_THREADS), 0, s, cv, ci, (int)cur, cld, k, sortn,
                               index_offset, nchunks, ov, oi);
            R4D_CHECK_LAUNCH("topk_large");
        }
        if (nchunks == 1) break;
        cv = ov; ci = oi; cur = (long long)nchunks * k; cld = cur; index_offset = 0;
    }
    return R4D_OK;
}

}  // namespace r4d
