// The pieces the per-row selection kernels share (sampling.hip: sample_advance_kernel, beam.hip: beam_rows_kernel): one workgroup of
// 16 wavefronts per row, 64-bit wavefront sums and scans, the 256-bucket histogram of one radix level with its bucket search, and
// the two index-order routines.  Every sum is an integer sum, so LDS atomics may build the histograms.
#pragma once
#include "common.h"
#include "topk_key.h"

namespace r4d {

constexpr int SNT = 1024, SNW = SNT / 64;
constexpr int SAMPLE_LDS_COLS = 16384;
typedef unsigned long long u64;
typedef KeyOf<float> FK;

__device__ __forceinline__ u64 shfl_xor64(u64 v, int o) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_up64(u64 v, int o) {
    const unsigned lo = (unsigned)__shfl_up((int)(unsigned)v, o), hi = (unsigned)__shfl_up((int)(unsigned)(v >> 32), o);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl64(u64 v, int src) {
    const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += shfl_xor64(v, o);
    return v;
}
__device__ __forceinline__ u64 wave_max64(u64 v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const u64 t = shfl_xor64(v, o); v = t > v ? t : v; }
    return v;
}
__device__ __forceinline__ u64 wave_incl_scan64(u64 v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const u64 t = shfl_up64(v, o); if (lane >= o) v += t; }
    return v;
}

// hist[bucket] += MASS ? q : 1 for the lanes with `valid`, called by whole wavefronts.  Keys of one row crowd into a few buckets at
// the upper levels, and 64 lanes on one LDS address go one after the other: lanes that share the first lane's bucket are summed
// in registers first (twice), the rest go to the atomic unit directly
template <bool MASS> __device__ __forceinline__ void hist_add(u64* hist, bool valid, int bucket, u64 q, int lane) {
    for (int round = 0; round < 2; ++round) {
        const u64 m = __ballot(valid);
        if (!m) return;
        const int leader = __ffsll((long long)m) - 1;
        const int lb = __shfl(bucket, leader);
        const bool mine = valid && bucket == lb;
        const u64 same = __ballot(mine);
        if (__popcll(same) < 4) break;
        const u64 s = MASS ? wave_sum64(mine ? q : 0ull) : (u64)__popcll(same);
        if (lane == leader) atomicAdd(&hist[lb], s);
        valid = valid && !mine;
    }
    if (valid) atomicAdd(&hist[bucket], MASS ? q : 1ull);
}

struct SelectOut { int bucket; u64 above, bmass, target; };      // (in LDS)
// Wavefront 0: the bucket, walking DOWN from 255, in which the running sum first exceeds `target` (out->bucket = -1: the sum of all
// buckets does not), the sum of the buckets above it and its own.  from_top_p: target = floor(top_p * the sum of all buckets)
__device__ __forceinline__ void find_bucket(const u64* hist, u64 target, bool from_top_p, float top_p, SelectOut* out, int lane) {
    u64 h[4], loc = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { h[i] = hist[255 - 4 * lane - i]; loc += h[i]; }
    const u64 incl = wave_incl_scan64(loc, lane), excl = incl - loc, total = shfl64(incl, 63);
    if (from_top_p) target = (u64)((double)top_p * (double)total);
    if (lane == 0) { out->target = target; if (total <= target) out->bucket = -1; }
    if (excl <= target && target < incl) {
        u64 c = excl;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (target < c + h[i]) { out->bucket = 255 - 4 * lane - i; out->above = c; out->bmass = h[i]; break; }
            c += h[i];
        }
    }
}

// Index order.  The row in SNW contiguous segments of L columns (L a multiple of 64): seg[w] = the sum of f over segment w, by
// wavefront w.  Returns the sum over the row; the caller synchronises before seg is written again
template <class F> __device__ __forceinline__ u64 seg_sums(int V, int L, F f, u64* seg) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int lo = wid * L, hi = min(V, lo + L);
    u64 acc = 0;
    for (int j = lo + lane; j < hi; j += 64) acc += f(j);
    acc = wave_sum64(acc);
    if (lane == 0) seg[wid] = acc;
    __syncthreads();
    u64 total = 0;
#pragma unroll
    for (int w = 0; w < SNW; ++w) total += seg[w];
    return total;
}
// ... and the lowest index j whose inclusive prefix sum of f exceeds `target` (-1: none): the segment from seg, then its
// wavefront alone -- a contiguous chunk of L / 64 columns per lane, a scan of the 64 chunk sums, a walk through one chunk
template <class F> __device__ __forceinline__ int seg_find(int V, int L, F f, u64 target, const u64* seg, int* res) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int s = -1;
    u64 c = 0;
    for (int w = 0; w < SNW; ++w) {
        if (target < c + seg[w]) { s = w; break; }
        c += seg[w];
    }
    if (tid == 0) *res = -1;
    __syncthreads();
    if (wid == s) {
        const u64 t = target - c;
        const int C = L / 64, lo = min(V, s * L + lane * C), hi = min(V, lo + C);
        u64 acc = 0;
        for (int j = lo; j < hi; ++j) acc += f(j);
        const u64 incl = wave_incl_scan64(acc, lane), excl = incl - acc;
        if (excl <= t && t < incl) {
            u64 cc = excl;
            for (int j = lo; j < hi; ++j) {
                cc += f(j);
                if (t < cc) { *res = j; break; }
            }
        }
    }
    __syncthreads();
    return *res;
}

}  // namespace r4d
