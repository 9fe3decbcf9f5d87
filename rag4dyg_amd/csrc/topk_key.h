// Order-preserving unsigned keys of the ranking kernels (topk.hip, topk_large.hip): larger value <=> larger key.
#pragma once
#include <math.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace r4d {

template <typename T> struct KeyOf;
template <> struct KeyOf<float> {
    typedef uint32_t K;
    static __device__ __forceinline__ K make(float x) {           // larger value <=> larger key; NaN sorts with -inf
        x = (x == x) ? x + 0.0f : -INFINITY;                       // -0.0 + 0.0 == +0.0
        const uint32_t b = __builtin_bit_cast(uint32_t, x);
        return b ^ (uint32_t)(((int32_t)b >> 31) | (int32_t)0x80000000);
    }
    static __device__ __forceinline__ float value(K k) {
        const uint32_t b = k ^ ((k & 0x80000000u) ? 0x80000000u : 0xffffffffu);
        return __builtin_bit_cast(float, b);
    }
};
template <> struct KeyOf<double> {
    typedef uint64_t K;
    static __device__ __forceinline__ K make(double x) {
        x = (x == x) ? x + 0.0 : -(double)INFINITY;
        const uint64_t b = __builtin_bit_cast(uint64_t, x);
        return b ^ (uint64_t)(((int64_t)b >> 63) | (int64_t)0x8000000000000000ull);
    }
    static __device__ __forceinline__ double value(K k) {
        const uint64_t b = k ^ ((k >> 63) ? 0x8000000000000000ull : 0xffffffffffffffffull);
        return __builtin_bit_cast(double, b);
    }
};
// Key 0 is below every real key (the smallest real key is that of -inf): it marks padding and consumed slots.

}  // namespace r4d
