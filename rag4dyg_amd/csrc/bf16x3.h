// The three-term bf16 form of an fp32 number, x = hi + mid + lo exactly (gemm_s3.hip has the derivation), and its first term alone,
// the plain-bf16 rounding of gemm_b1.hip / gemm_b1tn.hip.  ONE definition for the GEMMs, the weight-gradient GEMMs and the pool
// scan of score.hip: that a score does not depend on the shard, and that the scoring GEMM matches the scan, rests on it.
#pragma once
#include "gemm_common.h"

namespace r4d {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));          // (bf16x2 and cvt_pk_bf16: gemm_common.h)
typedef short s16x4 __attribute__((ext_vector_type(4)));            // what the transposing LDS read returns
typedef short s16x8 __attribute__((ext_vector_type(8)));

// two fp32 -> packed (hi, hi), (mid, mid), (lo, lo)
__device__ __forceinline__ void split3_pair(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
    h = cvt_pk_bf16(x0, x1);
    const float r0 = x0 - __builtin_bit_cast(float, h << 16), r1 = x1 - __builtin_bit_cast(float, h & 0xffff0000u);
    m = cvt_pk_bf16(r0, r1);
    const float s0 = r0 - __builtin_bit_cast(float, m << 16), s1 = r1 - __builtin_bit_cast(float, m & 0xffff0000u);
    l = cvt_pk_bf16(s0, s1);
}

}  // namespace r4d
