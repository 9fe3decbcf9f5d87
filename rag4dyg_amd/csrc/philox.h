// The counter-based dropout generator of the training steps (train_ops.hip has the why): Philox-4x32-10 (Salmon et al., SC'11) and
// the block of an attention-probability element.  ONE definition for the dropout kernels and the fused training attention, which
// regenerates the masks launch_dropout draws (attention_train_fused.hip).
#pragma once
#include "common.h"

namespace r4d {

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u; k.y += 0xBB67AE85u;
    }
    return c;
}
// element idx = pbase + (bh * T + i) * ld + j of a P-shaped block -> the Philox block c = idx / 4, word idx % 4
__device__ __forceinline__ uint4 attn_philox(unsigned long long c, DropKey key, unsigned site) {
    return philox4x32_10(make_uint4((unsigned)c, site + ((unsigned)(c >> 32) << 16), key.step_lo, key.step_hi),
                         make_uint2(key.seed_lo, key.seed_hi));
}

}  // namespace r4d
