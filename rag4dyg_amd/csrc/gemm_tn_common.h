// What the two weight-gradient ("TN") kernels share, gemm_s3tn.hip (bf16x3) and gemm_b1tn.hip (plain bf16): the shape, the slice
// geometry on the host, and the kernel text both spell the same way -- as MACROS over the kernels' own locals, not functions (a
// function around the accumulators or the staging registers changes the register allocation: DESIGN_LOG 12.15).  The tail of both
// kernels is shared as text, gemm_tn_tail.h.  What differs stays in its file: the number of LDS images, the split or the rounding,
// the fragment sets, the products, the B item's addressing, the launch bounds.
#pragma once
#include "bf16x3.h"

namespace r4d {

struct TnShape {
    int M;                 // token rows in all
    int I, J, lda, ldb;    // features of X / dY and their row strides (floats)
    int kper;              // token rows per slice (multiple of 32)
};

typedef __attribute__((address_space(3))) s16x4* lds_tr_t;

// host: S wanted slices -> the shape (tn_row_slices(M, S) slices hold rows) and its grid, one workgroup per 128 x 256 tile and slice
static inline TnShape tn_shape(int I, int J, int M, int lda, int ldb, int S) {
    return TnShape{M, I, J, lda, ldb, cdiv(cdiv(M, S), 32) * 32};
}
static inline dim3 tn_grid(const TnShape& sh) { return dim3((sh.I / 128) * (sh.J / 256), 1, cdiv(sh.M, sh.kper)); }

}  // namespace r4d

// staging coordinates of the A item: a thread owns 8 consecutive features of one token (token = tid >> 4, chunk = tid & 15); the
// 16-byte chunk index of the LDS row is XOR-ed with (token & 3) << 2
#define TN_A_ITEM                                                                                  \
    const int a_tok = tid >> 4, a_ch = tid & 15;                                                   \
    const int a_voff = (a_tok * g.lda + i0 + a_ch * 8) * 4;                                        \
    const int a_dst = a_tok * A_ROW + ((a_ch ^ ((a_tok & 3) << 2)) << 4);
// column sums over the staged dY items of a k-tile that belongs to this slice (the registers hold k-tile KT)
#define TN_COLSUM(KT)                                                                              \
    if (do_cs && (KT) < nkt) {                                                                     \
        _Pragma("unroll") for (int r = 0; r < 2; ++r) {                                            \
            const f32x4 c0_ = __builtin_bit_cast(f32x4, rb[r][0]), c1_ = __builtin_bit_cast(f32x4, rb[r][1]); \
            _Pragma("unroll") for (int e = 0; e < 4; ++e) { cs[e] += c0_[e]; cs[4 + e] += c1_[e]; } \
        }                                                                                          \
    }
// the pipeline both kernels run over their own LOAD(k-tile) / STORE(stage) / ITER(stage) macros: k-tile 0 staged and k-tile 1
// requested before the loop, then one ITER per k-tile on alternating stages -- two per trip, so the stage is a constant in each
#define TN_PIPELINE(LOAD, STORE, ITER)                                                             \
    LOAD(0)                                                                                        \
    TN_COLSUM(0)                                                                                   \
    STORE(0)                                                                                       \
    LOAD(1)                                                                                        \
    __syncthreads();                                                                               \
    int kt = 0;                                                                                    \
    for (; kt + 1 < nkt; kt += 2) {                                                                \
        ITER(0)                                                                                    \
        { ++kt; ITER(1) }                                                                          \
        --kt;                                                                                      \
    }                                                                                              \
    if (kt < nkt) ITER(0)
// transposed fragment reads.  Lane l: h = l >> 5 (tokens 8h .. 8h+7 of the k-step), 16-lane group g16 = (l >> 4) & 1
// (features 16 g16 .. +15 of the 32-wide tile), q = (l & 15) >> 2 (token row of the 4 x 16 block), p = l & 3 (features
// 4p .. 4p+3 of the group): address = row (16 s + 8 h + 4 u + q), chunk ((F / 8) + 2 g16 + (p >> 1)) ^ (q << 2), byte 8 (p & 1).
// Each kernel forms its lanes' offsets at s = u = 0 itself (fh, fg, fq, fp for h, g16, q, p): the two spell the sum in a different
// order, and one spelling for both changed gemm_b1tn's register allocation (DESIGN_LOG 12.19).
#define TN_TR(PTR) __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_t)(PTR))
#define TN_FRAG(DST, BASE, ROWB, S)                                                                \
    {                                                                                              \
        const s16x4 lo_ = TN_TR((BASE) + (16 * (S)) * (ROWB)), hi_ = TN_TR((BASE) + (16 * (S) + 4) * (ROWB)); \
        const s16x8 v_ = __builtin_shufflevector(lo_, hi_, 0, 1, 2, 3, 4, 5, 6, 7);                \
        DST = __builtin_bit_cast(u32x4, v_);                                                       \
    }
