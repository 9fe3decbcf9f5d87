// The two-term fp16 form of an fp32 number (gemm_h2.hip, attention_h2.hip):  x = hi + 2^-11 lo' + e,  hi = RN16(x),
// lo' = RN16((x - hi) 2^11),  |e| <= 2^-22 |x|  (the header of gemm_h2.hip has the derivation and the range).
//
// split2_pair / split2_vq form the second term with ONE mixed-precision fma per element: lo' = RN16(fma(hi, -2^11, q)), q = 2^11 x.
// hi 2^11, q and their difference are exact in fp32, so the fma hands RN16 the same real number as (x - hi) 2^11 does: the same
// bits for every finite x (a hi that overflows gives a non-finite lo' either way, inf or NaN).  v_fma_mixlo_f16 / v_fma_mixhi_f16
// read hi as the fp16 half it already is and write the half of the destination that is wanted: no conversion back to fp32, no
// second v_cvt_pk.  hipcc does not select them from C (fma of a converted half), so they stand as inline asm, not volatile: the
// compiler schedules and drops them like any other arithmetic.
//
// What an asm statement READS here is only the result of a plain VALU instruction the compiler emitted itself (the packed multiply
// that forms q, v_cvt_pk_f16_f32) or of the other statement, never a caller's value as it comes.  The compiler inserts the wait
// states gfx950 wants between a producer and a consumer it knows -- one after a transcendental (v_exp_f32) in front of a VALU that
// reads its result, two in front of a DPP read -- and does not look inside inline asm: a mix instruction that read a v_exp_f32
// result directly lost second terms in the attention kernels.  build.py checks every listing (check_h2_asm_neighbours).
#pragma once

namespace r4d {

typedef float h2_f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h2_f16x2 __attribute__((ext_vector_type(2)));

constexpr float H2_A_PRESCALE = 0.25f;        // 2^-2 on an activation operand (exact), undone by the consumer
constexpr float H2_A_UNSCALE = 4.0f;
constexpr float H2_LO_SCALE = 2048.0f;        // 2^11 on the second term of BOTH operands
constexpr float H2_LO_UNSCALE = 1.0f / 2048.0f;

// two fp32 ALREADY scaled, v and q = 2^11 v -> packed (hi, hi), (lo', lo'): a v_cvt_pk and two mix instructions.  For callers
// that form v and q themselves, packed over another pairing than the one the words want (the c_fc line epilogue of gemm_h2p)
__device__ __forceinline__ void split2_vq(float v0, float v1, float q0, float q1, unsigned& h, unsigned& l) {
    const h2_f32x2 v = {v0, v1};
    h = __builtin_bit_cast(unsigned, __builtin_convertvector(v, h2_f16x2));     // v_cvt_pk_f16_f32: RNE
    unsigned ll;
    asm("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(ll) : "v"(h), "s"(-H2_LO_SCALE), "v"(q0));     // (the high half: written next)
    asm("v_fma_mixhi_f16 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(ll) : "v"(h), "s"(-H2_LO_SCALE), "v"(q1));
    l = ll;
}

// two fp32 -> packed (hi, hi), (lo', lo') of x * PRE: five instructions, four without the prescale
template <bool PRESCALE>
__device__ __forceinline__ void split2_pair(float x0, float x1, unsigned& h, unsigned& l) {
    const h2_f32x2 x = {x0, x1};
    const h2_f32x2 v = PRESCALE ? x * H2_A_PRESCALE : x;
    const h2_f32x2 q = x * ((PRESCALE ? H2_A_PRESCALE : 1.0f) * H2_LO_SCALE);  // exact
    split2_vq(v.x, v.y, q.x, q.y, h, l);
}

// The conversion form of the same split: hi back to fp32, the rest, its scaling, a second v_cvt_pk (seven instructions with the
// prescale).  The h2 words keep it: with the mix form their launches (c_attn, attention) measured no faster (DESIGN_LOG 12.30), and
// the attention kernels hand in results of v_exp_f32, which inline asm must not read directly.
template <bool PRESCALE>
__device__ __forceinline__ void split2_pair_cvt(float x0, float x1, unsigned& h, unsigned& l) {
    h2_f32x2 v = {x0, x1};
    if (PRESCALE) v = v * H2_A_PRESCALE;
    const h2_f16x2 hh = __builtin_convertvector(v, h2_f16x2);         // v_cvt_pk_f16_f32: RNE
    const h2_f32x2 hf = __builtin_convertvector(hh, h2_f32x2);
    const h2_f32x2 r = (v - hf) * H2_LO_SCALE;                        // exact
    const h2_f16x2 ll = __builtin_convertvector(r, h2_f16x2);
    h = __builtin_bit_cast(unsigned, hh);
    l = __builtin_bit_cast(unsigned, ll);
}

// "h2 word" of an element: hi in the low half, lo' in the high half -- as an MFMA operand a register of such words is
// two k-slots (hi, lo') of ONE element.  Against it the other operand takes the forms
//     F1 = (hi, 0)    ->  sum hi.hi                    (first accumulator set)
//     F2 = (lo', hi)  ->  sum hi.lo' + lo'.hi          (second set, factor 2^11)
// so the three partial products of the f16x2 form cost two instructions per 8 elements (attention_h2.hip).
template <bool PRESCALE>
__device__ __forceinline__ void h2_words(float x0, float x1, unsigned& w0, unsigned& w1) {
    unsigned h, l;
    split2_pair_cvt<PRESCALE>(x0, x1, h, l);
    w0 = __builtin_amdgcn_perm(l, h, 0x05040100u);                    // bytes: h.0 h.1 l.0 l.1
    w1 = __builtin_amdgcn_perm(l, h, 0x07060302u);                    //        h.2 h.3 l.2 l.3
}
__device__ __forceinline__ void h2_forms(float x0, float x1, unsigned& f1_0, unsigned& f1_1, unsigned& f2_0, unsigned& f2_1) {
    unsigned h, l;
    split2_pair_cvt<false>(x0, x1, h, l);
    f1_0 = h & 0xffffu;
    f1_1 = h >> 16;
    f2_0 = __builtin_amdgcn_perm(h, l, 0x05040100u);                  // bytes: l.0 l.1 h.0 h.1
    f2_1 = __builtin_amdgcn_perm(h, l, 0x07060302u);
}

}  // namespace r4d
