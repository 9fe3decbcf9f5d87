// The row-major epilogue of the MFMA GEMM kernels gemm_f32_kc, gemm_s3, gemm_s3p and gemm_h2 (gemm_h2p.hip keeps a copy of its
// own, see there): bias, the fused kind EPI, and the stores of a wavefront's TM x TN accumulator tiles of 32 x 32.
//
// This is TEXT, included inside the kernel body at the point of use, not a function: as a __forceinline__ function template
// (value lambda, or accumulators by reference) it reassigns registers through the whole of the 256-VGPR kernels, k-loop
// included -- a different kernel that would need its own timing (DESIGN_LOG 12.15).  Included as text, every kernel's assembly
// is what its own copy gave (tools/isa_equal.py).  A .h so that build.py's dependency scan sees it.
//
// C/D layout of a 32 x 32 tile: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5), independent of the data type.
// The epilogue kind is a TEMPLATE parameter and interior tiles take a path without bounds checks: with a runtime switch and
// per-element guards the 32 outputs of a lane cost ~2,800 instructions (ten branches each) -- at K = 512 that, not the stores
// themselves, was the 8 % between a launch (130 TF) and the k-loop asymptote (143).  (Measured and dropped earlier: float4
// stores through swapped MFMA operands; two-iteration load prefetch.)
//
// In scope at the point of inclusion:
//     constants BM, BN, WM, WN, TM, TN, EPI;   wave / lane coordinates wm, wn, li, lh;   the tile origin m0, n0;
//     float* C, const float* biasg (nullable), const float* residg (the second buffer), g with .M .N .ldc .ldr
// Parameters (macros of the including kernel; all #undef-ed here):
//     EPILOGUE_VALUE(i, j, r)      the fp32 result element r of accumulator tile (i, j), before the bias
//     EPILOGUE_SCALE_DIVISOR       optional: the divisor of EPI_SCALE_DIV (only gemm_f32_kc's shape block carries one)
//     EPILOGUE_EDGE_PRELOAD        optional, 0 / 1: an edge tile loads the 16 second-buffer values of an accumulator tile ahead of its
//                             element loop (the one-workgroup-per-tile kernels that were written that way keep their instruction
//                             order) instead of one by one inside it
//     EPILOGUE_DBG_NO_STORES       optional, 0 / 1: ablation builds (KC_DBG bit 4) keep the values alive but store (almost) nothing
//     EPILOGUE_PAIR_WORDS          optional, 0 / 1: an interior tile forms the two stored words of a register pair ahead of the two stores
//                             (the h2-word output needs the pair; gemm_h2 was written that way for all its kinds and keeps its
//                             instruction order) instead of each word at its store
// Unused arms are dead code under the constant EPI; the second buffer's descriptor is an empty range over C for kinds without one.
// The fragment does not return: a persistent kernel goes on to its next tile behind it.
#ifndef EPILOGUE_VALUE
#error "gemm_epilogue_rowmajor.h: define EPILOGUE_VALUE(i, j, r) first"
#endif
#ifndef EPILOGUE_EDGE_PRELOAD
#define EPILOGUE_EDGE_PRELOAD 0
#endif
#ifndef EPILOGUE_DBG_NO_STORES
#define EPILOGUE_DBG_NO_STORES 0
#endif
#ifndef EPILOGUE_PAIR_WORDS
#define EPILOGUE_PAIR_WORDS 0
#endif
{
    static_assert(EPI != EPI_H2WORDS || EPILOGUE_PAIR_WORDS, "the h2-word output forms its two words from the pair");
    // the second buffer is read (residual; training backward: the pre-activation) or written (training forward: the pre-activation)
    // GELU_KEEP_BF16 (gemm_b1 only): GELU_KEEP whose C is bf16 [M, N] -- ldc counts bf16 elements, N and ldc are even; NONE_BF16 and
    // GELU_BF16 (gemm_b1 only): the plain result / gelu(v) as bf16 in the same way, no second buffer
    constexpr bool KEEPS = EPI == EPI_GELU_KEEP || EPI == EPI_GELU_KEEP_BF16, GELUS = EPI == EPI_GELU || EPI == EPI_GELU_BF16 || KEEPS;
    constexpr bool C_BF16 = EPI == EPI_GELU_KEEP_BF16 || EPI == EPI_NONE_BF16 || EPI == EPI_GELU_BF16;
    constexpr bool USES_R = EPI == EPI_RESIDUAL || KEEPS || EPI == EPI_GELU_GRAD;
    constexpr bool LOADS_R = EPI == EPI_RESIDUAL || EPI == EPI_GELU_GRAD;
    constexpr int C_SZ = C_BF16 ? 2 : 4;
    const bool interior = (m0 + BM <= g.M) & (n0 + BN <= g.N);       // wave-uniform
    if (interior) {
        // buffer stores / loads from the tile's origin: the lane's byte offset is computed once (voffset), the
        // (compile-time row) * ld part lives on the scalar unit (soffset) -- one VALU instruction per element (the bias add)
        // (bf16 C: a lane pair exchanges one value per register pair, so that the even lane stores columns (li, li + 1) of row r2
        //  and the odd lane the same columns of row r2 + 1 as ONE 32-bit word each: the row of the odd lane is one further down)
        const int lane_c = C_BF16 ? ((wm * WM + 4 * lh + (li & 1)) * g.ldc + wn * WN + (li & ~1)) * 2
                                  : ((wm * WM + 4 * lh) * g.ldc + wn * WN + li) * 4;
        const int lane_r = ((wm * WM + 4 * lh) * g.ldr + wn * WN + li) * 4;
        const __amdgpu_buffer_rsrc_t c_rsrc = __builtin_amdgcn_make_buffer_rsrc(
            C_BF16 ? (float*)((unsigned short*)C + (long long)m0 * g.ldc + n0) : C + (long long)m0 * g.ldc + n0, 0,
            ((BM - 1) * g.ldc + BN) * C_SZ, 0x00020000);
        const __amdgpu_buffer_rsrc_t r_rsrc = __builtin_amdgcn_make_buffer_rsrc(       // (unused kinds: an empty range over C)
            USES_R ? const_cast<float*>(residg) + (long long)m0 * g.ldr + n0 : C, 0,
            USES_R ? ((BM - 1) * g.ldr + BN) * 4 : 0, 0x00020000);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const float bias = biasg ? biasg[n0 + wn * WN + j * 32 + li] : 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                float res[16];
                if (LOADS_R) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        res[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                            r_rsrc, lane_r, ((i * 32 + (r & 3) + 8 * (r >> 2)) * g.ldr + j * 32) * 4, 0));
                }
#pragma unroll
                for (int r2 = 0; r2 < 16; r2 += 2) {
                    f32x2 v2 = {EPILOGUE_VALUE(i, j, r2) + bias, EPILOGUE_VALUE(i, j, r2 + 1) + bias};
                    if (KEEPS) {                                      // training forward: the pre-activation goes to the second buffer
#pragma unroll
                        for (int h2 = 0; h2 < 2; ++h2) {
                            const int r = r2 + h2;
                            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, h2 ? v2.y : v2.x), r_rsrc, lane_r,
                                                                  ((i * 32 + (r & 3) + 8 * (r >> 2)) * g.ldr + j * 32) * 4, 0);
                        }
                    }
                    if (GELUS) v2 = gelu_new2(v2);
                    else if (EPI == EPI_RESIDUAL) { v2.x += res[r2]; v2.y += res[r2 + 1]; }
                    else if (EPI == EPI_GELU_GRAD) { v2.x *= gelu_new_grad(res[r2]); v2.y *= gelu_new_grad(res[r2 + 1]); }
#ifdef EPILOGUE_SCALE_DIVISOR
                    else if (EPI == EPI_SCALE_DIV) { v2.x = v2.x / EPILOGUE_SCALE_DIVISOR; v2.y = v2.y / EPILOGUE_SCALE_DIVISOR; }
#endif
                    else if (EPI == EPI_HALF_PLUS) { v2.x = (v2.x + 1.0f) / 2.0f; v2.y = (v2.y + 1.0f) / 2.0f; }     // train_retriever.py:438
                    if constexpr (C_BF16) {                           // rows r2 / r2 + 1 of this lane's column -> one word of two columns
                        const float vx = v2.x, vy = v2.y;
                        const float send = (li & 1) ? vx : vy;
                        const float recv = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, send), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
                        const unsigned word = (li & 1) ? cvt_pk_bf16(recv, vy) : cvt_pk_bf16(vx, recv);
                        __builtin_amdgcn_raw_buffer_store_b32(word, c_rsrc, lane_c, ((i * 32 + (r2 & 3) + 8 * (r2 >> 2)) * g.ldc + j * 32) * 2, 0);
                        continue;
                    }
                    unsigned o2[2] = {0u, 0u};
                    if (EPILOGUE_PAIR_WORDS) {
                        const float vx = v2.x, vy = v2.y;     // (copies first: __builtin_bit_cast on an ext-vector ELEMENT reads element 0)
                        o2[0] = __builtin_bit_cast(unsigned int, vx); o2[1] = __builtin_bit_cast(unsigned int, vy);
                        if (EPI == EPI_H2WORDS) h2_words<true>(v2.x, v2.y, o2[0], o2[1]);     // C is the uint32 word image of the result (attention_h2.hip)
                    }
#pragma unroll
                    for (int h2 = 0; h2 < 2; ++h2) {
                        const int r = r2 + h2;
                        const float v = h2 ? v2.y : v2.x;
                        if (!EPILOGUE_DBG_NO_STORES || v == 12345.678f)      // (ablation: (almost) never true, keeps v alive)
                            __builtin_amdgcn_raw_buffer_store_b32(EPILOGUE_PAIR_WORDS ? o2[h2] : __builtin_bit_cast(unsigned int, v), c_rsrc, lane_c,
                                                                  ((i * 32 + (r & 3) + 8 * (r >> 2)) * g.ldc + j * 32) * 4, 0);
                    }
                }
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < TN; ++j) {                               // edge tiles: clamped reads, guarded stores
            const int col = n0 + wn * WN + j * 32 + li;
            const bool col_ok = col < g.N;
            const int colc = min(col, g.N - 1);
            const float bias = biasg ? biasg[colc] : 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                float res[16];
                if (EPILOGUE_EDGE_PRELOAD && LOADS_R) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = min(m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh, g.M - 1);
                        res[r] = residg[(long long)row * g.ldr + colc];
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    float v = EPILOGUE_VALUE(i, j, r) + bias;
                    if (!EPILOGUE_EDGE_PRELOAD && LOADS_R) res[r] = residg[(long long)min(row, g.M - 1) * g.ldr + colc];
                    if (KEEPS && row < g.M && col_ok) const_cast<float*>(residg)[(long long)row * g.ldr + col] = v;
                    if (GELUS) v = gelu_new1(v);
                    else if (EPI == EPI_RESIDUAL) v += res[r];
                    else if (EPI == EPI_GELU_GRAD) v *= gelu_new_grad(res[r]);
#ifdef EPILOGUE_SCALE_DIVISOR
                    else if (EPI == EPI_SCALE_DIV) v = v / EPILOGUE_SCALE_DIVISOR;
#endif
                    else if (EPI == EPI_HALF_PLUS) v = (v + 1.0f) / 2.0f;
                    else if (EPI == EPI_H2WORDS) { unsigned w0, w1; h2_words<true>(v, 0.f, w0, w1); v = __builtin_bit_cast(float, w0); }
                    if constexpr (C_BF16) {
                        if (row < g.M && col_ok) reinterpret_cast<unsigned short*>(C)[(long long)row * g.ldc + col] = (unsigned short)cvt_pk_bf16(v, v);
                        continue;
                    }
                    if ((!EPILOGUE_DBG_NO_STORES || v == 12345.678f) && row < g.M && col_ok) C[(long long)row * g.ldc + col] = v;
                }
            }
        }
    }
}
#undef EPILOGUE_VALUE
#undef EPILOGUE_SCALE_DIVISOR
#undef EPILOGUE_EDGE_PRELOAD
#undef EPILOGUE_DBG_NO_STORES
#undef EPILOGUE_PAIR_WORDS
