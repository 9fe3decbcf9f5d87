// Which kernel a Conv1D GEMM runs on, in ONE place.  Plain C++, no HIP header (tools/route_grid.cpp includes it); the route functions launch nothing and read only g_gemm_split3.
#pragma once
#include <stdint.h>
#include "../../include/r4d.h"

namespace r4d {

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

enum GemmEpilogue { EPI_NONE = 0, EPI_GELU = 1, EPI_RESIDUAL = 2, EPI_SCALE_DIV = 3, EPI_HALF_PLUS = 4,
                    // gemm_s3 and gemm_b1 only (training): GELU_KEEP writes gelu(v) to C and the pre-activation v to the `resid` buffer;
                    // GELU_GRAD writes v * gelu'(u) with u read from the `resid` buffer
                    EPI_GELU_KEEP = 5, EPI_GELU_GRAD = 6,
                    // gemm_h2 only: C receives the result as uint32 "h2 words" (fp16 hi | fp16 lo' << 16 of value / 4: csrc/h2.h), the
                    // operand format of attention_h2.hip
                    EPI_H2WORDS = 7,
                    // gemm_b1 only (training, r4d_set_train_act_bf16): GELU_KEEP whose gelu(v) leaves as bf16 [M, N] (RNE; ldc in bf16 elements);
                    // the pre-activation stays fp32.  Appended: route conditions compare against EPI_RESIDUAL's ordering
                    EPI_GELU_KEEP_BF16 = 8,
                    // gemm_b1 only (encoder, r4d_set_encode_attention_bf16): EPI_NONE whose result leaves as bf16 [M, N] (RNE; ldc in bf16
                    // elements): c_attn's q | k | v for attention_b1.hip, which rounds the fp32 form by the same rule while staging
                    EPI_NONE_BF16 = 9,
                    // gemm_b1 only (encoder, r4d_set_encode_act_bf16): EPI_GELU whose gelu(v) leaves as bf16 [M, N] (RNE; ldc in bf16
                    // elements) and nothing else: c_fc's f for mlp.c_proj, which rounds the fp32 form by the same rule while staging
                    EPI_GELU_BF16 = 10 };

extern int g_gemm_split3;             // Conv1D arithmetic (r4d_set_gemm_split3): 0 exact-f32 MFMA, 1 bf16x3 planes, 2 f16x2 planes (bf16x3 where a layer carries no f16 planes)

// ------------------------------------------------------------------ the kernels' shape contracts
// gemm_skinny.hip: M <= 32 rows against a k-contiguous weight [N,K], K a multiple of its 256-wide k-slice (decode step)
constexpr int SKINNY_KC = 256;
static inline bool gemm_skinny_supported(int M, int K, int N) { return M >= 1 && M <= 32 && K % SKINNY_KC == 0 && K >= SKINNY_KC && N >= 1; }
// gemm_s3.hip / gemm_h2.hip / gemm_b1.hip: K % 32 == 0, 32-bit offsets into the planes (6 / 4 / 2 bytes per weight element)
static inline bool gemm_planes_supported(int M, int K, int N, int plane_bytes) {
    return M >= 1 && K >= 32 && K % 32 == 0 && N >= 1 && (long long)N * K * plane_bytes < (1ll << 31) && (long long)M * K < (1ll << 29) &&
           128ll * N < (1ll << 29);
}
static inline bool gemm_s3_supported(int M, int K, int N) { return gemm_planes_supported(M, K, N, 6); }
static inline bool gemm_h2_supported(int M, int K, int N) { return gemm_planes_supported(M, K, N, 4); }
static inline bool gemm_b1_supported(int M, int K, int N) { return gemm_planes_supported(M, K, N, 2); }    // (so: every shape gemm_s3 takes)
// gemm_s3tn.hip: C[I,J] = X[M,I]^T . dY[M,J], whole 128 x 256 tiles
static inline bool gemm_s3tn_supported(int I, int J, int M, int lda, int ldb) {
    return I % 128 == 0 && J % 256 == 0 && M >= 32 && lda % 4 == 0 && ldb % 4 == 0 && (long long)M * lda < (1ll << 29) &&
           (long long)M * ldb < (1ll << 29);
}
// gemm_b1tn.hip: gemm_s3tn's shape contract; the 64 rows the pipeline requests past the last one stay inside 32-bit byte offsets
static inline bool gemm_b1tn_supported(int I, int J, int M, int lda, int ldb) {
    return I >= 128 && I % 128 == 0 && J >= 256 && J % 256 == 0 && M >= 32 && lda >= I && ldb >= J && lda % 4 == 0 && ldb % 4 == 0 &&
           ((long long)M + 64) * lda < (1ll << 29) && ((long long)M + 64) * ldb < (1ll << 29);
}
// The saved activations a bf16 training step may keep as bf16 [M, width] (r4d_set_train_act_bf16): a block's ln1 (layers
// >= 1: layer 0's leaves the fused embedding kernels), its ln2 and its f.  ONE rule for the layout, the forward and the backward, on
// shapes alone (the size query has no weights): both switches on (`on`), the producer's 16-byte bf16 stores (d % 256 == 0), and
// the block's two consumers take it -- gemm_b1 with a bf16 A operand forward, gemm_b1tn with a bf16 X operand for the weight gradient
enum TrainActBlock { ACT_LN1 = 0, ACT_LN2 = 1, ACT_F = 2 };
static inline bool train_act_bf16_block(int which, int layer, bool on, long long M, int d) {
    if (!on || d <= 0 || d % 256 != 0 || M < 32 || M >= (1ll << 29) || (which == ACT_LN1 && layer < 1)) return false;
    const int m = (int)M, in = which == ACT_F ? 4 * d : d, out = which == ACT_F ? d : which == ACT_LN1 ? 3 * d : 4 * d;
    return gemm_b1_supported(m, in, out) && gemm_b1tn_supported(in, out, m, in, out);
}
// gemm_f32.hip: slices of the exact-f32 weight-gradient GEMM C[M,N] = A[Kt,M]^T . B[Kt,N] over its Kt rows (an empty problem, which the launchers refuse: one)
static inline int tn_splits(int M, int N, int Kt) {
    if (M <= 0 || N <= 0 || Kt <= 0) return 1;
    const int tiles = cdiv(M, 128) * cdiv(N, 128);
    int S = cdiv(1024, tiles);                                       // ~4 workgroups per CU
    const int smax = cdiv(Kt, 256);                                  // at least 8 k-tiles per split
    if (S > smax) S = smax;
    if (S > 64) S = 64;
    return S < 1 ? 1 : S;
}

// ------------------------------------------------------------------ one Conv1D's weights
// Every form a caller may carry of ONE weight [in, out]: the reference layout `w`, its bias, the copy wT [out, in], the bf16x3 planes
// w3 [3][out][in] and w3t [3][in][out], the f16x2 planes h2, the decode step's LayerNorm-folded pair.  Null = not provided.  The LM head: no `w` (its table IS wT).
struct Conv1DW { const float *w, *b, *wT; const unsigned short *w3, *w3t, *h2; const float *wTg, *lnc; int in, out; };
enum Conv1DWhich { C_ATTN, ATTN_PROJ, C_FC, MLP_PROJ };
static inline Conv1DW conv1d_w(const r4d_gpt2_layer& L, Conv1DWhich which, int d) {
    switch (which) {
        case C_ATTN: return Conv1DW{L.c_attn_w, L.c_attn_b, L.c_attn_wT, L.c_attn_w3, L.c_attn_w3t, L.c_attn_h2, L.c_attn_wTg, L.c_attn_lnc, d, 3 * d};
        case ATTN_PROJ: return Conv1DW{L.attn_proj_w, L.attn_proj_b, L.attn_proj_wT, L.attn_proj_w3, L.attn_proj_w3t, L.attn_proj_h2, nullptr, nullptr, d, d};
        case C_FC: return Conv1DW{L.c_fc_w, L.c_fc_b, L.c_fc_wT, L.c_fc_w3, L.c_fc_w3t, L.c_fc_h2, L.c_fc_wTg, L.c_fc_lnc, d, 4 * d};
        default: return Conv1DW{L.mlp_proj_w, L.mlp_proj_b, L.mlp_proj_wT, L.mlp_proj_w3, L.mlp_proj_w3t, L.mlp_proj_h2, nullptr, nullptr, 4 * d, d};
    }
}
// The LM head's rows [c0, c0 + rows) of wte_pad (include/r4d.h: r4d_lm_head; the whole head: c0 = 0, rows = ldV).  w3 / w3t are
// laid chunk by chunk at 3 * c0 * d, h2 row-major over the vocabulary rows at 2 * c0 * d
static inline Conv1DW conv1d_w(const r4d_lm_head& h, int d, int c0, int rows) {
    const size_t o = (size_t)c0 * d;
    return Conv1DW{nullptr, nullptr, h.wte_pad + o, h.w3 ? h.w3 + 3 * o : nullptr, h.w3t ? h.w3t + 3 * o : nullptr,
                   h.h2 ? h.h2 + 2 * o : nullptr, nullptr, nullptr, d, rows};
}
// The cached decode step's view: no planes -- it keeps its weight streams, and the exact-f32 kernels beyond 32 rows
static inline Conv1DW conv1d_w_decode(Conv1DW W) { W.w3 = nullptr; W.h2 = nullptr; return W; }

// ------------------------------------------------------------------ the routes
enum GemmRoute { ROUTE_SKINNY, ROUTE_H2, ROUTE_S3, ROUTE_B1, ROUTE_F32_KCOPY, ROUTE_F32_REF,     // forward
                 ROUTE_DGRAD_B1, ROUTE_DGRAD_S3, ROUTE_DGRAD_F32,                              // dx = dy . W^T / head
                 ROUTE_WGRAD_B1TN, ROUTE_WGRAD_S3TN, ROUTE_WGRAD_F32TN,                        // dW = x^T . dy
                 ROUTE_COUNT };
static inline const char* gemm_route_name(int route) {
    static const char* const names[ROUTE_COUNT] = {"skinny", "h2", "s3", "b1", "f32_kcopy", "f32_ref", "dgrad_b1", "dgrad_s3", "dgrad_f32",
                                                   "wgrad_b1tn", "wgrad_s3tn", "wgrad_f32tn"};
    return route >= 0 && route < ROUTE_COUNT ? names[route] : "unknown";
}
// Who asks for plain bf16: the encoder calls (r4d_set_encode_bf16) allow it up to EPI_RESIDUAL only, the training forward any
// epilogue; the LM head's logits (r4d_set_train_head_bf16) take the training forward's route and count under their own branch
enum Bf16Use { BF16_OFF = 0, BF16_ENCODE = 1, BF16_TRAIN = 2, BF16_TRAIN_HEAD = 3 };
// The `bf16` argument of the two gradient routes: the layers' switch (r4d_set_train_bf16) or the LM head's (r4d_set_train_head_bf16)
enum TrainBf16 { TRAIN_BF16_OFF = 0, TRAIN_BF16_LAYERS = 1, TRAIN_BF16_HEAD = 2 };

// y = epilogue(x[M, in] . W + b).  `skinny`: the caller has the decode step's split-K scratch.  In order:
static inline GemmRoute conv1d_route(const Conv1DW& W, int M, int epilogue, bool skinny, int bf16) {
    const int K = W.in, N = W.out;
    if (bf16 && (bf16 >= BF16_TRAIN || epilogue <= EPI_RESIDUAL) && W.w3 && gemm_b1_supported(M, K, N)) return ROUTE_B1;   // plane 0 of w3, one bf16 MFMA per k-step
    if (skinny && W.wT && gemm_skinny_supported(M, K, N)) return ROUTE_SKINNY;          // decode step: a weight stream, not a tiled GEMM
    // f16x2 planes present and selected: fp16 matrix cores, three products per fp32 product (gemm_h2.hip), for the epilogues it has.
    // NOT gated on M, like the bf16x3 route: a row's result must not depend on how many other rows share the call
    if (W.h2 && g_gemm_split3 == 2 && (epilogue <= EPI_RESIDUAL || epilogue == EPI_GELU_KEEP || epilogue == EPI_H2WORDS) && gemm_h2_supported(M, K, N))
        return ROUTE_H2;
    if (W.w3 && g_gemm_split3 && gemm_s3_supported(M, K, N)) return ROUTE_S3;            // bf16 matrix cores at fp32 accuracy
    return W.wT ? ROUTE_F32_KCOPY : ROUTE_F32_REF;                                      // exact f32: the [out, in] copy (fast kernel), else the reference layout
}
// The training forward leaves gelu(v) AND v from c_fc's ONE launch (EPI_GELU_KEEP) where this holds: plain bf16, bf16x3, and f16x2
// only where the layer carries the bf16x3 planes too and their contract holds (the earlier precedence, kept: DESIGN.md 4.4)
static inline bool conv1d_fuses_gelu_keep(const Conv1DW& W, int M, int bf16) {
    const GemmRoute r = conv1d_route(W, M, EPI_GELU_KEEP, false, bf16);
    return r == ROUTE_B1 || r == ROUTE_S3 || (r == ROUTE_H2 && W.w3 && gemm_s3_supported(M, W.in, W.out));
}
// The activations a bf16 encoder forward may keep as bf16 [M, width] between producer and consumer (r4d_set_encode_act_bf16; DESIGN.md
// 7 item 13): a block's ln1 (every layer: the fused embedding kernel has a bf16 output), its ln2 and its f -- train_act_bf16_block's
// three (above), decided per buffer.  ONE rule on shapes and plane presence: both switches on (`on`), the producers' 16-byte bf16
// stores (d % 256 == 0), and every GEMM that touches the buffer on the plain-bf16 kernel: ln1's consumer c_attn, ln2's consumer
// c_fc, f's producer c_fc and its consumer mlp.c_proj.  Otherwise that buffer stays fp32 and the launches are those of the switch off
static inline bool encode_act_bf16_block(int which, bool on, const Conv1DW& Wqkv, const Conv1DW& Wfc, const Conv1DW& Wp, int M, int d) {
    if (!on || d <= 0 || d % 256 != 0) return false;
    const bool fc = conv1d_route(Wfc, M, EPI_GELU, false, BF16_ENCODE) == ROUTE_B1;
    switch (which) {
        case ACT_LN1: return conv1d_route(Wqkv, M, EPI_NONE, false, BF16_ENCODE) == ROUTE_B1;
        case ACT_LN2: return fc;
        case ACT_F: return fc && conv1d_route(Wp, M, EPI_RESIDUAL, false, BF16_ENCODE) == ROUTE_B1;
        default: return false;
    }
}
// dx[M, in] = dy[M, out] . W^T.  A Conv1D reads w [in, out] as the k-contiguous operand (b_trans = 1); the LM head (no `w`) reads
// its table [out, in] as a row-major one (b_trans = 0) and never takes the LAYERS' plain bf16: only its own switch
// (bf16 == TRAIN_BF16_HEAD) sends it to plane 0 of its w3t.  The data gradients stay on bf16x3 in EVERY
// split mode: their A operand is a gradient, which needs fp32's exponent range
static inline GemmRoute dgrad_route(const Conv1DW& W, int M, int bf16) {
    if (bf16 && (W.w || bf16 == TRAIN_BF16_HEAD) && W.w3t && gemm_b1_supported(M, W.out, W.in)) return ROUTE_DGRAD_B1;
    if (W.w3t && g_gemm_split3 && gemm_s3_supported(M, W.out, W.in)) return ROUTE_DGRAD_S3;
    return ROUTE_DGRAD_F32;
}
// dW[I, J] = x[M, I]^T . dy[M, J].  S == 1 (tn_splits): tiny problems stay on the exact-f32 kernel in every mode
static inline GemmRoute wgrad_route(int I, int J, int M, int lda, int ldb, int bf16) {
    if (bf16 && gemm_b1tn_supported(I, J, M, lda, ldb)) return ROUTE_WGRAD_B1TN;
    if (g_gemm_split3 && tn_splits(I, J, M) > 1 && gemm_s3tn_supported(I, J, M, lda, ldb)) return ROUTE_WGRAD_S3TN;
    return ROUTE_WGRAD_F32TN;
}

// The query behind r4d_conv1d_route (include/r4d.h): kind 0 encode, 1 decode, 2 train forward, 3 dgrad Conv1D, 4 dgrad head,
// 5 wgrad (M token rows, dW [K, N]); `have` bits: wT, w3, w3t, h2, skinny scratch.  -1 for an unknown kind or an empty shape.
// bf16 == 2 (TRAIN_BF16_HEAD) asks as the LM head under r4d_set_train_head_bf16: kind 2 its logits (N = a vocabulary chunk), kind 4
// its dh (N = the chunk), kind 5 its dwte (K = the chunk, N = d)
static inline int conv1d_route_query(int kind, int M, int K, int N, int epilogue, unsigned have, int bf16) {
    if (M <= 0 || K <= 0 || N <= 0) return -1;
    static const float f = 0.f;
    static const unsigned short u = 0;
    const Conv1DW W{kind == 4 ? nullptr : &f, nullptr, (have & 1u) || kind == 4 ? &f : nullptr, (have & 2u) ? &u : nullptr,
                    (have & 4u) ? &u : nullptr, (have & 8u) ? &u : nullptr, nullptr, nullptr, K, N};
    switch (kind) {
        case 0: return conv1d_route(W, M, epilogue, false, bf16 ? BF16_ENCODE : BF16_OFF);
        case 1: return conv1d_route(conv1d_w_decode(W), M, epilogue, (have & 16u) != 0, BF16_OFF);
        case 2: return conv1d_route(W, M, epilogue, false, bf16 == TRAIN_BF16_HEAD ? BF16_TRAIN_HEAD : bf16 ? BF16_TRAIN : BF16_OFF);
        case 3: case 4: return dgrad_route(W, M, bf16);
        case 5: return wgrad_route(K, N, M, K, N, bf16);
        default: return -1;
    }
}

}  // namespace r4d
