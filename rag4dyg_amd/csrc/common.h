// Shared helpers for the gfx950 kernels behind include/r4d.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/r4d.h"
#include "conv1d_route.h"      // GemmEpilogue, the kernels' shape contracts, Conv1DW, the routes (host-only text)

namespace r4d {

void set_error(const char* fmt, ...);
// 1 when the translation unit was built with its kernel-ablation macro set (tools/kc_ablate.sh): r4d_build_flags()
int dbgflag_kc(); int dbgflag_att(); int dbgflag_sk(); int dbgflag_jac(); int dbgflag_scan(); int dbgflag_s3(); int dbgflag_h2();

#define R4D_REQUIRE(cond, ...)                     \
    do {                                           \
        if (!(cond)) {                             \
            r4d::set_error(__VA_ARGS__);           \
            return R4D_ERR_INVALID;                \
        }                                          \
    } while (0)

#define R4D_HIP(call)                                                                  \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                        \
            r4d::set_error("%s: %s", #call, hipGetErrorString(e_));                    \
            return R4D_ERR_HIP;                                                        \
        }                                                                              \
    } while (0)

#define R4D_CHECK_LAUNCH(name)                                                         \
    do {                                                                               \
        hipError_t e_ = hipGetLastError();                                             \
        if (e_ != hipSuccess) {                                                        \
            r4d::set_error("%s: launch failed: %s", name, hipGetErrorString(e_));      \
            return R4D_ERR_HIP;                                                        \
        }                                                                              \
    } while (0)

// ------------------------------------------------------------------ launch profiler (profile.hip)
enum ProfClass {
    PK_GEMM_128x128_NN = 0, PK_GEMM_128x128_NT, PK_GEMM_128x64_NN, PK_GEMM_128x64_NT, PK_GEMM_64x64_NN,
    PK_GEMM_64x64_NT, PK_GEMM_KC_128x128x32, PK_GEMM_KC_128x128x16, PK_GEMM_KC_128x64x16, PK_GEMM_KC_64x64x32, PK_GEMM_S3_128x256, PK_GEMM_S3_128x128, PK_GEMM_S3TN, PK_GEMM_H2_128x256, PK_GEMM_H2_128x128, PK_GEMM_SKINNY, PK_GEMM_SKINNY_EPI,
    PK_EMBED_LN, PK_LAYERNORM, PK_SOFTMAX, PK_DECODE_ATTN, PK_GREEDY_ADVANCE,
    PK_ATTN_FUSED, PK_LNF_MEANPOOL, PK_MEANPOOL_REDUCE, PK_NORMALIZE, PK_POOL_SCAN, PK_TOPK, PK_MERGE_TOPK, PK_RANK_COUNT, PK_JACCARD, PK_JACCARD_PREP, PK_LM_CE,
    PK_SPLICE_EMBED, PK_WEIGHTED_BAG, PK_EMB_SCATTER, PK_GEMM_B1, PK_GEMM_B1TN, PK_GEMM_H2_ROWMAP, PK_PAD_CLASSIFY, PK_PAD_FILL, PK_GEMM_B1H_NT, PK_GEMM_B1H_NN,
    PK_ATTN_TRAIN_FUSED_FWD, PK_ATTN_TRAIN_FUSED_ROWSUM, PK_ATTN_TRAIN_FUSED_DKV, PK_ATTN_TRAIN_FUSED_DQ, PK_ATTN_B1, PK_SAMPLE_ADVANCE, PK_BEAM_ROWS, PK_BEAM_ADVANCE, PK_KV_REORDER, PK_COUNT
};
extern bool g_prof_on;
void prof_begin_impl(int cls, double work, hipStream_t s);
void prof_end_impl(hipStream_t s);
struct ProfScope {
    hipStream_t s; bool on;
    ProfScope(int cls, double work, hipStream_t st) : s(st), on(g_prof_on) { if (on) prof_begin_impl(cls, work, s); }
    ~ProfScope() { if (on) prof_end_impl(s); }
};

// ------------------------------------------------------------------ dispatcher-branch coverage (profile.hip)
// Every host-side decision that selects a kernel VARIANT (tile shape, template instantiation, split-K form, fallback) counts
// its launches under a name; r4d_dispatch_* enumerates the table so that a test can assert that each branch was exercised
// (tests/test_gpu_ops.py::test_every_dispatcher_branch_is_exercised -- a shape list keyed by config names missed the
// d = 256 decode path once: commit 2e9f5d4).  Names that start with "tuning:" are reachable through environment switches only.
#define R4D_BRANCH_LIST(X)                                                                                              \
    X(KC_128x128x16, "gemm_kc:128x128x16") X(KC_128x64x16, "gemm_kc:128x64x16") X(KC_64x64x32, "gemm_kc:64x64x32")       \
    X(KC_128x128x32, "tuning:gemm_kc:128x128x32") X(KC_ROWSPLIT, "gemm_kc:row-split (two launches)")                      \
    X(S3_128x256, "gemm_s3:128x256x32") X(S3_PERSISTENT, "gemm_s3:128x256x32 persistent (pipeline across tiles)") X(S3_128x128, "gemm_s3:128x128x32") X(S3_F32B, "gemm_s3:both operands split on the fly (scoring GEMM)") X(S3_TN, "gemm_s3tn:128x256x32 (weight gradients, transposing LDS reads)")      \
    X(H2_128x256, "gemm_h2:128x256x32 (f16x2)") X(H2_128x128, "gemm_h2:128x128x32 (f16x2)") X(H2P_128x256, "gemm_h2p:128x256x32 (f16x2, A as lines, LDS-DMA)") X(H2P_128x128, "gemm_h2p:128x128x32 (f16x2, A as lines, LDS-DMA)") X(H2P_ROWMAP, "gemm_h2p:row-block map (layer 0 c_attn without the repeated pad-row blocks)") \
    X(F32_128x128, "gemm_f32:128x128") X(F32_128x64, "gemm_f32:128x64") X(F32_64x64, "gemm_f32:64x64")                   \
    X(F32_NT, "gemm_f32:B as [N,K]") X(F32_NN, "gemm_f32:B as [K,N]") X(TN_SPLITK, "gemm_tn:split-K") X(TN_SINGLE, "gemm_tn:one slice") \
    X(SK16_NG2, "skinny16:ng2") X(SK16_NG3, "skinny16:ng3") X(SK16_NG2_LN, "skinny16:ng2+layernorm") X(SK16_LN_FOLDED, "skinny16:LayerNorm pre-folded into the weight") X(SK16_NG3_LN, "skinny16:ng3+layernorm") \
    X(SK16_SPLITK, "skinny16:split-K last-arriver") X(SK8_NG2, "skinny8:ng2") X(SK8_NG3, "skinny8:ng3")                    \
    X(SK8_LN, "tuning:skinny8:+layernorm") X(SK8_SPLITK, "skinny8:split-K + epilogue launch") X(SK_PLAIN, "skinny:plain + epilogue launch") \
    X(ATT_KS32, "attention:key-split hd32") X(ATT_KS64, "attention:key-split hd64") X(ATT_CS96, "attention:column-split hd96") \
    X(ATT_CS128, "attention:column-split hd128") X(ATT_CS256, "attention:column-split hd256") X(ATT_H2_KS32, "attention:f16x2 key-split hd32") X(ATT_H2_KS64, "attention:f16x2 key-split hd64") X(ATT_H2_KS96, "attention:f16x2 key-split hd96") X(ATT_H2_128, "attention:f16x2 hd128") X(ATT_H2_256, "attention:f16x2 hd256") X(ATT_H2_KS32_KBLK, "attention:f16x2 key-split hd32, key-blocked K") X(ATT_H2_KS64_KBLK, "attention:f16x2 key-split hd64, key-blocked K") X(ATT_H2_KS96_KBLK, "attention:f16x2 key-split hd96, key-blocked K") X(ATT_H2_128_KBLK, "attention:f16x2 hd128, key-blocked K") X(ATT_H2_256_KBLK, "attention:f16x2 hd256, key-blocked K")                              \
    X(ATT_KS_FORCED, "tuning:attention:key-split at hd96/128/256") X(ATT_3LAUNCH, "attention:three-launch GEMM form")      \
    X(SCAN_1_1, "scan:d32") X(SCAN_2_1, "scan:d64") X(SCAN_4_1, "scan:d128") X(SCAN_4_2, "scan:d256") X(SCAN_4_3, "scan:d384") \
    X(SCAN_8_2, "scan:d512") X(SCAN_4_4, "tuning:scan:d512 4-way") X(SCAN_8_3, "scan:d768") X(SCAN_8_4, "scan:d1024")       \
    X(SCAN_SHORT, "scan:short shard (even rows, two tiles in flight)") X(SCAN_DMA, "scan:short shard, LDS-DMA staged") X(SCAN_RING, "scan:long shard, LDS-DMA ring") X(SCAN_GEMM, "scan:tiled GEMM (Q > 64 or other d)") X(SCAN_TILED, "scan:128x256 tiles in the scan kernels' arithmetic (Q >= 64)") X(SCAN_BF16X3, "scan:bf16x3 operands") X(SCAN_F32, "scan:exact-f32 operands")  \
    X(TOPK_ONE_WG, "topk:one workgroup per row") X(TOPK_TICKET, "topk:cross-workgroup ticket merge")                      \
    X(TOPK_MULTI, "topk:second launch over candidates") X(TOPK_F64, "topk:f64 rows")                                      \
    X(TOPKL_ONE, "tuning:topk_large:one level") X(TOPKL_MULTI, "tuning:topk_large:several levels") X(TOPKL_MERGE, "tuning:topk_large:merge route") \
    X(EMBED_LN4, "embed+layernorm:16-byte lanes") X(EMBED_GENERIC, "embed+layernorm:generic") X(LN4_2, "layernorm:ln4<2>") X(LN4_4, "layernorm:ln4<4>") X(LN4_8, "layernorm:ln4<8>") X(LN_GENERIC, "layernorm:generic") \
    X(LNF_8, "lnf_meanpool:<8>") X(LNF_16, "lnf_meanpool:<16>") X(LNF_32, "lnf_meanpool:<32>")                             \
    X(DEC_ATT_32, "decode_attention:<32>") X(DEC_ATT_64, "decode_attention:<64>")                                         \
    X(JAC_LDS, "jaccard:LDS table") X(JAC_MERGE, "jaccard:merge walk (vocab too large for LDS)")                          \
    X(JAC_PREP_DENSE_LDS, "jaccard_prep:dense tokens, LDS histogram") X(JAC_PREP_DENSE_GLOBAL, "jaccard_prep:dense tokens, global histogram") X(JAC_PREP_ORDER, "jaccard_prep:rows longest first") \
    X(ARGSORT_ONE, "argsort:one chunk") X(ARGSORT_MULTI, "argsort:chunk sort + rank scatter")                              \
    X(B1_128x256, "tuning:encode_bf16:128x256x32") X(B1_128x128, "tuning:encode_bf16:128x128x32")                           \
    X(TB_FWD, "tuning:train_bf16:fwd") X(TB_DGRAD, "tuning:train_bf16:dgrad") X(TB_WGRAD, "tuning:train_bf16:wgrad") X(TB_WGRAD_FALLBACK, "tuning:train_bf16:wgrad_fallback") \
    X(TBA_NT, "tuning:train_bf16_attn:nt") X(TBA_NN, "tuning:train_bf16_attn:nn") \
    X(TBH_LOGITS, "tuning:train_head_bf16:logits") X(TBH_DGRAD, "tuning:train_head_bf16:dgrad") X(TBH_WGRAD, "tuning:train_head_bf16:wgrad") X(TBH_WGRAD_FALLBACK, "tuning:train_head_bf16:wgrad_fallback") \
    X(TAB_FWD, "tuning:train_act_bf16:fwd") X(TAB_WGRAD, "tuning:train_act_bf16:wgrad") X(TAB_LN, "tuning:train_act_bf16:ln") X(TAB_GELU, "tuning:train_act_bf16:gelu") \
    X(TAF_FWD, "tuning:train_attn_fused:fwd") X(TAF_ROWSUM, "tuning:train_attn_fused:rowsum") X(TAF_DKV, "tuning:train_attn_fused:dkv") X(TAF_DQ, "tuning:train_attn_fused:dq") \
    X(EBA_BF16, "tuning:encode_bf16_attn:bf16 qkv") X(EBA_F32, "tuning:encode_bf16_attn:fp32 qkv, rounded while staged") X(EBA_FALLBACK, "tuning:encode_bf16_attn:fallback to the exact-f32 attention") \
    X(EAB_LN1, "tuning:encode_act_bf16:ln1") X(EAB_LN2, "tuning:encode_act_bf16:ln2") X(EAB_F, "tuning:encode_act_bf16:f") X(EAB_KEPT_F32, "tuning:encode_act_bf16:kept fp32") \
    X(SAMPLE_LDS, "tuning:sample:keyed row in LDS") X(SAMPLE_GLOBAL, "tuning:sample:row re-read from memory") \
    X(BEAM_LDS, "tuning:beam:keyed row in LDS") X(BEAM_GLOBAL, "tuning:beam:row re-read from memory")
enum DispatchBranch {
#define X(id, name) BR_##id,
    R4D_BRANCH_LIST(X)
#undef X
    BR_COUNT
};
extern unsigned long long g_branch_hits[BR_COUNT];
#define R4D_BRANCH(id) (++r4d::g_branch_hits[r4d::BR_##id])

// range guard (include/r4d.h: r4d_set_range_flag)
extern unsigned* g_range_flag;         // bits: R4D_RANGE_NONFINITE_HIDDEN, R4D_RANGE_BAD_NORM, R4D_RANGE_BAD_LABEL

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ------------------------------------------------------------------ fp32 MFMA GEMM (gemm_f32.hip)
enum GemmCausal { CAUSAL_NONE = 0, CAUSAL_QK = 1, CAUSAL_PV = 2 };

struct GemmArgs {
    const float* A; const float* B; float* C;
    const float* bias;      // [N] or null
    const float* resid;     // [M,N] (ldr) or null
    int M, N, K;            // K = full contraction length (CAUSAL_PV trims it per row tile)
    int lda, ldb, ldc, ldr;
    int b_trans;            // 0: B is [K,N] (ldb >= N)   1: B is [N,K] (ldb >= K)
    int b_rows;             // valid rows of B (guards loads): K for NN, N for NT
    int a_cols;             // valid columns of A (guards loads); 0 -> K
    int nbatch, nb1;        // batch z = z0 * nb1 + z1
    long long sA0, sA1, sB0, sB1, sC0, sC1;   // element strides per batch index
    int epilogue; float scale_div;
    int causal;
};
// C[M,N] = epilogue(A[M,K] . B + bias) on dense rows, one batch; B is [N,K] (b_trans) or [K,N]
static inline GemmArgs gemm_args(const float* A, const float* B, int b_trans, const float* bias, const float* resid, int M, int K, int N,
                                 int epilogue, float* C) {
    GemmArgs g{};
    g.A = A; g.B = B; g.C = C; g.bias = bias; g.resid = resid;
    g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = b_trans ? K : N; g.ldc = N; g.ldr = N;
    g.b_trans = b_trans; g.b_rows = b_trans ? N : K; g.nbatch = 1; g.nb1 = 1;
    g.epilogue = epilogue; g.scale_div = 1.f; g.causal = CAUSAL_NONE;
    return g;
}
int launch_gemm_f32(const GemmArgs& g, hipStream_t stream);
int launch_gemm_f32_kc(const GemmArgs& g, hipStream_t stream);      // B given as [N,K]: k-contiguous kernel
// C[M,N] = A[Kt,M]^T . B[Kt,N] (weight gradients), split-K partials in scratch (gemm_tn_scratch_floats floats)
size_t gemm_tn_scratch_floats(int M, int N, int Kt);
// (the exact-f32 kernel only: weight_grad below chooses between it and the two matrix-core forms)
int launch_gemm_f32_tn(const float* A, const float* B, float* C, int M, int N, int Kt, int lda, int ldb, float* scratch, hipStream_t stream);
// gemm_skinny.hip: M <= 32 rows against a k-contiguous weight [N,K], K % 256 == 0 (decode step); split-K partials in scratch
size_t gemm_skinny_scratch_floats(int K, int N);
bool gemm_skinny_fuses_ln(int M, int K, int N);       // y = epilogue(LayerNorm(x) . wT^T + bias) in one launch
// `counters_zeroed`: the caller cleared the split-K ticket counters (gemm_skinny_counters) on this stream since the last
// aborted launch (a completed launch leaves them at zero); otherwise the launcher clears them itself when K is split
void* gemm_skinny_counters(float* scratch, size_t* bytes);
int launch_gemm_skinny(const float* x, const float* wT, const float* bias, const float* resid, int M, int K, int N,
                       int epilogue, float* y, float* scratch, hipStream_t s, const float* ln_w = nullptr,
                       const float* ln_b = nullptr, float ln_eps = 0.f, bool counters_zeroed = false, const float* ln_fold = nullptr);
int launch_fold_layernorm(const float* wT, const float* g, const float* beta, int N, int K, float* wTg, float* lnc, hipStream_t s);

// gemm_s3.hip: C = epilogue(A . W^T + bias) on the bf16 matrix cores at fp32 accuracy (A fp32, split on the fly into three
// bf16 terms; W given as three pre-split bf16 planes [3][N][K]); K % 32 == 0
struct S3Args {
    const float* A; const unsigned short* planes; float* C;
    const float* bias; const float* resid;
    int M, N, K, lda, ldc, ldr, epilogue;
    int a_bf16;                       // gemm_b1 only: A is bf16 [M, K] (lda in bf16 elements) behind the float pointer (r4d_set_train_act_bf16)
    unsigned* kblk; int kb_hd;        // gemm_h2p, EPI_H2WORDS, N = 3 d: columns [d, 2d) go to the key-blocked K image instead (kb_hd = head_dim; 0 = off)
};
// y[M,N] = epilogue(x[M,K] . planes + bias) on dense rows (lda = K, ldc = ldr = N): the arguments of every planes kernel
static inline S3Args s3_args(const float* x, const unsigned short* planes, const float* bias, const float* resid, int M, int K, int N,
                             int epilogue, float* y) {
    S3Args a{};
    a.A = x; a.planes = planes; a.C = y; a.bias = bias; a.resid = resid;
    a.M = M; a.N = N; a.K = K; a.lda = K; a.ldc = N; a.ldr = N; a.epilogue = epilogue;
    return a;
}
int launch_gemm_s3(const S3Args& a, hipStream_t stream);
bool gemm_s3_f32b_supported(int M, int K, int N);
int launch_gemm_s3_f32b(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldc, int epilogue, hipStream_t stream);
int launch_gemm_s3_scan_order(const float* q_hat, const float* pool_hat, float* scores, int Q, int N, int d, int ng, hipStream_t stream);
// w element (n, k) at w[k * ld_k + n * ld_n] -> planes [3][N][K] bf16 (hi, mid, lo)
// gemm_h2.hip: the same contract on the fp16 matrix cores, two fp16 terms per operand and THREE products (planes [2][N][K])
int launch_gemm_h2(const S3Args& a, hipStream_t stream);
int launch_split2_planes(const float* w, int N, int K, long long ld_k, long long ld_n, unsigned short* planes, hipStream_t s);
// gemm_h2p.hip: the same arithmetic with the A operand already split by its producer into f16x2 lines [M][K/32][2][32] fp16 (both
// tiles staged by LDS-DMA); out_lines: the GELU epilogue writes lines [M][N/32][2][32] fp16 into a.C.  a.A is ignored.
extern int g_gemm_h2p;
bool gemm_h2p_supported(int M, int K, int N);
int launch_gemm_h2p(const S3Args& a, const unsigned short* a_lines, bool out_lines, hipStream_t stream);
int launch_split2_lines(const float* x, long long rows, int K, unsigned short* lines, hipStream_t s);
// gemm_b1.hip: C = epilogue(RN_bf16(A) . RN_bf16(W)^T + bias), one bf16 MFMA per k-step (NOT fp32-accurate); a.planes = ONE bf16
// plane [N][K] (plane 0 of the bf16x3 planes); the bf16x3 kernel's shape contract; epilogues none / GELU / residual
// (training, r4d_set_train_bf16: also GELU_KEEP and GELU_GRAD).  a.a_bf16 (r4d_set_train_act_bf16): A is already bf16 in memory -- the
// same operand bits, one 16-byte load per item and no rounding; epilogues none / residual / GELU_KEEP / GELU_KEEP_BF16 (C as bf16)
// and, for the encoder (r4d_set_encode_act_bf16), GELU / GELU_BF16 / NONE_BF16
int launch_gemm_b1(const S3Args& a, hipStream_t stream);
// gemm_b1tn.hip: out[I,J] (one slice) or partials [S][I][J] <- RN_bf16(X[M,I])^T . RN_bf16(dY[M,J]) over S slices of the M rows,
// db_out (nullable) [J] or [S][J] <- column sums of the unrounded dY; gemm_s3tn's shape contract
// x_bf16: X is bf16 [M, lda] behind the pointer (lda in bf16 elements, a multiple of 8): the same operand bits, no rounding
int launch_gemm_b1tn(const float* X, const float* dY, float* out, float* db_out, int I, int J, int M, int lda, int ldb, int S,
                     hipStream_t stream, bool x_bf16 = false);
// gemm_b1h.hip: the per-head attention products of the training steps on plain bf16 operands (r4d_set_train_attention_bf16; NOT
// fp32-accurate): the GemmArgs of launch_gemm_f32's batched form -- both operand forms, epilogues none / scale-div, the three causal
// flags, no bias, no residual
int launch_gemm_b1h(const GemmArgs& g, hipStream_t stream);
// gemm_s3tn.hip: partials [slices][I][J] <- X[M,I]^T . dY[M,J] on the bf16 matrix cores at fp32 accuracy, db_partials (nullable)
// [slices][J] <- column sums of dY; one slice is a partial too
int launch_gemm_s3tn(const float* X, const float* dY, float* out, float* db_partials, int I, int J, int M, int lda, int ldb, int S,
                     hipStream_t stream);
// Slices both kernels WANT over the M token rows: enough 128 x 256 workgroups for two rounds of the 256 CUs (gemm_s3tn at one
// workgroup per CU; gemm_b1tn at two per CU: one round -- the same 512), at least 8 k-tiles of 32 rows each, never more than
// `max_slices`: the room of the caller's scratch.  One rule because both walk the same tiles over the same rows; every caller's
// `max_slices` is at most 64 (tn_splits, or the b1tn callers' own cap).
static inline int gemm_tn_slices(int I, int J, int M, int max_slices) {
    const int tiles = (I / 128) * (J / 256);
    int S = cdiv(512, tiles);
    const int smax = cdiv(M, 256);
    if (S > smax) S = smax;
    if (S > max_slices) S = max_slices;
    return S < 1 ? 1 : S;
}
// slices that HOLD rows when M token rows are cut into S slices of whole 32-row steps
static inline int tn_row_slices(int M, int S) { return cdiv(M, cdiv(cdiv(M, S), 32) * 32); }
// gemm_f32.hip: C[4 n4] = part[0] + part[1] + ... + part[S-1] (slices of 4 n4 floats), added in that order
int launch_splitk_reduce(const float* part, long long n4, int S, float* C, hipStream_t stream);
extern int g_encode_bf16;             // r4d_set_encode_bf16: the encoder calls' Conv1D GEMMs on gemm_b1 wherever a layer carries *_w3
// y[M, W.out] = epilogue(x[M, W.in] . W + W.b) on the kernel conv1d_route names (encoder.hip): the encoder calls, the decode step,
// the training forward and the LM head.  `resid`: the second buffer of the residual / GELU_KEEP epilogues
struct Conv1DOpts {
    float* skinny_scratch = nullptr;   // decode step: the split-K scratch of the weight-stream kernel (gemm_skinny_scratch_floats)
    bool counters_zeroed = false;      // ... whose ticket counters the caller cleared on this stream
    int bf16 = BF16_OFF;               // Bf16Use: who asks for plain bf16
    bool x_bf16 = false;               // training, r4d_set_train_act_bf16: x is bf16 [M, W.in] behind the pointer; gemm_b1 only (else refused)
};
int conv1d(const Conv1DW& W, const float* x, const float* resid, int M, int epilogue, float* y, hipStream_t s, const Conv1DOpts& opts = {});
int launch_split3_planes(const float* w, int N, int K, long long ld_k, long long ld_n, unsigned short* planes, hipStream_t s);

// ------------------------------------------------------------------ train_ops.hip
struct DropKey { unsigned seed_lo, seed_hi, step_lo, step_hi; };      // Philox key (seed) and counter words 2-3 (step)
// out = (resid ? resid : 0) + dropout_p(x): element i uses counter (base + i) / 4 of `site`; out may alias x / resid
int launch_dropout(const float* x, const float* resid, long long n, float* out, float p, DropKey key, unsigned site,
                   unsigned long long base, hipStream_t s);
// 64-bit fixed-point token-gradient tables (train_ops.hip, embedding backward): S with |g| 2^S M < 2^62 for every |g| <= max,
// M = 2^lg_rows >= the contributions that can meet in one element
constexpr int EMB_SUM_BITS = 62;
__device__ __forceinline__ int emb_scale_exp(unsigned max_bits, int lg_rows) {
    const int e = (int)((max_bits >> 23) & 255u) - 126;                                  // max < 2^e (exponent field 0: a subnormal)
    return EMB_SUM_BITS - lg_rows - e;
}
static inline int emb_lg_rows(long long table_rows) {
    int lg = 0;
    while ((1LL << lg) < table_rows) ++lg;
    return lg;
}
int launch_embedding_fix_to_f32(const unsigned long long* acc, long long n, long long table_rows, float* out, hipStream_t s);

// attention_train_fused.hip: Attention._attn of one batch [B, T] and its backward on the "+attn" arithmetic with no [T, T] block in
// memory (r4d_set_train_attention_fused).  att [B, T, d] merged heads (the backward does not read it), lse / Dscr [B * H, T]; the dropout mask of element (bh, i, j)
// is launch_dropout's at pbase + (bh T + i) ceil128(T) + j.  Shapes outside attn_train_fused_supported are refused before any launch.
bool attn_train_fused_supported(int B, int T, int H, int d);
size_t attn_train_fused_bwd_scratch_floats(int B, int T, int H);
int launch_attn_train_fused_fwd(const float* qkv, int B, int T, int H, int d, float* att, float* lse, float attn_p, DropKey key,
                                unsigned site, unsigned long long pbase, hipStream_t s);
int launch_attn_train_fused_bwd(const float* qkv, const float* att, const float* lse, const float* dao, int B, int T, int H, int d,
                                float* dqkv, float* Dscr, float attn_p, DropKey key, unsigned site, unsigned long long pbase, hipStream_t s);

// ------------------------------------------------------------------ train.hip (the training forward / backward, shared with lm_head.hip)
// The process-wide training switches as a value (train.hip: kTrainModes, one row per switch -- its r4d_set_train_* / r4d_get_train_*
// pair, its setter's conventions and whether the backward guards it).  Every extern "C" entry point reads them ONCE, through
// train_modes(), and hands the value down as an argument; nothing below an entry point looks at the global.
// head_bf16 is the LM head's alone (lm_head.hip): the transformer's forward and backward do not look at it.
// act_bf16 acts only while bf16 is on: which saved activations are bf16 in memory (conv1d_route.h: train_act_bf16_block).
// attn_fused needs attn_bf16 (the entries refuse it alone): attention by the fused kernels, no P-shaped block.
struct TrainModes { int attention, activations, bf16, attn_bf16, head_bf16, act_bf16, attn_fused; };
TrainModes train_modes();
static inline bool train_modes_ok(const TrainModes& md) { return !md.attn_fused || md.attn_bf16; }   // else: size queries 0, entries refuse
size_t gpt2_train_workspace_floats(const r4d_gpt2_config* cfg, int n_groups, const int32_t* Bs, const int32_t* Ts, TrainModes md);
// output: EITHER out_meanpool_d [sum B, d] OR out_hidden_d [rows, d] (the ln_f output); the backward takes the matching gradient
// `sp` (nullable, one batch only): a SPLICED input (RAG generator): ids_d[0] holds -100 at the positions 2 .. 2 + r - 1, whose
// embedding rows are sp->fused [B, r, d] instead of wte rows (rag_train.hip: launch_splice_embed_ln)
struct SpliceIn { const float* fused; int r; };
int gpt2_train_forward(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, int n_groups, const int64_t* const* ids_d,
                       const int32_t* Bs, const int32_t* Ts, float* out_meanpool_d, float* out_hidden_d,
                       const r4d_train_dropout* dropout, void* workspace_d, size_t workspace_bytes, TrainModes md, hipStream_t s,
                       const SpliceIn* sp = nullptr);
// `gr` == nullptr: FROZEN transformer -- no parameter gradient at all (no weight GEMM, no LayerNorm gain / shift sums, no
// embedding scatter), only the data gradients down to the embeddings; `d_fused` must then be given.  `d_fused` (with `sp`):
// [B, r, d] <- the gradient of the spliced rows (behind the embedding dropout's mask)
int gpt2_train_backward(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_gpt2_grads* gr, int n_groups,
                        const int64_t* const* ids_d, const int32_t* Bs, const int32_t* Ts, const float* d_meanpool_d,
                        const float* d_hidden_d, const r4d_train_dropout* dropout, void* workspace_d, size_t workspace_bytes,
                        TrainModes md, hipStream_t s, const SpliceIn* sp = nullptr, float* d_fused = nullptr);
// dx[M, W.in] = epilogue(dy[M, W.out] . W^T) on the kernel dgrad_route names (train.hip): optional residual (dx = resid + ...),
// optional fused gelu_new' (dx = (...) * gelu_new'(gelu_pre); the planes routes only).  `bf16`: TrainBf16
int data_grad(const Conv1DW& W, const float* dy, int M, float* dx, const float* resid, const float* gelu_pre, hipStream_t s, int bf16 = 0);
// dW[I,J] = x[M,I]^T . dy[M,J] on the kernel wgrad_route names, db (nullable) [J] = column sums of dy (train.hip).  `part`: room for
// the slices' partials (gemm_tn_scratch_floats(I, J, M) floats); `red`: colsum_scratch_floats(M, J) floats (with db only).
// `bf16`: TrainBf16.  `x_bf16`: x is bf16 [M, lda] behind the pointer (a block train_act_bf16_block names: gemm_b1tn takes it)
int weight_grad(const float* x, const float* dy, float* dW, float* db, int I, int J, int M, int lda, int ldb, float* part, float* red,
                hipStream_t s, int bf16 = 0, bool x_bf16 = false);
int launch_splice_embed_ln(const int64_t* aug_ids, const float* fused, int r, const float* wte, const float* wpe, int vocab, int B,
                           int T, int d, const float* w, const float* b, float eps, float* x_out, float* y_out, hipStream_t s);

// ------------------------------------------------------------------ lm_head.hip (the LM head of the training steps)
struct LMLayout { size_t train, h, logits, dh, dwte, tn, ce, total; };
LMLayout lm_layout(const r4d_gpt2_config* cfg, int B, int T, int ldV, TrainModes md);
// One training step through the LM head (the bodies of r4d_gpt2_lm_train_step_f32 and r4d_rag_train_step_f32 behind their
// argument checks): forward -> head (loss, dh, dwte) -> backward -> head gradient per `head_mode` (R4D_HEAD_GRAD_*).  `md`: the
// modes the export read, for the transformer's two passes and (head_bf16) the head
int head_train_step(const char* who, const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_gpt2_grads* grads,
                    const r4d_lm_head* head, int head_mode, float* head_grad, const int64_t* ids_d, const SpliceIn* sp, int B, int T,
                    float gscale, float* loss, float* d_fused, float* hidden_out, const r4d_train_dropout* dropout, void* workspace_d,
                    size_t workspace_bytes, TrainModes md, hipStream_t s);

// ------------------------------------------------------------------ topk.hip
// rows x n values -> rows x k best (value, global index), canonical order; `counters_zeroed`: the caller already cleared
// the ticket counters (first rows * 4 bytes of ws) on this stream
template <typename T> size_t topk_ws_bytes(int rows, int n, int k);
template <typename T>
int topk_rows(const T* vals, const long long* idx_in, int rows, int n, long long ld, int k, long long index_offset, T* out_v,
              long long* out_i, void* ws, size_t ws_bytes, bool counters_zeroed, hipStream_t s);

// ------------------------------------------------------------------ topk_large.hip
// f32 rows at 64 < k <= TOPK_MAX_K (radix select + LDS sort per 16384 list positions, one launch per level); topk_rows<float> and
// topk_ws_bytes<float> route here, no other caller
constexpr int TOPK_MAX_K = 2048;
size_t topk_large_ws_bytes(int rows, int n, int k);
int topk_large_rows(const float* vals, const long long* idx_in, int rows, int n, long long ld, int k, long long index_offset,
                    float* out_v, long long* out_i, void* ws, hipStream_t s);

// ------------------------------------------------------------------ encoder_ops.hip
int launch_layernorm(const float* x, const float* w, const float* b, int rows, int d, float eps, float* y,
                     hipStream_t s);
// launch_layernorm's statistics and arithmetic (its 16-byte-lane kernel), y as bf16 [rows, d] (RNE), 16 bytes per store; d % 256 == 0
int launch_layernorm_bf16(const float* x, const float* w, const float* b, int rows, int d, float eps, unsigned short* y, hipStream_t s);
bool layernorm_lines_supported(int d);
int launch_layernorm_lines(const float* x, const float* w, const float* b, int rows, int d, float eps, unsigned short* y_lines, hipStream_t s);
constexpr int ATT_MAXG = 16;
// Up to ATT_MAXG right-padded batches handled by ONE launch of a row kernel (each batch keeps its own T): rows of the
// batches are consecutive in x / y, sequences consecutive in the pooled output.  ids[g] / emb[g]: exactly one is set.
struct RowGroups {
    int n;
    int B[ATT_MAXG], T[ATT_MAXG];
    const int64_t* ids[ATT_MAXG];
    const float* emb[ATT_MAXG];
};
int launch_embed_layernorm_groups(const RowGroups& G, const float* wte, const float* wpe, int vocab, int d,
                                  const float* w, const float* b, float eps, float* x_out, float* y_out, hipStream_t s, bool y_lines = false,
                                  bool y_bf16 = false);
int launch_causal_softmax(float* S, int nbh, int T, int ld, int row_tile, hipStream_t s, bool normalise = true);
// rows of out [B*T, d] (merged heads) divided by the row sums of the unnormalised P [B*H, T, ld] (encoder.hip: attention())
int launch_attention_rows_normalise(const float* P, float* out, int B, int T, int H, int d, int ld, hipStream_t s);
// decode step (one new position per sequence): x = (ids ? wte[id] : emb) + wpe[pos], y = LayerNorm(x)
int launch_embed_pos_layernorm(const int64_t* ids, const float* emb, const int32_t* pos, const float* wte,
                               const float* wpe, int vocab, int n_positions, int t_cap, int B, int d, const float* w,
                               const float* b, float eps, float* x_out, float* y_out, hipStream_t s,
                               void* zero_words = nullptr, size_t zero_bytes = 0);   // also clears zero_bytes at zero_words
// one query per (sequence, head) against the cached keys/values; writes the new K/V row into the cache first
int launch_decode_attention(const float* qkv_new, float* kv_layer, const int32_t* pos, int B, int t_cap, int H, int d,
                            float* out, hipStream_t s);
// device-side greedy loop state (encoder_ops.hip: greedy_advance_kernel; r4d.h: r4d_greedy_state)
struct GreedyState {
    int64_t* next; int32_t* lens; int32_t* pos; int32_t* active; int32_t* gen_len; int32_t* out_tokens;
    const int32_t* params;       // device int32[8]: max_gen, len_limit, n_eos, eos[0..3], 0
    int out_cap, t_cap;
};
// optional second job of the bookkeeping kernel: the decode step's input rows x[b,:] = wte[next[b]] + wpe[pos[b]] and the
// clearing of `n_zero` 32-bit words (the step's split-K ticket counters)
struct GreedyEmbed { const float* wte; const float* wpe; float* x_out; unsigned* zero_words; int vocab, n_positions, d, n_zero; };
int launch_greedy_advance(const float* logits, int B, int V, const GreedyState& st, hipStream_t s, const GreedyEmbed* embed = nullptr);
// sampling.hip: sample_advance_kernel in the greedy kernel's place (repetition penalty, temperature, top-k, top-p, one Philox draw per
// sequence).  seen (nullable) uint32 [B, ceil(V / 32)]; stream int32 [B]; fpar float[4] {temperature, top_p, repetition_penalty, -};
// ipar int32[4] {do_sample, top_k, seed_lo, seed_hi}, both read on the device.  With `st` the step counter is st->gen_len and the
// greedy bookkeeping follows (embed as in launch_greedy_advance); without it `step` int32 [B] counts and out_token int64 [B] is written.
// out_keep (nullable) uint32 [B, ceil(V / 32)]: the kept set; out_u (nullable) float [B]: the uniform drawn
struct SampleArgs {
    unsigned* seen; const int32_t* step; const int32_t* stream; const float* fpar; const int32_t* ipar;
    int64_t* out_token; unsigned* out_keep; float* out_u;
};
int launch_sample_advance(const float* logits, int B, int V, const SampleArgs& sa, const GreedyState* st, hipStream_t s,
                          const GreedyEmbed* embed = nullptr);
int sample_advance_prepare();      // the kernel's LDS attribute on the current device (also before a capture)
// beam.hip: the beam step's choice (r4d.h, "Beam search").  Rows R = B0 * n, rows b n .. b n + n - 1 the beams of prompt b.
// fpar float[4] {length_penalty, repetition_penalty, -, -}, read on the device; the other fields as r4d_beam_state names them;
// out_score / out_flat [B0, 2n]: the merged candidates, written by the single operation only
struct BeamArgs {
    int n;
    unsigned* seen; const float* fpar; float* beam_scores; int32_t* beam_idx; float* cand_score; int32_t* cand_id;
    int32_t *lo, *hi, *group_active, *done, *hyp_count, *hyp_added, *status;
    double *worst, *hyp_score; int32_t *hyp_len, *hyp_seq, *hyp_ids;
    float* out_score; int32_t* out_flat;
};
int launch_beam_rows(const float* logits, int R, int V, const BeamArgs& ba, hipStream_t s);       // the 2n best of every row
// the prompts' 2n best; with `st`: the reference's walk over them, the bookkeeping and (embed) the decode step's input rows
int launch_beam_advance(int B0, int V, const BeamArgs& ba, const GreedyState* st, const GreedyEmbed* embed, hipStream_t s);
int beam_rows_prepare();           // as sample_advance_prepare
int launch_kv_reorder(float* kv, const int* src_row, const int* lo, const int* hi, const int* active, int n_layer, int B0, int n, int t_cap,
                      int d, hipStream_t s);
// Up to ATT_MAXG right-padded batches (each with its own T) in ONE attention launch: the workgroup index walks the sequences
// of all batches; the batch of a sequence is found by a short scan of the prefix table (kernel argument, by value).
struct AttnGroups {
    int n;
    int seq_prefix[ATT_MAXG + 1];     // first global sequence index of each batch
    int T[ATT_MAXG];
    long long row0[ATT_MAXG];         // first token row of each batch in qkv / out
};
// attention_h2.hip: the same attention on the fp16 matrix cores (f16x2 form), qkv as uint32 "h2 words" (csrc/h2.h; written by
// gemm_h2's EPI_H2WORDS epilogue or launch_pack_h2_words); head_dim 32 / 64 / 96 / 128 / 256 (attention_h2_supported)
bool attention_h2_supported(int H, int d);
int launch_attention_h2_groups(const unsigned* qkv_words, int n, const int* Bs, const int* Ts, const long long* row0s, int H, int d,
                               float* out, hipStream_t s, bool out_lines = false, const unsigned* kblk = nullptr);
// the key-blocked K image of h2 words (attention_h2.hip: attn_h2_kernel<HD, true>): [ceil(M / 32)][H][hd / 8][2][32][4] uint32
int launch_pack_kblk_words(const unsigned* qkv_words, long long M, int H, int d, unsigned* kblk, hipStream_t s);
static inline size_t kblk_words(size_t M, int d) { return (M + 31) / 32 * 32 * (size_t)d; }
int launch_pack_h2_words(const float* x, long long n, unsigned* words, hipStream_t s);
int dbgflag_att_h2();
// attention_fused.hip: R4D_OK / error, or +1 when head_dim has no fused instantiation
int launch_attention_fused(const float* qkv, int B, int T, int H, int d, float* out, hipStream_t s);
int launch_attention_fused_groups(const float* qkv, int n, const int* Bs, const int* Ts, const long long* row0s, int H,
                                  int d, float* out, hipStream_t s);
extern int g_attention_variant;
// attention_b1.hip: the encoder's opt-in bf16 attention (r4d_set_encode_attention_bf16; NOT fp32-accurate): the groups of one launch
// as launch_attention_fused_groups takes them; qkv fp32 or bf16 [rows, 3d], out fp32 or bf16 [rows, d].  Shapes outside
// attention_b1_supported (head_dim % 16, 16 .. 256) and launches of more than 65,535 sequences are refused before any launch
bool attention_b1_supported(int H, int d);
int launch_attention_b1_groups(const void* qkv, bool qkv_bf16, int n, const int* Bs, const int* Ts, const long long* row0s, int H, int d,
                               void* out, bool out_bf16, hipStream_t s);
extern int g_encode_attn_bf16;       // r4d_set_encode_attention_bf16: read by the encoder entries, only while g_encode_bf16 is on
extern int g_encode_act_bf16;        // r4d_set_encode_act_bf16: read by the encoder entries, only while g_encode_bf16 is on
extern int g_attention_fused;        // -1 auto (default), 1 fused, 0 three-launch GEMM form (r4d_set_attention_fused)
// Layer 0's repeated pad rows (encoder.hip: encode_impl).  The layer-0 c_attn row depends on (token, position) only,
// so 32-row blocks (by GLOBAL row index, as in the key-blocked image) whose rows all carry one candidate token c are dropped from
// that GEMM and filled afterwards from `Tcap` TABLE rows (c, p), p = 0 .. Tcap - 1, that ride along at row Mp = round_up(M, 32).
// One region of 32-bit words in the workspace holds the plan of a call, all of it written on the device before it is read:
//   hdr[0] n_list (kept blocks + table blocks, padded with repeats of the last entry to a multiple of 4), hdr[1] n_drop, hdr[2] c,
//   hdr[3] / hdr[4] the word offsets of the two lists from hdr;  int64 tab_ids[Tcap];  tok[Mp];  pos[Mp];  list[lmax];  drop[nblk];
//   hist[vocab] (counts of the sequences' last-position tokens: c = the most frequent, ties to the lowest id)
constexpr int PAD_ROWS_HDR = 8;
struct PadRowsPlan {
    int M, Mp, Tmax, Tcap, nblk, ntab, lmax, vocab;
    size_t words() const { return (size_t)PAD_ROWS_HDR + 2 * (size_t)Tcap + lmax + nblk + 2 * (size_t)Mp + vocab; }
    size_t rows() const { return (size_t)Mp + Tcap; }            // rows of x, the LayerNorm lines, qkv and the key-blocked image
};
static inline PadRowsPlan pad_rows_plan(size_t M, int Tmax, int vocab) {
    PadRowsPlan p;
    p.M = (int)M; p.Mp = (int)((M + 31) / 32 * 32); p.Tmax = Tmax; p.Tcap = (Tmax + 31) / 32 * 32;
    p.nblk = p.Mp / 32; p.ntab = p.Tcap / 32; p.lmax = (p.nblk + p.ntab + 3) / 4 * 4; p.vocab = vocab;
    return p;
}
struct PadRowsBuf {
    int* hdr; long long* tab_ids; int *list, *drop, *tok, *pos, *hist;
};
static inline PadRowsBuf pad_rows_buf(int* hdr, const PadRowsPlan& p) {
    PadRowsBuf b;
    b.hdr = hdr; b.tab_ids = reinterpret_cast<long long*>(hdr + PAD_ROWS_HDR);
    b.tok = hdr + PAD_ROWS_HDR + 2 * p.Tcap; b.pos = b.tok + p.Mp; b.list = b.pos + p.Mp; b.drop = b.list + p.lmax; b.hist = b.drop + p.nblk;      // (tok: 16-byte aligned)
    return b;
}
// tok / pos of the rows of up to ATT_MAXG batches (first row: row_base) and the last-position counts (hist cleared by the caller)
int launch_pad_rows_gather(const RowGroups& G, int vocab, long long row_base, const PadRowsBuf& b, hipStream_t s);
// c, the two block lists, the header and the table's ids; one workgroup, no host synchronisation
int launch_pad_rows_classify(const PadRowsPlan& p, const PadRowsBuf& b, hipStream_t s);
// q and v words and the key-blocked K pieces of every dropped block's rows, from the table rows of their positions
int launch_pad_rows_fill(const PadRowsPlan& p, const PadRowsBuf& b, unsigned* qkv_words, unsigned* kblk, int d, hipStream_t s);
// gemm_h2p.hip with the row-block map: the h2-word c_attn over the listed blocks only (a.M = the rows that exist: p.rows())
int launch_gemm_h2p_rowmap(const S3Args& a, const unsigned short* a_lines, const PadRowsPlan& p, const PadRowsBuf& b, hipStream_t stream);
constexpr int LNF_ROWS_PER_CHUNK = 16;
size_t lnf_meanpool_scratch_floats(int B, int T, int d);
// x / hidden_out: first row of the first batch; pool_out: first sequence of the first batch; scratch: the sum over the
// batches of lnf_meanpool_scratch_floats
int launch_lnf_meanpool_groups(const RowGroups& G, const float* x, const float* w, const float* b, int d, float eps,
                               float* hidden_out, float* pool_out, float* scratch, hipStream_t s);

}  // namespace r4d
