// C-ABI entry points of the GPT-2 encoder: orchestration of the gfx950 kernels, no device allocation,
// everything enqueued on the caller's stream (graph-capturable).  See include/r4d.h for the contract.
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "common.h"

namespace r4d {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int g_gemm_split3 = 1;                // r4d_set_gemm_split3: 0 exact f32, 1 bf16x3, 2 f16x2
int g_encode_bf16 = 0;                // r4d_set_encode_bf16: the encoder calls' Conv1D GEMMs in plain bf16 (gemm_b1.hip), whatever the mode above
int g_encode_attn_bf16 = 0;           // r4d_set_encode_attention_bf16: ... and their attention on bf16 operands (attention_b1.hip); read only while the switch above is on
int g_encode_act_bf16 = 0;            // r4d_set_encode_act_bf16: ... and ln1 / ln2 / f as bf16 between producer and consumer; read only while r4d_set_encode_bf16 is on

int conv1d(const Conv1DW& W, const float* x, const float* resid, int M, int epilogue, float* y, hipStream_t s, const Conv1DOpts& opts) {
    const int K = W.in, N = W.out;
    const GemmRoute route = conv1d_route(W, M, epilogue, opts.skinny_scratch != nullptr, opts.bf16);
    R4D_REQUIRE(!(opts.x_bf16 || epilogue == EPI_GELU_KEEP_BF16) || route == ROUTE_B1,
                "conv1d: a bf16 activation block (train-act-bf16) needs the plain-bf16 GEMM, but this [%d, %d] weight carries no bf16x3 planes (*_w3)", K, N);
    switch (route) {
        case ROUTE_B1:
            if (opts.bf16 == BF16_TRAIN) R4D_BRANCH(TB_FWD);
            else if (opts.bf16 == BF16_TRAIN_HEAD) R4D_BRANCH(TBH_LOGITS);
            if (opts.x_bf16) {                                      // a bf16 block of the training step (r4d_set_train_act_bf16)
                S3Args a = s3_args(x, W.w3, W.b, resid, M, K, N, epilogue, y);
                a.a_bf16 = 1;
                R4D_BRANCH(TAB_FWD);
                return launch_gemm_b1(a, s);
            }
            return launch_gemm_b1(s3_args(x, W.w3, W.b, resid, M, K, N, epilogue, y), s);
        case ROUTE_SKINNY:
            return launch_gemm_skinny(x, W.wT, W.b, resid, M, K, N, epilogue, y, opts.skinny_scratch, s, nullptr, nullptr, 0.f,
                                      opts.counters_zeroed);
        case ROUTE_H2: return launch_gemm_h2(s3_args(x, W.h2, W.b, resid, M, K, N, epilogue, y), s);
        case ROUTE_S3: return launch_gemm_s3(s3_args(x, W.w3, W.b, resid, M, K, N, epilogue, y), s);
        default: break;
    }
    R4D_REQUIRE(epilogue != EPI_H2WORDS, "conv1d: the h2-word epilogue exists in the f16x2 GEMM only");
    const bool kcopy = route == ROUTE_F32_KCOPY;
    return launch_gemm_f32(gemm_args(x, kcopy ? W.wT : W.w, kcopy, W.b, resid, M, K, N, epilogue, y), s);
}

// Conv1D whose input rows are f16x2 LINES written by their producer (gemm_h2p.hip): f16x2 mode only, so it is no route of
// conv1d; out_lines: the GELU epilogue writes the result as lines too (c_fc -> mlp.c_proj)
// kblk / kb_hd (c_attn with the h2-word epilogue only): the K third goes to the key-blocked image of attention_h2.hip
static int conv1d_lines(const Conv1DW& W, const unsigned short* x_lines, const float* resid, int M, int epilogue, void* y, bool out_lines,
                        hipStream_t s, unsigned* kblk = nullptr, int kb_hd = 0) {
    S3Args a = s3_args(nullptr, W.h2, W.b, resid, M, W.in, W.out, epilogue, (float*)y);
    a.kblk = kblk; a.kb_hd = kb_hd;
    return launch_gemm_h2p(a, x_lines, out_lines, s);
}

static inline int tpad(int T) { return (T + 127) / 128 * 128; }

// Attention._attn + split_heads/merge_heads (modeling_gpt2.py:140-175) as three launches over the packed
// c_attn output: batched per-head Q.K^T (tiles above the diagonal skipped, logits DIVIDED by sqrt(hd) as
// in :143), in-place causal softmax weights exp(s - max), batched P.V (K-loop trimmed to the causal range) writing
// straight into the merged-head layout -- and a fourth, small one that divides the rows of P.V by the row sums (normalising P
// first costs 1.4e-5 on a row of ~1000 equal weights: launch_attention_rows_normalise).  The B*H*T*T score block (29 MB at the worst UCI_13 batch) stays in
// the 256 MB Infinity Cache between the launches.
int g_attention_fused = -1;           // -1 auto (by head_dim), 0 three launches, 1 fused wherever instantiated
int g_attention_h2 = 1;               // r4d_set_attention_h2: in f16x2 mode, head_dim 128 / 256 on the fp16 matrix cores (attention_h2.hip)
static int g_attention_kblk = -1;     // tuning aid, read once: R4D_ATT_KBLK=0 keeps the row-major K words (the key-blocked image needs the LDS-DMA c_attn)

static int attention(const float* qkv, int B, int T, int H, int d, float* a_out, float* scores, hipStream_t s) {
    // Measured on MI355X (tools/attn_bench.py, B=128, T=128..300): the fused kernels are 1.15-2.7x faster than the
    // three-launch form at every instantiated head_dim (key-split kernel for hd 32 / 64, column-split for 96 / 128 / 256),
    // so auto == fused; head dims without an instantiation fall through to the GEMM form.
    const bool fused = g_attention_fused != 0;
    if (fused) {
        const int rc_f = launch_attention_fused(qkv, B, T, H, d, a_out, s);
        if (rc_f <= 0) return rc_f;                      // +1: no fused instantiation for this head_dim
    }
    R4D_BRANCH(ATT_3LAUNCH);
    const int hd = d / H, ld = tpad(T);
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = qkv; g.B = qkv + d; g.C = scores;
    g.M = T; g.N = T; g.K = hd; g.lda = 3 * d; g.ldb = 3 * d; g.ldc = ld;
    g.b_trans = 1; g.b_rows = T; g.nbatch = B * H; g.nb1 = H;
    g.sA0 = (long long)T * 3 * d; g.sA1 = hd; g.sB0 = g.sA0; g.sB1 = hd;
    g.sC0 = (long long)H * T * ld; g.sC1 = (long long)T * ld;
    g.epilogue = EPI_SCALE_DIV; g.scale_div = (float)sqrt((double)hd); g.causal = CAUSAL_QK;
    int rc = launch_gemm_f32(g, s);
    if (rc) return rc;
    rc = launch_causal_softmax(scores, B * H, T, ld, 128, s, /*normalise=*/false);
    if (rc) return rc;
    memset(&g, 0, sizeof(g));
    g.A = scores; g.B = qkv + 2 * d; g.C = a_out;
    g.M = T; g.N = hd; g.K = T; g.lda = ld; g.ldb = 3 * d; g.ldc = d;
    g.b_trans = 0; g.b_rows = T; g.nbatch = B * H; g.nb1 = H;
    g.sA0 = (long long)H * T * ld; g.sA1 = (long long)T * ld;
    g.sB0 = (long long)T * 3 * d; g.sB1 = hd; g.sC0 = (long long)T * d; g.sC1 = hd;
    g.a_cols = ld;
    g.epilogue = EPI_NONE; g.scale_div = 1.f; g.causal = CAUSAL_PV;
    rc = launch_gemm_f32(g, s);
    if (rc) return rc;
    return launch_attention_rows_normalise(scores, a_out, B, T, H, d, ld, s);
}

struct Group {                 // one right-padded reference batch inside a fused launch sequence
    const int64_t* ids; const float* emb; int B, T; size_t row0, seq0;
};

static RowGroups row_groups(const Group* groups, int g0, int n_groups) {
    RowGroups R;
    R.n = n_groups - g0 < ATT_MAXG ? n_groups - g0 : ATT_MAXG;
    for (int j = 0; j < ATT_MAXG; ++j) {
        const bool in = j < R.n;
        R.B[j] = in ? groups[g0 + j].B : 0; R.T[j] = in ? groups[g0 + j].T : 0;
        R.ids[j] = in ? groups[g0 + j].ids : nullptr; R.emb[j] = in ? groups[g0 + j].emb : nullptr;
    }
    return R;
}

// The batches g0 .. of one attention launch (ATT_MAXG at the most) as the attention launchers take them; returns how many,
// *nseq their sequences (a launch holds 65,535)
static int attn_chunk(const Group* groups, int g0, int n_groups, int* Bs, int* Ts, long long* r0, int* nseq) {
    const int n = n_groups - g0 < ATT_MAXG ? n_groups - g0 : ATT_MAXG;
    *nseq = 0;
    for (int j = 0; j < n; ++j) {
        Bs[j] = groups[g0 + j].B; Ts[j] = groups[g0 + j].T; r0[j] = (long long)groups[g0 + j].row0;
        *nseq += Bs[j];
    }
    return n;
}

struct Workspace {
    float *x, *ln, *qkv, *att, *fc, *scores, *pool;
    unsigned* kblk;       // key-blocked K words of the f16x2 attention (attention_h2.hip): ceil32(M) x d
    int* pad_rows;        // the plan of layer 0's repeated pad rows (common.h: PadRowsPlan); null in the decode workspaces
    size_t pad_rows_off;
    size_t bytes;
};
// `pr` (the encoder calls): x, the LayerNorm rows, qkv and the key-blocked image get room for the table rows behind
// round_up(M, 32) -- pr->rows() rows where there were M -- and the plan's words follow the key-blocked image
static Workspace carve(void* base, size_t M, size_t score_floats, size_t pool_floats, int d, const PadRowsPlan* pr = nullptr) {
    size_t off = 0;
    auto take = [&](size_t nfloat) {
        float* p = base ? (float*)((char*)base + off) : nullptr;
        off += align_up(nfloat * sizeof(float), 256);
        return p;
    };
    const size_t Mx = pr ? pr->rows() : M;
    Workspace w;
    w.x = take(Mx * d); w.ln = take(Mx * d); w.qkv = take(Mx * 3 * d); w.att = take(M * d); w.fc = take(M * 4 * d);
    w.scores = take(score_floats);
    w.pool = take(pool_floats);
    w.kblk = reinterpret_cast<unsigned*>(take(kblk_words(Mx, d)));
    w.pad_rows_off = off;
    w.pad_rows = pr ? reinterpret_cast<int*>(take(pr->words())) : nullptr;
    w.bytes = off;
    return w;
}
static int g_layer0_pad_rows = -1;    // r4d_set_layer0_pad_rows; -1: R4D_LAYER0_PAD_ROWS in the environment, read once (default on)
static int layer0_pad_rows_on() {
    if (g_layer0_pad_rows < 0) { const char* e = getenv("R4D_LAYER0_PAD_ROWS"); g_layer0_pad_rows = e ? atoi(e) != 0 : 1; }
    return g_layer0_pad_rows;
}
static PadRowsPlan groups_pad_rows_plan(const r4d_gpt2_config* cfg, size_t M, int n_groups, const int32_t* Ts) {
    int Tmax = 1;
    for (int g = 0; g < n_groups; ++g) Tmax = Ts[g] > Tmax ? Ts[g] : Tmax;
    return pad_rows_plan(M, Tmax, cfg->vocab > 0 ? cfg->vocab : 1);
}
static size_t score_floats(int B, int H, int T) { return (size_t)B * H * T * tpad(T); }

static int check_cfg(const r4d_gpt2_config* c) {
    R4D_REQUIRE(c != nullptr, "gpt2: null config");
    R4D_REQUIRE(c->n_layer >= 1 && c->n_head >= 1 && c->n_embd >= 64, "gpt2: bad config L=%d H=%d d=%d", c->n_layer,
                c->n_head, c->n_embd);
    R4D_REQUIRE(c->n_embd % 64 == 0 && c->n_embd <= 2048, "gpt2: n_embd=%d must be a multiple of 64, <= 2048", c->n_embd);
    R4D_REQUIRE(c->n_embd % c->n_head == 0 && (c->n_embd / c->n_head) % 16 == 0,
                "gpt2: head_dim=%d/%d must be a multiple of 16", c->n_embd, c->n_head);
    return R4D_OK;
}

}  // namespace r4d

using namespace r4d;

extern "C" {

int r4d_abi_version(void) { return R4D_ABI_VERSION; }
int r4d_build_flags(void) {
    return dbgflag_kc() | (dbgflag_att() << 1) | (dbgflag_sk() << 2) | (dbgflag_jac() << 3) | (dbgflag_scan() << 4) | (dbgflag_s3() << 5) | (dbgflag_h2() << 6) | (dbgflag_att_h2() << 7);
}
int r4d_fold_layernorm_f32(const float* wT_d, const float* ln_w_d, const float* ln_b_d, int32_t N, int32_t K, float* wTg_d,
                           float* lnc_d, void* stream) {
    return launch_fold_layernorm(wT_d, ln_w_d, ln_b_d, N, K, wTg_d, lnc_d, (hipStream_t)stream);
}
// The decode step's weight-stream GEMM alone (gemm_skinny.hip): every check that launch_gemm_skinny leaves to its callers,
// then launch_gemm_skinny itself -- the same kernels, chosen the same way
size_t r4d_conv1d_skinny_workspace_bytes(int32_t K, int32_t N) {
    return gemm_skinny_supported(1, K, N) ? sizeof(float) * gemm_skinny_scratch_floats(K, N) : 0;
}
int r4d_conv1d_skinny_f32(const float* x_d, const float* wT_d, const float* bias_d, const float* residual_d, int32_t M, int32_t K,
                          int32_t N, int32_t epilogue, const float* ln_w_d, const float* ln_b_d, float ln_eps, const float* ln_fold_d,
                          int32_t counters_zeroed, float* y_d, void* workspace_d, size_t workspace_bytes, void* stream) {
    R4D_REQUIRE(gemm_skinny_supported(M, K, N), "conv1d_skinny: unsupported shape M=%d K=%d N=%d (1 <= M <= 32, K a multiple of 256, N >= 1)",
                M, K, N);
    R4D_REQUIRE(x_d && wT_d && y_d && workspace_d, "conv1d_skinny: null pointer");
    R4D_REQUIRE(((uintptr_t)x_d % 16) == 0 && ((uintptr_t)wT_d % 16) == 0, "conv1d_skinny: x and wT must be 16-byte aligned");
    R4D_REQUIRE(epilogue == EPI_NONE || epilogue == EPI_GELU || epilogue == EPI_RESIDUAL, "conv1d_skinny: epilogue=%d", epilogue);
    R4D_REQUIRE((epilogue == EPI_RESIDUAL) == (residual_d != nullptr), "conv1d_skinny: a residual goes with epilogue 2 and only with it");
    R4D_REQUIRE((ln_w_d != nullptr) == (ln_b_d != nullptr), "conv1d_skinny: ln_w and ln_b come together");
    R4D_REQUIRE(!ln_fold_d || !ln_w_d, "conv1d_skinny: a folded LayerNorm (ln_fold) and a per-launch one (ln_w, ln_b) exclude each other");
    R4D_REQUIRE((!ln_w_d && !ln_fold_d) || gemm_skinny_fuses_ln(M, K, N), "conv1d_skinny: LayerNorm needs K = 512 or 768, got K=%d", K);
    R4D_REQUIRE(((uintptr_t)ln_w_d % 16) == 0 && ((uintptr_t)ln_b_d % 16) == 0, "conv1d_skinny: ln_w and ln_b must be 16-byte aligned");
    if (workspace_bytes < r4d_conv1d_skinny_workspace_bytes(K, N)) {
        set_error("conv1d_skinny: workspace too small (%zu < %zu bytes)", workspace_bytes, r4d_conv1d_skinny_workspace_bytes(K, N));
        return R4D_ERR_WORKSPACE;
    }
    return launch_gemm_skinny(x_d, wT_d, bias_d, residual_d, M, K, N, epilogue, y_d, (float*)workspace_d, (hipStream_t)stream, ln_w_d,
                              ln_b_d, ln_eps, counters_zeroed != 0, ln_fold_d);
}

int r4d_set_gemm_split3(int32_t mode) { g_gemm_split3 = mode == 2 ? 2 : (mode != 0); return R4D_OK; }
int r4d_get_gemm_split3(void) { return g_gemm_split3; }
int r4d_set_encode_bf16(int32_t on) {
    const int prev = g_encode_bf16;
    g_encode_bf16 = on != 0;
    return prev;
}
int r4d_get_encode_bf16(void) { return g_encode_bf16; }
int r4d_set_encode_attention_bf16(int32_t on) {
    const int prev = g_encode_attn_bf16;
    g_encode_attn_bf16 = on != 0;
    return prev;
}
int r4d_get_encode_attention_bf16(void) { return g_encode_attn_bf16; }
int r4d_set_encode_act_bf16(int32_t on) {
    const int prev = g_encode_act_bf16;
    g_encode_act_bf16 = on != 0;
    return prev;
}
int r4d_get_encode_act_bf16(void) { return g_encode_act_bf16; }
int r4d_set_range_flag(uint32_t* flag_d) { g_range_flag = flag_d; return R4D_OK; }
int r4d_set_attention_kblk(int32_t on) {
    const int prev = g_attention_kblk < 0 ? 1 : g_attention_kblk;
    g_attention_kblk = on != 0;
    return prev;
}
int r4d_set_attention_h2(int32_t on) {
    const int prev = g_attention_h2;
    g_attention_h2 = on != 0;
    return prev;
}

int r4d_set_attention_fused(int32_t mode) {
    // mode 2: fused with the key-split kernel forced at head_dim 96/128/256 (A/B tuning); 1: fused (column-split there)
    g_attention_variant = (mode == 2) ? 1 : 0;
    g_attention_fused = mode < 0 ? -1 : (mode != 0);
    return R4D_OK;
}
const char* r4d_last_error(void) { return g_err; }

size_t r4d_gpt2_workspace_bytes(const r4d_gpt2_config* cfg, int32_t B, int32_t T) {
    if (!cfg || B <= 0 || T <= 0) return 0;
    const PadRowsPlan pr = groups_pad_rows_plan(cfg, (size_t)B * T, 1, &T);
    return carve(nullptr, (size_t)B * T, score_floats(B, cfg->n_head, T), lnf_meanpool_scratch_floats(B, T, cfg->n_embd),
                 cfg->n_embd, &pr).bytes;
}

size_t r4d_gpt2_groups_workspace_bytes(const r4d_gpt2_config* cfg, int32_t n_groups, const int32_t* Bs,
                                       const int32_t* Ts) {
    if (!cfg || n_groups <= 0 || !Bs || !Ts) return 0;
    size_t M = 0, sc = 0, pl = 0;
    for (int g = 0; g < n_groups; ++g) {
        if (Bs[g] <= 0 || Ts[g] <= 0) return 0;
        M += (size_t)Bs[g] * Ts[g];
        const size_t f = score_floats(Bs[g], cfg->n_head, Ts[g]);
        if (f > sc) sc = f;
        pl += lnf_meanpool_scratch_floats(Bs[g], Ts[g], cfg->n_embd);      // all batches pooled by one launch
    }
    const PadRowsPlan pr = groups_pad_rows_plan(cfg, M, n_groups, Ts);
    return carve(nullptr, M, sc, pl, cfg->n_embd, &pr).bytes;
}

// tests: the byte offset of the pad-row plan's header in a workspace of r4d_gpt2_groups_workspace_bytes (0: bad arguments)
size_t r4d_gpt2_layer0_pad_rows_offset(const r4d_gpt2_config* cfg, int32_t n_groups, const int32_t* Bs, const int32_t* Ts) {
    if (!cfg || n_groups <= 0 || !Bs || !Ts) return 0;
    size_t M = 0, sc = 0, pl = 0;
    for (int g = 0; g < n_groups; ++g) {
        if (Bs[g] <= 0 || Ts[g] <= 0) return 0;
        M += (size_t)Bs[g] * Ts[g];
        const size_t f = score_floats(Bs[g], cfg->n_head, Ts[g]);
        if (f > sc) sc = f;
        pl += lnf_meanpool_scratch_floats(Bs[g], Ts[g], cfg->n_embd);
    }
    const PadRowsPlan pr = groups_pad_rows_plan(cfg, M, n_groups, Ts);
    return carve(nullptr, M, sc, pl, cfg->n_embd, &pr).pad_rows_off;
}

int r4d_set_layer0_pad_rows(int32_t on) {
    const int prev = layer0_pad_rows_on();
    g_layer0_pad_rows = on != 0;
    return prev;
}

}  // extern "C"

namespace r4d {

// The whole encoder over G right-padded batches.  Row-wise work (LayerNorm, the four Conv1D GEMMs per block)
// runs ONCE over the concatenated rows of all batches -- a mean-pooled embedding depends on its own batch's
// padding only through the attention / position / pooling steps, which stay per batch -- so a launch sees
// G times more tiles and the GEMM tail (a CU holds ~3 tiles of a single 32 x T batch) amortises.
static int encode_impl(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const Group* groups, int n_groups,
                       float* out_hidden_d, float* out_meanpool_d, float* out_layers_d, float* out_qkv_d,
                       void* workspace_d, size_t workspace_bytes, hipStream_t s) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    R4D_REQUIRE(w && w->wte && w->wpe && w->ln_f_w && w->ln_f_b && w->layers, "gpt2: null weights");
    R4D_REQUIRE(out_hidden_d || out_meanpool_d, "gpt2: no output requested");
    const int d = cfg->n_embd, H = cfg->n_head;
    size_t Mtot = 0, sc = 0, pl = 0;
    int Tmax = 1;
    bool all_ids = true;
    for (int g = 0; g < n_groups; ++g) {
        const Group& G = groups[g];
        Tmax = G.T > Tmax ? G.T : Tmax;
        all_ids = all_ids && G.ids != nullptr;
        R4D_REQUIRE((G.ids != nullptr) != (G.emb != nullptr),
                    "gpt2: specify exactly one of input_ids and inputs_embeds");     // modeling_gpt2.py:400-401,409
        R4D_REQUIRE(G.B >= 1 && G.T >= 1, "gpt2: empty batch B=%d T=%d", G.B, G.T);
        R4D_REQUIRE(G.T <= cfg->n_positions && G.T <= 1024, "gpt2: T=%d exceeds n_positions=%d", G.T, cfg->n_positions);
        Mtot += (size_t)G.B * G.T;
        const size_t f = score_floats(G.B, H, G.T);
        if (f > sc) sc = f;
        pl += lnf_meanpool_scratch_floats(G.B, G.T, d);
    }
    R4D_REQUIRE(Mtot <= 0x7fffffff / (size_t)(16 * d), "gpt2: %zu rows in one call is too many", Mtot);   // [M,4d] f32 byte offsets fit 31 bits
    const int M = (int)Mtot;
    const PadRowsPlan pr = pad_rows_plan(Mtot, Tmax, cfg->vocab > 0 ? cfg->vocab : 1);
    Workspace ws = carve(workspace_d, Mtot, sc, pl, d, &pr);
    if (!workspace_d || workspace_bytes < ws.bytes) {
        set_error("gpt2: workspace %zu bytes < required %zu", workspace_bytes, ws.bytes);
        return R4D_ERR_WORKSPACE;
    }
    for (int l = 0; l < cfg->n_layer; ++l) {
        const r4d_gpt2_layer& L = w->layers[l];
        R4D_REQUIRE(L.ln_1_w && L.c_attn_w && L.attn_proj_w && L.ln_2_w && L.c_fc_w && L.mlp_proj_w,
                    "gpt2: null weight in layer %d", l);
        const Conv1DW Wqkv = conv1d_w(L, C_ATTN, d), Wo = conv1d_w(L, ATTN_PROJ, d), Wfc = conv1d_w(L, C_FC, d), Wp = conv1d_w(L, MLP_PROJ, d);
        const Conv1DOpts enc{nullptr, false, g_encode_bf16 ? BF16_ENCODE : BF16_OFF};
        // f16x2 mode, round 5: the LayerNorms write their rows as f16x2 LINES, the c_fc GELU epilogue too, and c_attn / c_fc /
        // mlp.c_proj take them through LDS-DMA (gemm_h2p.hip) -- the values of the register-staged gemm_h2 path, bit for bit
        // (r4d_set_gemm_h2p(0) keeps that one); the buffers keep their size (4 bytes per element either way)
        // (bf16 precision takes the structure of the bf16x3 path: fp32 activations, exact-f32 attention, no lines or h2 words;
        //  its own switches move the attention and the activations to bf16 below)
        const bool lines = !g_encode_bf16 && g_gemm_split3 == 2 && g_gemm_h2p && Wqkv.h2 && Wfc.h2 && Wp.h2 && layernorm_lines_supported(d) &&
                           gemm_h2p_supported(M, d, 3 * d) && gemm_h2p_supported(M, d, 4 * d) && gemm_h2p_supported(M, 4 * d, d);
        unsigned short* ln_lines = reinterpret_cast<unsigned short*>(ws.ln);
        unsigned short* fc_lines = reinterpret_cast<unsigned short*>(ws.fc);
        float* qkv = out_qkv_d ? out_qkv_d + (size_t)l * M * 3 * d : ws.qkv;
        // f16x2 mode, head_dim 128 / 256, qkv not handed out: c_attn writes h2 words (csrc/h2.h) and the attention runs on
        // the fp16 matrix cores (attention_h2.hip); every other case: fp32 qkv and the exact-f32 kernels below
        bool words = !g_encode_bf16 && !out_qkv_d && g_attention_h2 && g_attention_fused != 0 && g_gemm_split3 == 2 && Wqkv.h2 &&
                     attention_h2_supported(H, d) && gemm_h2_supported(M, d, 3 * d);
        int Bs[ATT_MAXG], Ts[ATT_MAXG], nseq;                   // one attention launch's batches (attn_chunk)
        long long r0[ATT_MAXG];
        for (int g0 = 0; g0 < n_groups && words; g0 += ATT_MAXG) {
            attn_chunk(groups, g0, n_groups, Bs, Ts, r0, &nseq);
            if (nseq > 65535) words = false;
        }
        // bf16 precision with the attention switch ("bf16+attn"): the attention on bf16 operands (attention_b1.hip) wherever that kernel
        // serves the shape, else this block takes the route of "bf16" alone (counted).  bf16 BETWEEN producer and consumer where
        // nothing else reads the fp32 form: c_attn on gemm_b1 writes RN(q | k | v) as bf16 [M, 3d] unless the caller asked for qkv
        // (then fp32 as before, and the kernel rounds while staging: the same bits), the attention writes RN(O) as bf16 [M, d]
        // where attn.c_proj is on gemm_b1, which reads it as its bf16 A operand.  Both fit the fp32 buffers.
        const bool want_battn = g_encode_bf16 && g_encode_attn_bf16;
        bool battn = want_battn && attention_b1_supported(H, d);
        for (int g0 = 0; g0 < n_groups && battn; g0 += ATT_MAXG) {
            attn_chunk(groups, g0, n_groups, Bs, Ts, r0, &nseq);
            if (nseq > 65535) battn = false;
        }
        if (want_battn && !battn) R4D_BRANCH(EBA_FALLBACK);
        const bool qkv_b = battn && !out_qkv_d && conv1d_route(Wqkv, M, EPI_NONE, false, BF16_ENCODE) == ROUTE_B1;
        const bool att_b = battn && conv1d_route(Wo, M, EPI_RESIDUAL, false, BF16_ENCODE) == ROUTE_B1;
        // bf16 precision with the activation switch (r4d_set_encode_act_bf16): ln1, ln2 and f are rounded ONCE where they are produced and
        // travel as bf16 [M, width] in the first half of ws.ln / ws.fc to a gemm_b1 that reads them as its bf16 A operand -- the bits it
        // would have rounded while staging the fp32 form.  Per buffer (conv1d_route.h: encode_act_bf16_block), counted
        const bool want_act = g_encode_bf16 && g_encode_act_bf16;
        const bool ln1_b = encode_act_bf16_block(ACT_LN1, want_act, Wqkv, Wfc, Wp, M, d), ln2_b = encode_act_bf16_block(ACT_LN2, want_act, Wqkv, Wfc, Wp, M, d),
                   f_b = encode_act_bf16_block(ACT_F, want_act, Wqkv, Wfc, Wp, M, d);
        if (want_act) {
            if (ln1_b) R4D_BRANCH(EAB_LN1); else R4D_BRANCH(EAB_KEPT_F32);
            if (ln2_b) R4D_BRANCH(EAB_LN2); else R4D_BRANCH(EAB_KEPT_F32);
            if (f_b) R4D_BRANCH(EAB_F); else R4D_BRANCH(EAB_KEPT_F32);
        }
        unsigned short* ln_b16 = reinterpret_cast<unsigned short*>(ws.ln);
        // ... and its K third as the key-blocked image the head_dim 128 / 256 kernel loads by whole cache lines (attention_h2.hip)
        if (g_attention_kblk < 0) { const char* e = getenv("R4D_ATT_KBLK"); g_attention_kblk = e ? atoi(e) != 0 : 1; }
        const bool kblk = words && lines && g_attention_kblk && (d / H) % 32 == 0;      // every head_dim attention_h2.hip serves
        // Layer 0 on that path, every batch given as ids: the c_attn row of a position depends on (token, position) only, so the
        // 32-row blocks that hold ONE token throughout -- the reference's right padding, 58 % of the bench step's blocks -- leave
        // the GEMM and are filled from `Tcap` table rows that ride along behind round_up(M, 32) (common.h: PadRowsPlan; bit-identical)
        const bool pad0 = l == 0 && kblk && all_ids && layer0_pad_rows_on() && (3 * d) % 256 == 0 && gemm_h2p_supported((int)pr.rows(), d, 3 * d) &&
                          pr.rows() <= 0x7fffffff / (size_t)(16 * d);
        const PadRowsBuf pb = pad_rows_buf(ws.pad_rows, pr);
        if (pad0) {
            if (hipMemsetAsync(pb.hist, 0, (size_t)pr.vocab * sizeof(int), s) != hipSuccess) { set_error("gpt2: memset of the token counts failed"); return R4D_ERR_HIP; }
            for (int g0 = 0; g0 < n_groups; g0 += ATT_MAXG)
                if ((rc = launch_pad_rows_gather(row_groups(groups, g0, n_groups), cfg->vocab, (long long)groups[g0].row0, pb, s))) return rc;
            if ((rc = launch_pad_rows_classify(pr, pb, s))) return rc;
        }
        if (l == 0) {
            for (int g0 = 0; g0 < n_groups; g0 += ATT_MAXG) {          // ATT_MAXG batches per launch
                const RowGroups R = row_groups(groups, g0, n_groups);
                const size_t r0 = groups[g0].row0;
                rc = launch_embed_layernorm_groups(R, w->wte, w->wpe, cfg->vocab, d, L.ln_1_w, L.ln_1_b, cfg->ln_eps,
                                                   ws.x + r0 * d, ln1_b ? reinterpret_cast<float*>(ln_b16 + r0 * d) : ws.ln + r0 * d, s, lines, ln1_b);
                if (rc) return rc;
            }
            if (pad0) {                                                   // the table: one sequence of Tmax positions, every id = c
                RowGroups R = {};
                R.n = 1; R.B[0] = 1; R.T[0] = pr.Tmax; R.ids[0] = reinterpret_cast<const int64_t*>(pb.tab_ids);
                if ((rc = launch_embed_layernorm_groups(R, w->wte, w->wpe, cfg->vocab, d, L.ln_1_w, L.ln_1_b, cfg->ln_eps,
                                                        ws.x + (size_t)pr.Mp * d, ws.ln + (size_t)pr.Mp * d, s, lines))) return rc;
            }
        } else if ((rc = lines ? launch_layernorm_lines(ws.x, L.ln_1_w, L.ln_1_b, M, d, cfg->ln_eps, ln_lines, s)
                       : ln1_b ? launch_layernorm_bf16(ws.x, L.ln_1_w, L.ln_1_b, M, d, cfg->ln_eps, ln_b16, s)
                               : launch_layernorm(ws.x, L.ln_1_w, L.ln_1_b, M, d, cfg->ln_eps, ws.ln, s))) {
            return rc;
        }
        if (out_layers_d &&
            hipMemcpyAsync(out_layers_d + (size_t)l * M * d, ws.x, (size_t)M * d * sizeof(float),
                           hipMemcpyDeviceToDevice, s) != hipSuccess) {
            set_error("gpt2: layer copy failed");
            return R4D_ERR_HIP;
        }
        if (kblk && !pad0 && (M & 31) &&        // the last block's rows past M are never written: keep them finite (they are masked keys at most)
            hipMemsetAsync(ws.kblk + (size_t)(M / 32) * 32 * d, 0, (size_t)32 * d * sizeof(unsigned), s) != hipSuccess) {
            set_error("gpt2: memset of the key-block tail failed");
            return R4D_ERR_HIP;
        }
        if (pad0) {                    // (writes the last block whole: its rows past M as copies of row M - 1)
            S3Args a = s3_args(nullptr, Wqkv.h2, Wqkv.b, nullptr, (int)pr.rows(), d, 3 * d, EPI_H2WORDS, qkv);
            a.kblk = ws.kblk; a.kb_hd = d / H;
            if ((rc = launch_gemm_h2p_rowmap(a, ln_lines, pr, pb, s))) return rc;
            rc = launch_pad_rows_fill(pr, pb, reinterpret_cast<unsigned*>(qkv), ws.kblk, d, s);
        } else if (lines) rc = conv1d_lines(Wqkv, ln_lines, nullptr, M, words ? EPI_H2WORDS : EPI_NONE, qkv, false, s, kblk ? ws.kblk : nullptr, kblk ? d / H : 0);
        else if (qkv_b || ln1_b) {          // (ln1_b: c_attn is on gemm_b1 by the rule)
            S3Args a = s3_args(ws.ln, Wqkv.w3, Wqkv.b, nullptr, M, d, 3 * d, qkv_b ? EPI_NONE_BF16 : EPI_NONE, qkv);
            a.a_bf16 = ln1_b;
            rc = launch_gemm_b1(a, s);
        }
        else rc = conv1d(Wqkv, ws.ln, nullptr, M, words ? EPI_H2WORDS : EPI_NONE, qkv, s, enc);
        if (rc) return rc;
        // ... and with them the attention output: attn_h2_kernel writes its merged-head rows as lines for attn.c_proj
        const bool att_lines = words && lines && Wo.h2 && gemm_h2p_supported(M, d, d);
        bool fused_done = false;
        if (battn) {
            fused_done = true;
            for (int g0 = 0; g0 < n_groups; g0 += ATT_MAXG) {
                const int n = attn_chunk(groups, g0, n_groups, Bs, Ts, r0, &nseq);
                if ((rc = launch_attention_b1_groups(qkv, qkv_b, n, Bs, Ts, r0, H, d, ws.att, att_b, s))) return rc;
            }
        } else if (words) {
            fused_done = true;
            for (int g0 = 0; g0 < n_groups; g0 += ATT_MAXG) {
                const int n = attn_chunk(groups, g0, n_groups, Bs, Ts, r0, &nseq);
                if ((rc = launch_attention_h2_groups(reinterpret_cast<const unsigned*>(qkv), n, Bs, Ts, r0, H, d, ws.att, s, att_lines,
                                                     kblk ? ws.kblk : nullptr))) return rc;
            }
        } else if (g_attention_fused != 0) {             // all batches of the call in ceil(n/16) fused launches
            fused_done = true;
            for (int g0 = 0; g0 < n_groups && fused_done; g0 += ATT_MAXG) {
                const int n = attn_chunk(groups, g0, n_groups, Bs, Ts, r0, &nseq);
                if (nseq > 65535) { fused_done = false; break; }
                rc = launch_attention_fused_groups(qkv, n, Bs, Ts, r0, H, d, ws.att, s);
                if (rc < 0) return rc;
                if (rc > 0) fused_done = false;          // no fused instantiation for this head_dim
            }
        }
        if (!fused_done) {
            for (int g = 0; g < n_groups; ++g) {
                const Group& G = groups[g];
                if ((rc = attention(qkv + G.row0 * 3 * d, G.B, G.T, H, d, ws.att + G.row0 * d, ws.scores, s))) return rc;
            }
        }
        if (att_lines) rc = conv1d_lines(Wo, reinterpret_cast<const unsigned short*>(ws.att), ws.x, M, EPI_RESIDUAL, ws.x, false, s);
        else if (att_b) {
            S3Args a = s3_args(ws.att, Wo.w3, Wo.b, ws.x, M, d, d, EPI_RESIDUAL, ws.x);
            a.a_bf16 = 1;
            rc = launch_gemm_b1(a, s);
        } else rc = conv1d(Wo, ws.att, ws.x, M, EPI_RESIDUAL, ws.x, s, enc);
        if (rc) return rc;
        if (lines) {
            if ((rc = launch_layernorm_lines(ws.x, L.ln_2_w, L.ln_2_b, M, d, cfg->ln_eps, ln_lines, s))) return rc;
            if ((rc = conv1d_lines(Wfc, ln_lines, nullptr, M, EPI_GELU, fc_lines, true, s))) return rc;
            if ((rc = conv1d_lines(Wp, fc_lines, ws.x, M, EPI_RESIDUAL, ws.x, false, s))) return rc;
            continue;
        }
        if ((rc = ln2_b ? launch_layernorm_bf16(ws.x, L.ln_2_w, L.ln_2_b, M, d, cfg->ln_eps, ln_b16, s)
                        : launch_layernorm(ws.x, L.ln_2_w, L.ln_2_b, M, d, cfg->ln_eps, ws.ln, s))) return rc;
        if (ln2_b) {                        // (c_fc is on gemm_b1 by the rule; f_b implies ln2_b)
            S3Args a = s3_args(ws.ln, Wfc.w3, Wfc.b, nullptr, M, d, 4 * d, f_b ? EPI_GELU_BF16 : EPI_GELU, ws.fc);
            a.a_bf16 = 1;
            rc = launch_gemm_b1(a, s);
        } else rc = conv1d(Wfc, ws.ln, nullptr, M, EPI_GELU, ws.fc, s, enc);
        if (rc) return rc;
        if (f_b) {
            S3Args a = s3_args(ws.fc, Wp.w3, Wp.b, ws.x, M, 4 * d, d, EPI_RESIDUAL, ws.x);
            a.a_bf16 = 1;
            rc = launch_gemm_b1(a, s);
        } else rc = conv1d(Wp, ws.fc, ws.x, M, EPI_RESIDUAL, ws.x, s, enc);
        if (rc) return rc;
    }
    size_t part0 = 0;                                                   // scratch offset of the launch's first batch
    for (int g0 = 0; g0 < n_groups; g0 += ATT_MAXG) {
        const RowGroups R = row_groups(groups, g0, n_groups);
        const Group& G = groups[g0];
        rc = launch_lnf_meanpool_groups(R, ws.x + G.row0 * d, w->ln_f_w, w->ln_f_b, d, cfg->ln_eps,
                                        out_hidden_d ? out_hidden_d + G.row0 * d : nullptr,
                                        out_meanpool_d ? out_meanpool_d + G.seq0 * d : nullptr, ws.pool + part0, s);
        if (rc) return rc;
        for (int j = 0; j < R.n; ++j) part0 += lnf_meanpool_scratch_floats(R.B[j], R.T[j], d);
    }
    return R4D_OK;
}

}  // namespace r4d

extern "C" {

int r4d_gpt2_encode_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const int64_t* ids_d,
                        const float* inputs_embeds_d, int32_t B, int32_t T, float* out_hidden_d,
                        float* out_meanpool_d, float* out_layers_d, float* out_qkv_d, void* workspace_d,
                        size_t workspace_bytes, void* stream) {
    Group G = {ids_d, inputs_embeds_d, B, T, 0, 0};
    return encode_impl(cfg, w, &G, 1, out_hidden_d, out_meanpool_d, out_layers_d, out_qkv_d, workspace_d,
                       workspace_bytes, (hipStream_t)stream);
}

int r4d_gpt2_encode_groups_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, int32_t n_groups,
                               const int64_t* const* ids_d, const int32_t* Bs, const int32_t* Ts,
                               float* out_meanpool_d, void* workspace_d, size_t workspace_bytes, void* stream) {
    R4D_REQUIRE(n_groups >= 1 && n_groups <= 4096 && ids_d && Bs && Ts, "gpt2 groups: bad arguments");
    R4D_REQUIRE(out_meanpool_d, "gpt2 groups: out_meanpool_d is null");
    std::vector<Group> gs((size_t)n_groups);
    size_t row0 = 0, seq0 = 0;
    for (int g = 0; g < n_groups; ++g) {
        gs[g] = Group{ids_d[g], nullptr, Bs[g], Ts[g], row0, seq0};
        if (Bs[g] > 0 && Ts[g] > 0) { row0 += (size_t)Bs[g] * Ts[g]; seq0 += (size_t)Bs[g]; }
    }
    return encode_impl(cfg, w, gs.data(), n_groups, nullptr, out_meanpool_d, nullptr, nullptr, workspace_d,
                       workspace_bytes, (hipStream_t)stream);
}

int r4d_gpt2_encode_groups_ex_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, int32_t n_groups,
                                  const int64_t* const* ids_d, const float* const* embeds_d, const int32_t* Bs,
                                  const int32_t* Ts, float* out_hidden_d, float* out_meanpool_d, float* out_qkv_d,
                                  void* workspace_d, size_t workspace_bytes, void* stream) {
    R4D_REQUIRE(n_groups >= 1 && n_groups <= 4096 && Bs && Ts, "gpt2 groups: bad arguments");
    R4D_REQUIRE((ids_d != nullptr) != (embeds_d != nullptr), "gpt2 groups: specify exactly one of ids_d and embeds_d");
    std::vector<Group> gs((size_t)n_groups);
    size_t row0 = 0, seq0 = 0;
    for (int g = 0; g < n_groups; ++g) {
        gs[g] = Group{ids_d ? ids_d[g] : nullptr, embeds_d ? embeds_d[g] : nullptr, Bs[g], Ts[g], row0, seq0};
        if (Bs[g] > 0 && Ts[g] > 0) { row0 += (size_t)Bs[g] * Ts[g]; seq0 += (size_t)Bs[g]; }
    }
    return encode_impl(cfg, w, gs.data(), n_groups, out_hidden_d, out_meanpool_d, nullptr, out_qkv_d, workspace_d,
                       workspace_bytes, (hipStream_t)stream);
}

// decode workspace: the per-row buffers of the encoder + the split-K scratch of the skinny GEMM (largest projection:
// K = 4d, N = d and K = d, N = 4d both give (4d / 256) * 32 * 4d... the max of the four shapes is taken)
static size_t decode_skinny_floats(int d) {
    size_t m = 0;
    const int shapes[4][2] = {{d, 3 * d}, {d, d}, {d, 4 * d}, {4 * d, d}};
    for (auto& kn : shapes)
        if (gemm_skinny_supported(1, kn[0], kn[1])) { const size_t f = gemm_skinny_scratch_floats(kn[0], kn[1]); if (f > m) m = f; }
    return m;
}

size_t r4d_gpt2_decode_workspace_bytes(const r4d_gpt2_config* cfg, int32_t B) {
    if (!cfg || B <= 0) return 0;
    return carve(nullptr, (size_t)B, 0, decode_skinny_floats(cfg->n_embd), cfg->n_embd).bytes;
}

// y = epilogue(LayerNorm(x) . W + b) in ONE weight-stream launch (gemm_skinny_fuses_ln), the counters clear: on the LayerNorm
// pre-folded into a decode-only copy of the weight when the layer carries it, else on wT with the gain and shift
static int skinny_ln(const Conv1DW& W, const float* x, const float* ln_w, const float* ln_b, float eps, int M, int epilogue, float* y,
                     float* sk, hipStream_t s) {
    const bool folded = W.wTg && W.lnc;
    return launch_gemm_skinny(x, folded ? W.wTg : W.wT, W.b, nullptr, M, W.in, W.out, epilogue, y, sk, s, folded ? nullptr : ln_w,
                              folded ? nullptr : ln_b, eps, true, folded ? W.lnc : nullptr);
}

// `x_ready`: the un-normalised input rows are already in the workspace's x buffer and the ticket counters are clear (the
// greedy step's bookkeeping kernel did both): no embedding launch, layer 0 reads its LayerNorm like every other layer
static int decode_step_impl(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const int64_t* ids_d,
                            const float* inputs_embeds_d, const int32_t* pos_d, float* kv_cache_d, int32_t B,
                            int32_t t_cap, float* out_hidden_d, void* workspace_d, size_t workspace_bytes,
                            void* stream, bool x_ready) {
    hipStream_t s = (hipStream_t)stream;
    int rc = check_cfg(cfg);
    if (rc) return rc;
    R4D_REQUIRE(w && w->wte && w->wpe && w->ln_f_w && w->ln_f_b && w->layers, "gpt2 decode: null weights");
    R4D_REQUIRE(x_ready || (ids_d != nullptr) != (inputs_embeds_d != nullptr), "gpt2 decode: specify exactly one of ids and inputs_embeds");
    R4D_REQUIRE(pos_d && kv_cache_d && out_hidden_d, "gpt2 decode: null pointer");
    R4D_REQUIRE(B >= 1 && t_cap >= 1, "gpt2 decode: B=%d t_cap=%d", B, t_cap);
    const int d = cfg->n_embd, H = cfg->n_head;
    const size_t sk_floats = decode_skinny_floats(d);
    Workspace ws = carve(workspace_d, (size_t)B, 0, sk_floats, d);
    if (!workspace_d || workspace_bytes < ws.bytes) {
        set_error("gpt2 decode: workspace %zu bytes < required %zu", workspace_bytes, ws.bytes);
        return R4D_ERR_WORKSPACE;
    }
    float* sk = (sk_floats && B <= 32) ? ws.pool : nullptr;         // M <= 32: the projections run as weight streams
    const size_t layer_stride = (size_t)B * t_cap * 2 * d;
    size_t cbytes = 0;                                              // split-K ticket counters of the projections: cleared once per
    void* cnt = sk ? gemm_skinny_counters(sk, &cbytes) : nullptr;   // step, by the step's first kernel
    for (int l = 0; l < cfg->n_layer; ++l) {
        const r4d_gpt2_layer& L = w->layers[l];
        R4D_REQUIRE(L.ln_1_w && L.c_attn_w && L.attn_proj_w && L.ln_2_w && L.c_fc_w && L.mlp_proj_w,
                    "gpt2 decode: null weight in layer %d", l);
        const Conv1DW Wqkv = conv1d_w_decode(conv1d_w(L, C_ATTN, d)), Wo = conv1d_w_decode(conv1d_w(L, ATTN_PROJ, d)),
                      Wfc = conv1d_w_decode(conv1d_w(L, C_FC, d)), Wp = conv1d_w_decode(conv1d_w(L, MLP_PROJ, d));
        const Conv1DOpts first{sk, false, BF16_OFF}, later{sk, true, BF16_OFF};    // the two residual projections promise clear ticket counters
        // M <= 32 and d in {512, 768}: LayerNorm runs inside the projection that reads it (gemm_skinny8_kernel) -- x stays
        // the un-normalised residual stream and two launches per layer disappear
        const bool fuse_ln = sk && Wqkv.wT && Wfc.wT && gemm_skinny_fuses_ln(B, d, 3 * d);
        if (l == 0 && !x_ready)
            rc = launch_embed_pos_layernorm(ids_d, inputs_embeds_d, pos_d, w->wte, w->wpe, cfg->vocab, cfg->n_positions,
                                            t_cap, B, d, L.ln_1_w, L.ln_1_b, cfg->ln_eps, ws.x, ws.ln, s, cnt, cbytes);
        else if (!fuse_ln)
            rc = launch_layernorm(ws.x, L.ln_1_w, L.ln_1_b, B, d, cfg->ln_eps, ws.ln, s);
        if (rc) return rc;
        if (fuse_ln && (l > 0 || x_ready))
            rc = skinny_ln(Wqkv, ws.x, L.ln_1_w, L.ln_1_b, cfg->ln_eps, B, EPI_NONE, ws.qkv, sk, s);
        else
            rc = conv1d(Wqkv, ws.ln, nullptr, B, EPI_NONE, ws.qkv, s, first);
        if (rc) return rc;
        if ((rc = launch_decode_attention(ws.qkv, kv_cache_d + (size_t)l * layer_stride, pos_d, B, t_cap, H, d, ws.att, s)))
            return rc;
        if ((rc = conv1d(Wo, ws.att, ws.x, B, EPI_RESIDUAL, ws.x, s, later))) return rc;
        if (fuse_ln) {
            rc = skinny_ln(Wfc, ws.x, L.ln_2_w, L.ln_2_b, cfg->ln_eps, B, EPI_GELU, ws.fc, sk, s);
        } else {
            if ((rc = launch_layernorm(ws.x, L.ln_2_w, L.ln_2_b, B, d, cfg->ln_eps, ws.ln, s))) return rc;
            rc = conv1d(Wfc, ws.ln, nullptr, B, EPI_GELU, ws.fc, s, first);
        }
        if (rc) return rc;
        if ((rc = conv1d(Wp, ws.fc, ws.x, B, EPI_RESIDUAL, ws.x, s, later))) return rc;
    }
    return launch_layernorm(ws.x, w->ln_f_w, w->ln_f_b, B, d, cfg->ln_eps, out_hidden_d, s);
}

int r4d_gpt2_decode_step_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const int64_t* ids_d,
                             const float* inputs_embeds_d, const int32_t* pos_d, float* kv_cache_d, int32_t B,
                             int32_t t_cap, float* out_hidden_d, void* workspace_d, size_t workspace_bytes,
                             void* stream) {
    return decode_step_impl(cfg, w, ids_d, inputs_embeds_d, pos_d, kv_cache_d, B, t_cap, out_hidden_d, workspace_d, workspace_bytes,
                            stream, false);
}

static size_t greedy_pool_floats(const r4d_gpt2_config* cfg) {
    const size_t a = decode_skinny_floats(cfg->n_embd);
    const size_t b = gemm_skinny_supported(1, cfg->n_embd, cfg->vocab) ? gemm_skinny_scratch_floats(cfg->n_embd, cfg->vocab) : 0;
    return a > b ? a : b;
}

size_t r4d_gpt2_greedy_workspace_bytes(const r4d_gpt2_config* cfg, int32_t B) {
    if (!cfg || B <= 0) return 0;
    return carve(nullptr, (size_t)B, 0, greedy_pool_floats(cfg), cfg->n_embd).bytes;
}

// One step of a device-side decode loop: the LM head, the choice of the next token -- argmax (sa == ba == nullptr), the sampler
// (sa: sampling.hip) or the beam step (ba: beam.hip; B rows in groups of ba->n, then the reordering of the cache) -- with the bookkeeping,
// then the cached step on the chosen ids
static int advance_step(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_greedy_state* st, const SampleArgs* sa,
                        const BeamArgs* ba, float* kv_cache_d, int32_t B, int32_t t_cap, void* workspace_d, size_t workspace_bytes,
                        void* stream) {
    hipStream_t s = (hipStream_t)stream;
    int rc = check_cfg(cfg);
    if (rc) return rc;
    const char* who = ba ? "gpt2 beam" : sa ? "gpt2 sample" : "gpt2 greedy";
    R4D_REQUIRE(w && w->wte && st && st->last_d && st->logits_d, "%s: null pointer", who);
    R4D_REQUIRE(B >= 1 && t_cap >= 1, "%s: B=%d t_cap=%d", who, B, t_cap);
    const int d = cfg->n_embd, V = cfg->vocab;
    Workspace ws = carve(workspace_d, (size_t)B, 0, greedy_pool_floats(cfg), d);
    if (!workspace_d || workspace_bytes < ws.bytes) {
        set_error("%s: workspace %zu bytes < required %zu", who, workspace_bytes, ws.bytes);
        return R4D_ERR_WORKSPACE;
    }
    const float* head = w->lm_head ? w->lm_head : w->wte;            // untied checkpoints carry their own lm_head.weight
    if (B <= 32 && gemm_skinny_supported(B, d, V))                   // lm_head on B rows: a weight stream like the projections
        rc = launch_gemm_skinny(st->last_d, head, nullptr, nullptr, B, d, V, EPI_NONE, st->logits_d, ws.pool, s);
    else
        rc = r4d_lm_logits_f32(st->last_d, head, B, V, d, st->logits_d, stream);
    if (rc) return rc;
    GreedyState g;
    g.next = st->next_d; g.lens = st->lens_d; g.pos = st->pos_d; g.active = st->active_d; g.gen_len = st->gen_len_d;
    g.out_tokens = st->out_tokens_d; g.params = st->params_d; g.out_cap = st->out_cap; g.t_cap = t_cap;
    // the bookkeeping kernel also writes the chosen token's input row into the step's x buffer and clears the ticket counters
    GreedyEmbed ge;
    ge.wte = w->wte; ge.wpe = w->wpe; ge.x_out = ws.x; ge.vocab = cfg->vocab; ge.n_positions = cfg->n_positions; ge.d = d;
    size_t cbytes = 0;
    void* cnt = ws.pool ? gemm_skinny_counters(ws.pool, &cbytes) : nullptr;
    ge.zero_words = (unsigned*)cnt; ge.n_zero = (int)(cbytes / 4);
    if (ba) {
        R4D_REQUIRE(kv_cache_d && B % ba->n == 0, "%s: null cache or %d rows in groups of %d", who, B, ba->n);
        if ((rc = launch_beam_rows(st->logits_d, B, V, *ba, s))) return rc;
        if ((rc = launch_beam_advance(B / ba->n, V, *ba, &g, &ge, s))) return rc;
        rc = launch_kv_reorder(kv_cache_d, ba->beam_idx, ba->lo, ba->hi, ba->group_active, cfg->n_layer, B / ba->n, ba->n, t_cap, d, s);
    } else {
        rc = sa ? launch_sample_advance(st->logits_d, B, V, *sa, &g, s, &ge) : launch_greedy_advance(st->logits_d, B, V, g, s, &ge);
    }
    if (rc) return rc;
    return decode_step_impl(cfg, w, st->next_d, nullptr, st->pos_d, kv_cache_d, B, t_cap, st->last_d, workspace_d, workspace_bytes,
                            stream, true);
}

int r4d_gpt2_greedy_step_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_greedy_state* st,
                             float* kv_cache_d, int32_t B, int32_t t_cap, void* workspace_d, size_t workspace_bytes,
                             void* stream) {
    return advance_step(cfg, w, st, nullptr, nullptr, kv_cache_d, B, t_cap, workspace_d, workspace_bytes, stream);
}

// the sampled step's state as the greedy fields + the sampler's arguments
static bool split_sample_state(const r4d_sample_state* st, r4d_greedy_state* g, SampleArgs* sa) {
    if (!st || !st->stream_d || !st->fparams_d || !st->iparams_d) return false;
    *g = r4d_greedy_state{st->last_d, st->logits_d, st->next_d, st->lens_d, st->pos_d, st->active_d, st->gen_len_d, st->out_tokens_d,
                          st->params_d, st->out_cap};
    *sa = SampleArgs{st->seen_d, nullptr, st->stream_d, st->fparams_d, st->iparams_d, nullptr, nullptr, nullptr};
    return true;
}

size_t r4d_gpt2_sample_workspace_bytes(const r4d_gpt2_config* cfg, int32_t B) { return r4d_gpt2_greedy_workspace_bytes(cfg, B); }

int r4d_gpt2_sample_step_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_sample_state* st,
                             float* kv_cache_d, int32_t B, int32_t t_cap, void* workspace_d, size_t workspace_bytes,
                             void* stream) {
    r4d_greedy_state g;
    SampleArgs sa;
    R4D_REQUIRE(split_sample_state(st, &g, &sa), "gpt2 sample: null pointer");
    return advance_step(cfg, w, &g, &sa, nullptr, kv_cache_d, B, t_cap, workspace_d, workspace_bytes, stream);
}

struct r4d_decode_graph { hipGraph_t graph; hipGraphExec_t exec; };

static int capture_step(const char* who, const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_greedy_state* st,
                        const SampleArgs* sa, const BeamArgs* ba, float* kv_cache_d, int32_t B, int32_t t_cap, void* workspace_d,
                        size_t workspace_bytes, r4d_decode_graph** out_graph) {
    R4D_REQUIRE(out_graph, "%s: null out_graph", who);
    *out_graph = nullptr;
    R4D_REQUIRE(!g_prof_on, "%s: switch the launch profiler off before capturing", who);
    if (sa) { const int prc = sample_advance_prepare(); if (prc) return prc; }
    if (ba) { const int prc = beam_rows_prepare(); if (prc) return prc; }
    hipStream_t cap = nullptr;                                       // the caller's stream may be the null stream: not capturable
    R4D_HIP(hipStreamCreateWithFlags(&cap, hipStreamNonBlocking));
    hipError_t e = hipStreamBeginCapture(cap, hipStreamCaptureModeRelaxed);
    if (e != hipSuccess) {
        (void)hipStreamDestroy(cap);
        set_error("%s: begin capture: %s", who, hipGetErrorString(e));
        return R4D_ERR_HIP;
    }
    const int rc = advance_step(cfg, w, st, sa, ba, kv_cache_d, B, t_cap, workspace_d, workspace_bytes, cap);
    hipGraph_t graph = nullptr;
    e = hipStreamEndCapture(cap, &graph);                            // always end the capture, also after an error
    (void)hipStreamDestroy(cap);
    if (rc) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
    }
    if (e != hipSuccess || !graph) {
        set_error("%s: end capture: %s", who, hipGetErrorString(e));
        return R4D_ERR_HIP;
    }
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGraphDestroy(graph);
        set_error("%s: instantiate: %s", who, hipGetErrorString(e));
        return R4D_ERR_HIP;
    }
    *out_graph = new r4d_decode_graph{graph, exec};
    return R4D_OK;
}

int r4d_gpt2_greedy_graph_create(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_greedy_state* st,
                                 float* kv_cache_d, int32_t B, int32_t t_cap, void* workspace_d, size_t workspace_bytes,
                                 r4d_decode_graph** out_graph) {
    return capture_step("gpt2 greedy graph", cfg, w, st, nullptr, nullptr, kv_cache_d, B, t_cap, workspace_d, workspace_bytes, out_graph);
}

int r4d_gpt2_sample_graph_create(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_sample_state* st,
                                 float* kv_cache_d, int32_t B, int32_t t_cap, void* workspace_d, size_t workspace_bytes,
                                 r4d_decode_graph** out_graph) {
    r4d_greedy_state g;
    SampleArgs sa;
    if (out_graph) *out_graph = nullptr;
    R4D_REQUIRE(split_sample_state(st, &g, &sa), "gpt2 sample graph: null pointer");
    return capture_step("gpt2 sample graph", cfg, w, &g, &sa, nullptr, kv_cache_d, B, t_cap, workspace_d, workspace_bytes, out_graph);
}

// the beam step's state as the greedy fields (per row) + the beam kernels' arguments
static bool split_beam_state(const r4d_beam_state* st, r4d_greedy_state* g, BeamArgs* ba) {
    if (!st || !st->fparams_d || st->n_beams < 2 || st->n_beams > R4D_BEAM_MAX) return false;
    *g = r4d_greedy_state{st->last_d, st->logits_d, st->next_d, st->lens_d, st->pos_d, st->active_d, st->gen_len_d, st->out_tokens_d,
                          st->params_d, st->out_cap};
    *ba = BeamArgs{st->n_beams, st->seen_d, st->fparams_d, st->beam_scores_d, st->beam_idx_d, st->cand_scores_d, st->cand_ids_d,
                   st->lo_d, st->hi_d, st->group_active_d, st->done_d, st->hyp_count_d, st->hyp_added_d, st->status_d,
                   st->hyp_worst_d, st->hyp_score_d, st->hyp_len_d, st->hyp_seq_d, st->hyp_ids_d, nullptr, nullptr};
    return true;
}

size_t r4d_gpt2_beam_workspace_bytes(const r4d_gpt2_config* cfg, int32_t B0, int32_t n_beams) {
    if (B0 <= 0 || n_beams < 2 || n_beams > R4D_BEAM_MAX || (long long)B0 * n_beams > 0x7fffffffLL) return 0;
    return r4d_gpt2_greedy_workspace_bytes(cfg, B0 * n_beams);
}

int r4d_gpt2_beam_step_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_beam_state* st, float* kv_cache_d,
                           int32_t B0, int32_t t_cap, void* workspace_d, size_t workspace_bytes, void* stream) {
    r4d_greedy_state g;
    BeamArgs ba;
    R4D_REQUIRE(split_beam_state(st, &g, &ba), "gpt2 beam: null pointer or n_beams outside [2, %d]", R4D_BEAM_MAX);
    R4D_REQUIRE(B0 >= 1 && (long long)B0 * ba.n <= 0x7fffffffLL, "gpt2 beam: B0=%d", B0);
    return advance_step(cfg, w, &g, nullptr, &ba, kv_cache_d, B0 * ba.n, t_cap, workspace_d, workspace_bytes, stream);
}

int r4d_gpt2_beam_graph_create(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_beam_state* st, float* kv_cache_d,
                               int32_t B0, int32_t t_cap, void* workspace_d, size_t workspace_bytes, r4d_decode_graph** out_graph) {
    r4d_greedy_state g;
    BeamArgs ba;
    if (out_graph) *out_graph = nullptr;
    R4D_REQUIRE(split_beam_state(st, &g, &ba), "gpt2 beam graph: null pointer or n_beams outside [2, %d]", R4D_BEAM_MAX);
    R4D_REQUIRE(B0 >= 1 && (long long)B0 * ba.n <= 0x7fffffffLL, "gpt2 beam graph: B0=%d", B0);
    return capture_step("gpt2 beam graph", cfg, w, &g, nullptr, &ba, kv_cache_d, B0 * ba.n, t_cap, workspace_d, workspace_bytes, out_graph);
}

int r4d_decode_graph_launch(r4d_decode_graph* graph, int32_t n_steps, void* stream) {
    R4D_REQUIRE(graph && graph->exec && n_steps >= 0, "decode graph: null graph or n_steps=%d", n_steps);
    for (int i = 0; i < n_steps; ++i) R4D_HIP(hipGraphLaunch(graph->exec, (hipStream_t)stream));
    return R4D_OK;
}

void r4d_decode_graph_destroy(r4d_decode_graph* graph) {
    if (!graph) return;
    if (graph->exec) (void)hipGraphExecDestroy(graph->exec);
    if (graph->graph) (void)hipGraphDestroy(graph->graph);
    delete graph;
}

int r4d_lm_logits_f32(const float* hidden_d, const float* wte_d, int32_t M, int32_t V, int32_t d, float* logits_d,
                      void* stream) {
    R4D_REQUIRE(hidden_d && wte_d && logits_d, "lm_logits: null pointer");
    return launch_gemm_f32(gemm_args(hidden_d, wte_d, 1, nullptr, nullptr, M, d, V, EPI_NONE, logits_d), (hipStream_t)stream);
}

int r4d_layernorm_f32(const float* x_d, const float* w_d, const float* b_d, int32_t rows, int32_t d, float eps,
                      float* y_d, void* stream) {
    R4D_REQUIRE(x_d && w_d && b_d && y_d, "layernorm: null pointer");
    return launch_layernorm(x_d, w_d, b_d, rows, d, eps, y_d, (hipStream_t)stream);
}

int r4d_layernorm_lines_f32(const float* x_d, const float* w_d, const float* b_d, int32_t rows, int32_t d, float eps,
                            uint16_t* y_lines_d, void* stream) {
    R4D_REQUIRE(x_d && w_d && b_d && y_lines_d, "layernorm_lines: null pointer");
    return launch_layernorm_lines(x_d, w_d, b_d, rows, d, eps, y_lines_d, (hipStream_t)stream);
}

int r4d_layernorm_bf16_f32(const float* x_d, const float* w_d, const float* b_d, int32_t rows, int32_t d, float eps,
                           uint16_t* y_bf16_d, void* stream) {
    R4D_REQUIRE(x_d && w_d && b_d && y_bf16_d, "layernorm_bf16: null pointer");
    return launch_layernorm_bf16(x_d, w_d, b_d, rows, d, eps, y_bf16_d, (hipStream_t)stream);
}

int r4d_conv1d_f32(const float* x_d, const float* w_d, const float* w_t_d, const float* bias_d, const float* residual_d,
                   int32_t M, int32_t K, int32_t N, int32_t epilogue, float* y_d, void* stream) {
    R4D_REQUIRE(x_d && w_d && y_d, "conv1d: null pointer");
    R4D_REQUIRE(epilogue >= 0 && epilogue <= 2, "conv1d: epilogue %d not in {0,1,2}", epilogue);
    R4D_REQUIRE(epilogue != EPI_RESIDUAL || residual_d, "conv1d: residual epilogue needs residual_d");
    return conv1d(Conv1DW{w_d, bias_d, w_t_d, nullptr, nullptr, nullptr, nullptr, nullptr, K, N}, x_d, residual_d, M, epilogue, y_d, (hipStream_t)stream);
}

int32_t r4d_conv1d_route(int32_t kind, int32_t M, int32_t K, int32_t N, int32_t epilogue, uint32_t have, int32_t bf16) {
    return conv1d_route_query(kind, M, K, N, epilogue, have, bf16);
}
const char* r4d_conv1d_route_name(int32_t route) { return gemm_route_name(route); }

size_t r4d_attention_workspace_bytes(int32_t B, int32_t n_head, int32_t T) {
    if (B <= 0 || n_head <= 0 || T <= 0) return 0;
    return align_up((size_t)B * n_head * T * tpad(T) * sizeof(float), 256);
}

int r4d_attention_f32(const float* qkv_d, int32_t B, int32_t T, int32_t n_head, int32_t d, float* a_d,
                      void* scores_ws_d, size_t ws_bytes, void* stream) {
    R4D_REQUIRE(qkv_d && a_d && scores_ws_d, "attention: null pointer");
    R4D_REQUIRE(n_head >= 1 && d % n_head == 0 && (d / n_head) % 16 == 0, "attention: head_dim must be a multiple of 16");
    R4D_REQUIRE(T >= 1 && T <= 1024, "attention: T=%d out of range", T);
    R4D_REQUIRE(B >= 1, "attention: B=%d", B);       // the workspace size of B < 1 is 0: every buffer would pass the check below
    if (ws_bytes < r4d_attention_workspace_bytes(B, n_head, T)) {
        set_error("attention: workspace too small");
        return R4D_ERR_WORKSPACE;
    }
    return attention(qkv_d, B, T, n_head, d, a_d, (float*)scores_ws_d, (hipStream_t)stream);
}

}  // extern "C"
