// Retriever TRAINING step on gfx950: the encoder forward that KEEPS what the backward pass needs, and the
// backward pass itself -- the calculus torch autograd performs for the reference on the tensors of
// models/modeling_gpt2.py:140-235,400-509 when train/train_retriever.py:196 calls loss.backward().
//
//   forward  (r4d_gpt2_train_forward_f32):  per block  x -> ln_1 -> c_attn -> causal attention (probabilities kept) ->
//            c_proj + x -> ln_2 -> c_fc (pre-activation kept) -> gelu_new -> c_proj + x;  ln_f -> mean over T
//   backward (r4d_gpt2_train_backward_f32): d(mean-pooled embeddings) -> gradients of every parameter
// Dense contractions run on the exact-f32 MFMA GEMMs of the forward path: data gradients dX = dY . W^T read the Conv1D
// weight [in,out] as the k-contiguous B operand directly; weight gradients dW = X^T . dY read BOTH operands row by row over
// the contracted token index (the [K,M] x [K,N] form of gemm_f32_kernel, split over the tokens so that a d x d gradient still
// fills the chip, partials summed in a fixed order); attention backward is four batched per-head GEMMs around a row kernel
// (dP = dO . V^T,  dS = P (dP - rowsum(P dP)) / sqrt(hd),  dQ = dS . K,  dK = dS^T . Q,  dV = P^T . dO).
// All batches of a step (anchor, positive, negative and the two augmented views) form ONE launch sequence over their
// concatenated rows, like the inference path.  Dropout (embeddings, attention probabilities, both residual branches) draws
// its masks from a counter-based generator (train_ops.hip), so the backward regenerates them instead of storing them; the
// reference's torch RNG stream cannot be reproduced, the distribution and the calculus are the same.  Checked against the reference's autograd gradients (tests/test_gpu_training.py).
#include <math.h>
#include <string.h>
#include <vector>
#include <stdlib.h>
#include "common.h"

namespace r4d {

// train_ops.hip
size_t ln_bwd_scratch_floats(int rows, int d);
int launch_ln_bwd(const float* x, const float* w, const float* dy, const float* add, int rows, int d, float eps, float* dx,
                  float* dw, float* db, float* scratch, int accumulate, hipStream_t s);
size_t colsum_scratch_floats(long long rows, int n);
int launch_colsum(const float* x, long long rows, int n, int ld, float* out, float* scratch, int accumulate, hipStream_t s);
int launch_gelu_fwd(const float* pre, long long n, float* y, hipStream_t s);
int launch_gelu_fwd_bf16(const float* pre, long long n, unsigned short* y_bf16, hipStream_t s);
int launch_gelu_bwd(const float* pre, const float* dy, long long n, float* dx, hipStream_t s);
int launch_softmax_bwd(const float* P, float* dP, int nbh, int T, int ld, float scale_div, hipStream_t s);
int launch_transpose(const float* in, int rows, int cols, long long ld_in, long long stride_in, float* out, long long ld_out,
                     long long stride_out, int nbatch, hipStream_t s);
// recompute mode: dropout backward + softmax backward in place on dP and its transpose into dst; dropout + transpose of P
int launch_softmax_bwd_t(const float* P, float* dP, float* dst, int nbh, int T, int ld, float scale_div, float attn_p, DropKey key,
                         unsigned site, unsigned long long pbase, hipStream_t s);
int launch_dropout_transpose(const float* P, float* out, int nbh, int T, int ld, float attn_p, DropKey key, unsigned site,
                             unsigned long long pbase, hipStream_t s);
int launch_embedding_bwd(const float* dx, const int64_t* ids, int B, int T, int d, int vocab, unsigned long long* acc_wte, float* dwpe,
                         int first_group, long long table_rows, hipStream_t s);
int launch_embedding_fix_to_f32(const unsigned long long* acc, long long n, long long table_rows, float* out, hipStream_t s);
int launch_embedding_absmax(const float* dx, long long n, unsigned long long* acc_wte, long long table_elems, hipStream_t s);
int launch_meanpool_bwd(const float* d_pool, long long rows, int T, int d, float* dh, hipStream_t s);

// The process-wide training switches: ONE value (common.h: TrainModes) behind the fourteen r4d_set_train_* / r4d_get_train_*
// exports, and ONE table with a row per switch.  A row carries what differs between the exports -- the name in messages, whether the
// setter refuses a value outside 0 / 1 (`refusal`: its message, one %d) or normalises it to on != 0 (nullptr), whether it returns
// the previous value or R4D_OK -- and whether the backward must find the switch as the forward that filled its workspace left it
// (`guarded`: it would read another layout or run other arithmetic on the saved blocks).  A new switch is a TrainModes member and a
// row here, its export pair below, and whatever reads it.
static TrainModes g_modes{};
TrainModes train_modes() { return g_modes; }
struct TrainModeRow { int TrainModes::*field; const char* name; const char* refusal; bool returns_prev, guarded; };
enum { TM_ATTENTION, TM_ACTIVATIONS, TM_BF16, TM_ATTN_BF16, TM_HEAD_BF16, TM_ACT_BF16, TM_ATTN_FUSED };
static const TrainModeRow kTrainModes[] = {
    // 0 stored (the forward keeps P of every layer), 1 recompute (the backward forms P again with the forward's two launches; no
    // per-layer P blocks)
    {&TrainModes::attention, "train-attention mode", "set_train_attention: mode %d is neither 0 (stored) nor 1 (recompute)", false, true},
    // 0 stored (the forward keeps ln1 .. f of every layer), 1 recompute (it keeps each layer's input; the backward forms one layer's
    // activations at a time again, with the forward's launches, in ONE set all layers share)
    {&TrainModes::activations, "train-activations mode", "set_train_activations: mode %d is neither 0 (stored) nor 1 (recompute)", false, true},
    // 0 the gemm mode's arithmetic (default), 1 the twelve Conv1D GEMMs of a block on plain bf16 operands (gemm_b1.hip, gemm_b1tn.hip)
    // wherever the layer carries the plane and the shape is supported.  NOT fp32-accurate
    {&TrainModes::bf16, "train-bf16", nullptr, true, true},
    // 0 the six per-head attention products of a block on the exact-f32 kernel (default), 1 on plain bf16 operands (gemm_b1h.hip).
    // Independent of bf16.  NOT fp32-accurate
    {&TrainModes::attn_bf16, "train-attention-bf16", nullptr, true, true},
    // 0 the LM head's three GEMMs on the gemm mode's kernels (default), 1 on plain bf16 operands wherever the head carries the plane
    // and the shape is supported (lm_head.hip).  Independent of the two above; the retriever step has no head and does not read it, and
    // no saved block depends on it: not guarded.  NOT fp32-accurate
    {&TrainModes::head_bf16, "train-head-bf16", nullptr, true, false},
    // 0 every saved activation fp32 (default), 1 -- only while bf16 is on -- the blocks train_act_bf16_block names (ln1 of layers >= 1,
    // ln2, f) are kept as bf16: their producers round once, with the rounding the GEMMs that read them apply while staging, so every
    // result keeps its bits
    {&TrainModes::act_bf16, "train-act-bf16", "set_train_act_bf16: %d is neither 0 (fp32 activations) nor 1 (bf16 store)", true, true},
    // 0 attention as six products around a P-shaped block (default), 1 -- only TOGETHER with attn_bf16; alone every entry refuses it
    // (train_modes_ok) -- the fused kernels of attention_train_fused.hip: no P-shaped block at all, one log-sum-exp per (sequence, head,
    // query) kept instead.  `attention` has no effect then
    {&TrainModes::attn_fused, "train-attention-fused",
     "set_train_attention_fused: %d is neither 0 (six products around a P block) nor 1 (fused kernels)", false, true},
};
static_assert(sizeof(kTrainModes) / sizeof(kTrainModes[0]) == TM_ATTN_FUSED + 1, "one kTrainModes row per TM_* index, in that order");
static int set_mode(const TrainModeRow& row, int value) {
    if (row.refusal) R4D_REQUIRE(value == 0 || value == 1, row.refusal, value);
    const int prev = g_modes.*row.field;
    g_modes.*row.field = value != 0;
    return row.returns_prev ? prev : R4D_OK;
}
// tuning aid: R4D_TRAIN_FUSE_GELU=0 keeps the two element-wise GELU launches (read once)
static bool train_fuse_gelu() {
    static const int v = [] { const char* e = getenv("R4D_TRAIN_FUSE_GELU"); return e ? atoi(e) : 1; }();
    return v != 0;
}
// The most recent training forward: its workspace, the modes it ran under and, in activations-recompute mode, the layer whose
// activations that workspace's shared set holds (-1: none).  It guards the backward: on that workspace under another mode it
// would read the wrong layout -> refused; straight behind its forward it need not form the last layer's activations again.
static struct { const void* ws; TrainModes modes; int shared_layer; } g_last_fwd = {nullptr, {}, -1};

static inline int tpad128(int T) { return (T + 127) / 128 * 128; }
static inline int up4(long long x) { return (int)((x + 3) / 4 * 4); }

struct TrainGroup { const int64_t* ids; int B, T; size_t row0, seq0, p0; };     // p0: offset of the group's P block (floats)

// Workspace layout, identical in the size query, the forward and the backward (bump allocation in a fixed order)
struct TrainLayout {
    size_t M, Ptot, pmax;
    int L, d;
    // per layer (offsets in floats)
    std::vector<size_t> x_in, ln1, qkv, att, x_mid, ln2, pre, f, P, lse;
    size_t x_out, pool_scratch;
    bool recompute;                                     // no P blocks; scratch pA holds the P of the batch at hand
    bool fused;                                         // r4d_set_train_attention_fused: no P-shaped block at all (P, pA, dP, PT); lse [M H] per layer and attD [M H] instead
    size_t MH, attD;
    bool act_recompute;                                 // ln1 .. f (and P) of every layer are ONE shared set; x_in stays per layer
    // r4d_set_train_act_bf16 (train_act_bf16_block): the block is bf16 [M, width] -- half the floats at its offset
    bool act_on;
    bool bf(int which, int l) const { return train_act_bf16_block(which, l, act_on, (long long)M, d); }
    // backward temporaries (pA, dP, PT: attn_bwd's scratch blocks A, B, C; pA in recompute mode only)
    size_t dx, dy, dbig, dqkv, xT, pA, dP, PT, red;
    size_t emb_acc;                                     // [vocab, d] 64-bit fixed-point token-gradient table (two floats per entry)
    size_t total;
};

static TrainLayout layout(const r4d_gpt2_config* cfg, const TrainGroup* gs, int n, TrainModes md) {
    TrainLayout t;
    t.L = cfg->n_layer; t.d = cfg->n_embd;
    t.fused = md.attn_fused && md.attn_bf16;
    t.recompute = md.attention == 1 && !t.fused;        // (the stored / recompute switch sizes and launches nothing while fused)
    t.act_recompute = md.activations == 1;
    t.act_on = md.bf16 && md.act_bf16;
    const size_t d = t.d;
    t.M = 0; t.Ptot = 0; t.pmax = 0;
    size_t pool = 0;
    for (int g = 0; g < n; ++g) {
        t.M += (size_t)gs[g].B * gs[g].T;
        const size_t pf = (size_t)gs[g].B * cfg->n_head * gs[g].T * tpad128(gs[g].T);
        t.Ptot += pf;
        if (pf > t.pmax) t.pmax = pf;
        pool += lnf_meanpool_scratch_floats(gs[g].B, gs[g].T, t.d);
    }
    t.MH = t.M * cfg->n_head;
    size_t off = 0;
    auto take = [&](size_t nfloat) { const size_t o = off; off += (nfloat + 63) / 64 * 64; return o; };
    // a block that may be bf16 (two elements per float; M d / 2 is a multiple of 64 wherever a block qualifies)
    auto take_act = [&](int which, int l, size_t elems) { return take(t.bf(which, l) ? elems / 2 : elems); };
    for (int l = 0; l < t.L; ++l) {
        if (t.act_recompute && l >= 1) {
            // layer 0 owns its ln1 (it left the fused embedding kernel; launch_layernorm is not promised to give its bits);
            // layers 1 .. L-1 share one ln1, and every layer shares the blocks behind it
            t.x_in.push_back(take(t.M * d)); t.ln1.push_back(l == 1 ? take_act(ACT_LN1, l, t.M * d) : t.ln1[1]); t.qkv.push_back(t.qkv[0]);
            t.att.push_back(t.att[0]); t.x_mid.push_back(t.x_mid[0]); t.ln2.push_back(t.ln2[0]);
            t.pre.push_back(t.pre[0]); t.f.push_back(t.f[0]); t.P.push_back(t.P[0]); t.lse.push_back(t.lse[0]);
            continue;
        }
        t.x_in.push_back(take(t.M * d)); t.ln1.push_back(take_act(ACT_LN1, l, t.M * d)); t.qkv.push_back(take(t.M * 3 * d));
        t.att.push_back(take(t.M * d)); t.x_mid.push_back(take(t.M * d)); t.ln2.push_back(take_act(ACT_LN2, l, t.M * d));
        t.pre.push_back(take(t.M * 4 * d)); t.f.push_back(take_act(ACT_F, l, t.M * 4 * d)); t.P.push_back(t.recompute || t.fused ? 0 : take(t.Ptot));
        t.lse.push_back(t.fused ? take(t.MH) : 0);
    }
    t.x_out = take(t.M * d);
    t.pool_scratch = take(pool);
    t.dx = take(t.M * d); t.dy = take(t.M * d); t.dbig = take(t.M * 4 * d); t.dqkv = take(t.M * 3 * d);
    {   // split-K partials of the four weight-gradient shapes
        size_t sk = gemm_tn_scratch_floats(4 * t.d, t.d, (int)t.M);
        const size_t o[3] = {gemm_tn_scratch_floats(t.d, 4 * t.d, (int)t.M), gemm_tn_scratch_floats(t.d, t.d, (int)t.M),
                             gemm_tn_scratch_floats(t.d, 3 * t.d, (int)t.M)};
        for (size_t v : o) if (v > sk) sk = v;
        t.xT = take(sk);
    }
    t.pA = t.recompute ? take(t.pmax) : 0;
    t.dP = t.fused ? 0 : take(t.pmax); t.PT = t.fused ? 0 : take(t.pmax);
    t.attD = t.fused ? take(t.MH) : 0;
    size_t red = ln_bwd_scratch_floats((int)t.M, t.d);
    const size_t cs = colsum_scratch_floats((long long)t.M, 4 * t.d);
    if (cs > red) red = cs;
    t.red = take(red);
    t.emb_acc = take((size_t)cfg->vocab * d * 2 + 4);   // + two 64-bit words behind the table: poison, max |contribution|
    t.total = off;
    return t;
}

static int check_groups(const r4d_gpt2_config* cfg, int n_groups, const int64_t* const* ids_d, const int32_t* Bs, const int32_t* Ts,
                        std::vector<TrainGroup>& gs) {
    R4D_REQUIRE(cfg && cfg->n_layer >= 1 && cfg->n_embd % 64 == 0 && cfg->n_embd <= 2048 && cfg->n_head >= 1 &&
                cfg->n_embd % cfg->n_head == 0 && (cfg->n_embd / cfg->n_head) % 16 == 0, "gpt2 train: bad config");
    R4D_REQUIRE(n_groups >= 1 && n_groups <= ATT_MAXG && ids_d && Bs && Ts, "gpt2 train: 1..%d batches per step", ATT_MAXG);
    gs.resize(n_groups);
    size_t row0 = 0, seq0 = 0, p0 = 0;
    for (int g = 0; g < n_groups; ++g) {
        R4D_REQUIRE(ids_d[g] && Bs[g] >= 1 && Ts[g] >= 1 && Ts[g] <= cfg->n_positions && Ts[g] <= 1024,
                    "gpt2 train: bad batch %d (B=%d T=%d)", g, Bs[g], Ts[g]);
        R4D_REQUIRE((long long)Bs[g] * cfg->n_head <= 65535, "gpt2 train: B * n_head = %lld exceeds the batched-GEMM limit",
                    (long long)Bs[g] * cfg->n_head);
        gs[g] = TrainGroup{ids_d[g], Bs[g], Ts[g], row0, seq0, p0};
        row0 += (size_t)Bs[g] * Ts[g]; seq0 += (size_t)Bs[g];
        p0 += (size_t)Bs[g] * cfg->n_head * Ts[g] * tpad128(Ts[g]);
    }
    R4D_REQUIRE(row0 <= 0x7fffffff / (size_t)(16 * cfg->n_embd), "gpt2 train: %zu rows in one step is too many", row0);
    return R4D_OK;
}

// The data-gradient GEMM of the training steps: dx[M, W.in] = epilogue(dy[M, W.out] . W^T), dy a GRADIENT (conv1d_route.h:
// dgrad_route for the kernel and why no f16x2 form exists).  The exact-f32 kernel reads a Conv1D's w [in, out] as its k-contiguous
// operand, the LM head's table [out, in] (dh = dlogits . wte_pad) as a row-major one.
int data_grad(const Conv1DW& W, const float* dy, int M, float* dx, const float* resid, const float* gelu_pre, hipStream_t s, int bf16) {
    const int epi = gelu_pre ? EPI_GELU_GRAD : resid ? EPI_RESIDUAL : EPI_NONE;
    const GemmRoute route = dgrad_route(W, M, bf16);
    if (route != ROUTE_DGRAD_F32) {
        const S3Args a = s3_args(dy, W.w3t, nullptr, gelu_pre ? gelu_pre : resid, M, W.out, W.in, epi, dx);
        if (route == ROUTE_DGRAD_S3) return launch_gemm_s3(a, s);
        if (bf16 == TRAIN_BF16_HEAD) R4D_BRANCH(TBH_DGRAD); else R4D_BRANCH(TB_DGRAD);
        return launch_gemm_b1(a, s);
    }
    R4D_REQUIRE(!gelu_pre, "bwd_data: the fused GELU derivative needs the bf16x3 planes");
    return launch_gemm_f32(gemm_args(dy, W.w ? W.w : W.wT, W.w != nullptr, nullptr, resid, M, W.out, W.in, epi, dx), s);
}

// the matrix-core weight gradients' slices, added in slice order: dW <- part [Sx][I][J], db <- db_part [Sx][J] (null: no db)
static int reduce_slices(const float* part, const float* db_part, int Sx, float* dW, float* db, int I, int J, hipStream_t s) {
    const int rc = launch_splitk_reduce(part, (long long)I * J / 4, Sx, dW, s);
    return (rc || !db_part) ? rc : launch_splitk_reduce(db_part, (long long)(J / 4), Sx, db, s);
}

// gemm_b1tn and its reduces: dW <- RN(X)^T . RN(dY), db (nullable) <- column sums of dY.  `part` / `db_part`: room for the slices'
// partials (the slice count follows the room of `part`, at most 64; ONE slice writes dW / db itself and needs none).  *db_done:
// whether db was written.
static int wgrad_b1tn(const float* X, const float* dY, float* dW, float* db, int I, int J, int M, int lda, int ldb, float* part,
                      size_t part_floats, float* db_part, size_t db_part_floats, bool* db_done, hipStream_t s, bool x_bf16 = false) {
    R4D_REQUIRE(X && dY && dW, "gemm_b1tn: null pointer");
    R4D_REQUIRE(gemm_b1tn_supported(I, J, M, lda, ldb), "gemm_b1tn: unsupported shape I=%d J=%d M=%d lda=%d ldb=%d (I %% 128 == 0, J %% 256 == 0, M >= 32 wanted)", I, J, M, lda, ldb);
    R4D_REQUIRE(((uintptr_t)X % 16) == 0 && ((uintptr_t)dY % 16) == 0 && ((uintptr_t)dW % 16) == 0 && ((uintptr_t)part % 16) == 0,
                "gemm_b1tn: 16-byte alignment");
    const int max_s = part ? (int)(part_floats / ((size_t)I * J) > 64 ? 64 : part_floats / ((size_t)I * J)) : 1;
    const int S = gemm_tn_slices(I, J, M, max_s), Sx = tn_row_slices(M, S);
    const bool want_db = db && ((uintptr_t)db % 16) == 0 &&
                         (Sx == 1 || (db_part && ((uintptr_t)db_part % 16) == 0 && (size_t)Sx * J <= db_part_floats));
    int rc = launch_gemm_b1tn(X, dY, Sx > 1 ? part : dW, want_db ? (Sx > 1 ? db_part : db) : nullptr, I, J, M, lda, ldb, S, s, x_bf16);
    if (!rc && Sx > 1) rc = reduce_slices(part, want_db ? db_part : nullptr, Sx, dW, db, I, J, s);
    if (!rc) *db_done = want_db;
    return rc;
}

// dW[I,J] = x[M,I]^T . dy[M,J]: both operands read row by row over the contracted token index, split over it into slices whose
// partials (in `part`) are summed in slice order; db[J] = column sums of dy -- by the matrix-core kernels while they stage dy where
// `red` has the room for their slices' sums, else by the column-sum kernel.  wgrad_route names the kernel; the matrix-core
// kernels share one slice rule (the bits of dW depend on it): gemm_tn_slices, for gemm_b1tn within the room of `part` and 64, for
// gemm_s3tn within tn_splits
int weight_grad(const float* x, const float* dy, float* dW, float* db, int I, int J, int M, int lda, int ldb, float* part, float* red,
                hipStream_t s, int bf16, bool x_bf16) {
    const GemmRoute route = wgrad_route(I, J, M, lda, ldb, bf16);
    R4D_REQUIRE(!x_bf16 || route == ROUTE_WGRAD_B1TN, "weight_grad: a bf16 activation block (train-act-bf16) needs gemm_b1tn (I=%d J=%d M=%d)", I, J, M);
    if (x_bf16) R4D_BRANCH(TAB_WGRAD);
    const size_t red_floats = db ? colsum_scratch_floats(M, J) : 0;
    bool db_done = false;
    int rc;
    if (bf16 == TRAIN_BF16_HEAD) { if (route == ROUTE_WGRAD_B1TN) R4D_BRANCH(TBH_WGRAD); else R4D_BRANCH(TBH_WGRAD_FALLBACK); }
    else if (bf16) { if (route == ROUTE_WGRAD_B1TN) R4D_BRANCH(TB_WGRAD); else R4D_BRANCH(TB_WGRAD_FALLBACK); }
    if (route == ROUTE_WGRAD_B1TN) {
        rc = wgrad_b1tn(x, dy, dW, db, I, J, M, lda, ldb, part, gemm_tn_scratch_floats(I, J, M), red, red_floats, &db_done, s, x_bf16);
    } else if (route == ROUTE_WGRAD_S3TN) {
        R4D_REQUIRE(I > 0 && J > 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)dy % 16) == 0 && ((uintptr_t)dW % 16) == 0, "gemm_tn: 16-byte alignment");
        const int S = gemm_tn_slices(I, J, M, tn_splits(I, J, M));
        const bool cs = db && red && (size_t)S * J <= red_floats && ((uintptr_t)red % 16) == 0 && ((uintptr_t)db % 16) == 0;
        // (always partials and a reduce, also when only one slice holds rows)
        if ((rc = launch_gemm_s3tn(x, dy, part, cs ? red : nullptr, I, J, M, lda, ldb, S, s))) return rc;
        rc = reduce_slices(part, cs ? red : nullptr, tn_row_slices(M, S), dW, db, I, J, s);
        db_done = cs;
    } else {
        rc = launch_gemm_f32_tn(x, dy, dW, I, J, M, lda, ldb, part, s);
    }
    if (rc) return rc;
    return (db && !db_done) ? launch_colsum(dy, M, J, ldb, db, red, 0, s) : R4D_OK;
}

struct DropCtx {                                                  // dropout of one step; p == 0 everywhere -> identity
    float embd_p, attn_p, resid_p;
    DropKey key;
    bool on() const { return embd_p > 0.f || attn_p > 0.f || resid_p > 0.f; }
};
static int drop_ctx(const r4d_train_dropout* dp, DropCtx& c) {
    c = DropCtx{0.f, 0.f, 0.f, DropKey{0, 0, 0, 0}};
    if (!dp) return R4D_OK;
    R4D_REQUIRE(dp->embd_p >= 0.f && dp->embd_p < 1.f && dp->attn_p >= 0.f && dp->attn_p < 1.f && dp->resid_p >= 0.f && dp->resid_p < 1.f,
                "gpt2 train: dropout probabilities must be in [0, 1)");
    c.embd_p = dp->embd_p; c.attn_p = dp->attn_p; c.resid_p = dp->resid_p;
    c.key = DropKey{(unsigned)dp->seed, (unsigned)(dp->seed >> 32), (unsigned)dp->step, (unsigned)(dp->step >> 32)};
    return R4D_OK;
}

// The per-head batched GEMMs of one batch [B, T]: T rows per (sequence, head), hd = d / H columns per head.  An operand is
// a pointer and a HeadLd: its leading dimension and its strides per sequence and per head.  Three kinds occur:
struct HeadLd { int ld; long long s0, s1; };
struct HeadDims {
    int B, T, H, d, hd, ld, Tp;                                   // ld = tpad128(T): row stride of a P-shaped block; Tp = up4(T)
    HeadLd qkv, merged, probs;                                    // a Q / K / V slice of [B, T, 3d]; [B, T, d]; [B*H, T, ld]
    HeadDims(int B_, int T_, int H_, int d_)
        : B(B_), T(T_), H(H_), d(d_), hd(d_ / H_), ld(tpad128(T_)), Tp(up4(T_)), qkv{3 * d_, (long long)T_ * 3 * d_, d_ / H_},
          merged{d_, (long long)T_ * d_, d_ / H_}, probs{ld, (long long)H_ * T_ * ld, (long long)T_ * ld} {}
};
// C[T, N] = epilogue(A[T, K] . B) per (sequence, head); B is [N, K] (b_trans) or [K, N], T valid rows either way
static GemmArgs head_gemm(const HeadDims& D, const float* A, HeadLd a, const float* Bm, HeadLd b, float* C, HeadLd c, int N, int K,
                          int b_trans, int a_cols, int epilogue = EPI_NONE, float scale_div = 1.f, int causal = CAUSAL_NONE) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = A; g.B = Bm; g.C = C;
    g.M = D.T; g.N = N; g.K = K; g.lda = a.ld; g.ldb = b.ld; g.ldc = c.ld;
    g.b_trans = b_trans; g.b_rows = D.T; g.a_cols = a_cols; g.nbatch = D.B * D.H; g.nb1 = D.H;
    g.sA0 = a.s0; g.sA1 = a.s1; g.sB0 = b.s0; g.sB1 = b.s1; g.sC0 = c.s0; g.sC1 = c.s1;
    g.epilogue = epilogue; g.scale_div = scale_div; g.causal = causal;
    return g;
}

// The six per-head products of a block's attention, forward and backward.  Operands are pointers to the first element of the
// (sequence 0, head 0) block: Q / K / V slices of [B, T, 3d], merged-heads [B, T, d] or P-shaped [B*H, T, ld] as listed.
enum HeadProduct {
    HP_S = 0,       // S  [probs]  = Q [qkv] . K [qkv]^T / sqrt(hd)    NT, K = hd, tiles above the diagonal skipped
    HP_PV,          // O  [merged] = P [probs] . V [qkv]               NN, K = T, trimmed to the keys a row tile sees
    HP_DP,          // dP [probs]  = dO [merged] . V [qkv]^T           NT, K = hd
    HP_DQ,          // dQ [qkv]    = dS [probs] . K [qkv]              NN, K = up4(T)
    HP_DK,          // dK [qkv]    = dS^T [probs] . Q [qkv]            NN, K = up4(T)
    HP_DV,          // dV [qkv]    = Pd^T [probs] . dO [merged]        NN, K = up4(T)
    HP_COUNT
};
static GemmArgs head_product_args(const HeadDims& D, int which, const float* A, const float* Bm, float* C) {
    switch (which) {
        case HP_S: return head_gemm(D, A, D.qkv, Bm, D.qkv, C, D.probs, D.T, D.hd, 1, 0, EPI_SCALE_DIV, (float)sqrt((double)D.hd), CAUSAL_QK);
        case HP_PV: return head_gemm(D, A, D.probs, Bm, D.qkv, C, D.merged, D.hd, D.T, 0, D.ld, EPI_NONE, 1.f, CAUSAL_PV);
        case HP_DP: return head_gemm(D, A, D.merged, Bm, D.qkv, C, D.probs, D.T, D.hd, 1, 0);
        case HP_DV: return head_gemm(D, A, D.probs, Bm, D.merged, C, D.qkv, D.hd, D.Tp, 0, D.Tp);
        default: return head_gemm(D, A, D.probs, Bm, D.qkv, C, D.qkv, D.hd, D.Tp, 0, D.Tp);          // HP_DQ, HP_DK
    }
}
// one of the six on the kernel the mode names: `abf` (TrainModes::attn_bf16) -> gemm_b1h, else the exact-f32 kernel
static int head_product(const HeadDims& D, int which, const float* A, const float* Bm, float* C, int abf, hipStream_t s) {
    const GemmArgs g = head_product_args(D, which, A, Bm, C);
    return abf ? launch_gemm_b1h(g, s) : launch_gemm_f32(g, s);
}

// P [B*H, T, ld] = causal softmax(Q . K^T / sqrt(hd)): the forward's two launches (recompute mode runs them again in the backward)
static int attn_probs(const HeadDims& D, const float* qkv, float* P, int abf, hipStream_t s) {
    const int rc = head_product(D, HP_S, qkv, qkv + D.d, P, abf, s);
    if (rc) return rc;
    return launch_causal_softmax(P, D.B * D.H, D.T, D.ld, D.ld, s);                // row_tile = ld: zero-fill the whole row
}

// Attention._attn forward over one batch, probabilities kept in P [B*H, T, ld] with EVERY column right of the diagonal zero
// `Pdrop` (with attn_p > 0): scratch for the dropped-out probabilities the P.V product reads; P keeps the softmax output
static int attn_fwd(const HeadDims& D, const float* qkv, float* P, float* out, int abf, hipStream_t s, float attn_p, DropKey key,
                    unsigned site, unsigned long long pbase, float* Pdrop) {
    int rc = attn_probs(D, qkv, P, abf, s);
    if (rc) return rc;
    const float* Pv = P;
    if (attn_p > 0.f) {                                                            // attn_dropout(w), modeling_gpt2.py:153
        if ((rc = launch_dropout(P, nullptr, (long long)D.B * D.H * D.T * D.ld, Pdrop, attn_p, key, site, pbase, s))) return rc;
        Pv = Pdrop;
    }
    return head_product(D, HP_PV, Pv, qkv + 2 * D.d, out, abf, s);
}

// Attention backward over one batch: dao [B,T,d] (merged heads) -> dqkv [B,T,3d].  `P`: the probabilities the forward kept, or
// nullptr (recompute mode): they are formed again into A by the forward's two launches, the same bits.  A (recompute mode
// only), Bs, C: scratch blocks of the batch's [B*H, T, ld] size.  The four GEMMs are the same launches in both modes; the
// element-wise steps between them are separate launches in stored mode and, in recompute mode, the two row kernels that merge them
// (`row_kernels`: launch_softmax_bwd_t, launch_dropout_transpose), written to leave those launches' bits (stored mode can take the
// row kernels over once they have been timed against it).  Neither mode is r4d_set_train_attention_fused: that one never gets here.
static int attn_bwd(const HeadDims& D, const float* qkv, const float* P, const float* dao, float* dqkv, float* A, float* Bs, float* C,
                    int abf, hipStream_t s, float attn_p, DropKey key, unsigned site, unsigned long long pbase) {
    const int d = D.d, BH = D.B * D.H;
    const long long n = (long long)BH * D.T * D.ld;
    const float sd = (float)sqrt((double)D.hd);                  // the logits were divided by sqrt(hd) before the softmax
    const bool row_kernels = P == nullptr;
    int rc;
    if (!P) {
        if ((rc = attn_probs(D, qkv, A, abf, s))) return rc;
        P = A;
    }
    // dP = dO . V^T
    if ((rc = head_product(D, HP_DP, dao, qkv + 2 * d, Bs, abf, s))) return rc;
    // dS in place on Bs (through the dropout mask: d(softmax out) = mask * dP / (1 - p)), dS^T into C
    if (row_kernels) {
        if ((rc = launch_softmax_bwd_t(P, Bs, C, BH, D.T, D.ld, sd, attn_p, key, site, pbase, s))) return rc;
    } else {
        if (attn_p > 0.f && (rc = launch_dropout(Bs, nullptr, n, Bs, attn_p, key, site, pbase, s))) return rc;
        if ((rc = launch_softmax_bwd(P, Bs, BH, D.T, D.ld, sd, s))) return rc;
    }
    // dQ = dS . K,  dK = dS^T . Q
    if ((rc = head_product(D, HP_DQ, Bs, qkv + d, dqkv, abf, s))) return rc;
    if (!row_kernels && (rc = launch_transpose(Bs, D.T, D.T, D.ld, D.probs.s1, C, D.ld, D.probs.s1, BH, s))) return rc;
    if ((rc = head_product(D, HP_DK, C, qkv, dqkv + d, abf, s))) return rc;
    // dV = Pd^T . dO: the probabilities the forward multiplied V with, after dropout, transposed into C (free once the dK GEMM
    // ahead in the stream has read it; Bs is free by now)
    if (row_kernels) {
        if ((rc = launch_dropout_transpose(P, C, BH, D.T, D.ld, attn_p, key, site, pbase, s))) return rc;
    } else {
        if (attn_p > 0.f && (rc = launch_dropout(P, nullptr, n, Bs, attn_p, key, site, pbase, s))) return rc;
        if ((rc = launch_transpose(attn_p > 0.f ? Bs : P, D.T, D.T, D.ld, D.probs.s1, C, D.ld, D.probs.s1, BH, s))) return rc;
    }
    return head_product(D, HP_DV, C, dao, dqkv + 2 * d, abf, s);
}

static RowGroups row_groups_of(const std::vector<TrainGroup>& gs) {
    RowGroups R;
    R.n = (int)gs.size();
    for (int j = 0; j < ATT_MAXG; ++j) {
        const bool in = j < R.n;
        R.B[j] = in ? gs[j].B : 0; R.T[j] = in ? gs[j].T : 0;
        R.ids[j] = in ? gs[j].ids : nullptr; R.emb[j] = nullptr;
    }
    return R;
}

}  // namespace r4d

using namespace r4d;

extern "C" {

size_t r4d_weight_grad_workspace_bytes(int32_t rows, int32_t in_features, int32_t out_features) {
    if (rows <= 0 || in_features <= 0 || out_features <= 0) return 0;
    return (gemm_tn_scratch_floats(in_features, out_features, rows) + colsum_scratch_floats(rows, out_features) + 64) * sizeof(float);
}

int r4d_weight_grad_f32(const float* x_d, const float* dy_d, int32_t rows, int32_t in_features, int32_t out_features, float* dw_d,
                        float* db_d, void* workspace_d, size_t workspace_bytes, void* stream) {
    R4D_REQUIRE(x_d && dy_d && dw_d && rows > 0 && in_features > 0 && out_features > 0, "weight_grad: bad arguments");
    R4D_REQUIRE(workspace_d && workspace_bytes >= r4d_weight_grad_workspace_bytes(rows, in_features, out_features),
                "weight_grad: workspace too small");
    float* skp = (float*)workspace_d;
    float* red = skp + (gemm_tn_scratch_floats(in_features, out_features, rows) + 63) / 64 * 64;
    return weight_grad(x_d, dy_d, dw_d, db_d, in_features, out_features, rows, in_features, out_features, skp, red, (hipStream_t)stream);
}

int r4d_set_train_attention(int32_t mode) { return set_mode(kTrainModes[TM_ATTENTION], mode); }
int r4d_get_train_attention(void) { return g_modes.attention; }
int r4d_set_train_activations(int32_t mode) { return set_mode(kTrainModes[TM_ACTIVATIONS], mode); }
int r4d_get_train_activations(void) { return g_modes.activations; }
int r4d_set_train_bf16(int32_t on) { return set_mode(kTrainModes[TM_BF16], on); }
int r4d_get_train_bf16(void) { return g_modes.bf16; }
int r4d_set_train_attention_bf16(int32_t on) { return set_mode(kTrainModes[TM_ATTN_BF16], on); }
int r4d_get_train_attention_bf16(void) { return g_modes.attn_bf16; }
int r4d_set_train_head_bf16(int32_t on) { return set_mode(kTrainModes[TM_HEAD_BF16], on); }
int r4d_get_train_head_bf16(void) { return g_modes.head_bf16; }
int r4d_set_train_act_bf16(int32_t on) { return set_mode(kTrainModes[TM_ACT_BF16], on); }
int r4d_get_train_act_bf16(void) { return g_modes.act_bf16; }
int r4d_set_train_attention_fused(int32_t on) { return set_mode(kTrainModes[TM_ATTN_FUSED], on); }
int r4d_get_train_attention_fused(void) { return g_modes.attn_fused; }

int r4d_train_attn_fused_fwd_f32(const float* qkv_d, int32_t B, int32_t T, int32_t H, int32_t d, float* att_out_d, float* lse_out_d,
                                 const r4d_train_dropout* dropout, uint32_t site, uint64_t index_base, void* stream) {
    DropCtx dc;
    const int rc = drop_ctx(dropout, dc);
    if (rc) return rc;
    return launch_attn_train_fused_fwd(qkv_d, B, T, H, d, att_out_d, lse_out_d, dc.attn_p, dc.key, site, index_base, (hipStream_t)stream);
}
size_t r4d_train_attn_fused_bwd_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t d) {
    return attn_train_fused_supported(B, T, H, d) ? (attn_train_fused_bwd_scratch_floats(B, T, H) + 64) * sizeof(float) : 0;
}
int r4d_train_attn_fused_bwd_f32(const float* qkv_d, const float* att_d, const float* lse_d, const float* dao_d, int32_t B, int32_t T,
                                 int32_t H, int32_t d, float* dqkv_out_d, const r4d_train_dropout* dropout, uint32_t site,
                                 uint64_t index_base, void* workspace_d, size_t workspace_bytes, void* stream) {
    DropCtx dc;
    const int rc = drop_ctx(dropout, dc);
    if (rc) return rc;
    R4D_REQUIRE(attn_train_fused_supported(B, T, H, d),
                "train_attn_fused_bwd: bad shape B=%d T=%d H=%d d=%d (head_dim %% 16 == 0 in 16 .. 256, T in 1 .. 1024, B * H <= 65535 wanted)", B, T, H, d);
    if (!workspace_d || workspace_bytes < r4d_train_attn_fused_bwd_workspace_bytes(B, T, H, d)) {
        set_error("train_attn_fused_bwd: workspace %zu bytes < required %zu", workspace_bytes, r4d_train_attn_fused_bwd_workspace_bytes(B, T, H, d));
        return R4D_ERR_WORKSPACE;
    }
    return launch_attn_train_fused_bwd(qkv_d, att_d, lse_d, dao_d, B, T, H, d, dqkv_out_d, (float*)workspace_d, dc.attn_p, dc.key, site,
                                       index_base, (hipStream_t)stream);
}

size_t r4d_train_attn_probs_ld(int32_t T) { return T > 0 ? (size_t)tpad128(T) : 0; }

int r4d_train_attn_product_bf16_f32(int32_t which, const float* a_d, const float* b_d, float* c_d, int32_t B, int32_t T, int32_t H,
                                    int32_t d, void* stream) {
    R4D_REQUIRE(which >= 0 && which < HP_COUNT, "train_attn_product_bf16: product %d not in 0 .. %d", (int)which, HP_COUNT - 1);
    R4D_REQUIRE(a_d && b_d && c_d, "train_attn_product_bf16: null pointer");
    R4D_REQUIRE(B >= 1 && T >= 1 && T <= 1024 && H >= 1 && d >= 1 && d % H == 0 && (d / H) % 16 == 0 && (long long)B * H <= 65535,
                "train_attn_product_bf16: bad shape B=%d T=%d H=%d d=%d (head_dim %% 16 == 0, T <= 1024, B * H <= 65535 wanted)", B, T, H, d);
    return launch_gemm_b1h(head_product_args(HeadDims(B, T, H, d), which, a_d, b_d, c_d), (hipStream_t)stream);
}

int r4d_conv1d_bf16_keep_f32(const float* x_d, const uint16_t* w_bf16_d, const float* bias_d, int32_t M, int32_t K, int32_t N,
                             float* pre_d, float* y_d, void* stream) {
    R4D_REQUIRE(pre_d && y_d && pre_d != y_d, "conv1d_bf16_keep: two output buffers wanted");
    return launch_gemm_b1(s3_args(x_d, w_bf16_d, bias_d, pre_d, M, K, N, EPI_GELU_KEEP, y_d), (hipStream_t)stream);
}

int r4d_conv1d_bf16_dgrad_f32(const float* dy_d, const uint16_t* wt_bf16_d, int32_t M, int32_t in_features, int32_t out_features,
                              int32_t kind, const float* second_d, float* dx_d, void* stream) {
    R4D_REQUIRE(kind >= 0 && kind <= 2, "conv1d_bf16_dgrad: kind %d not in {0 none, 1 residual, 2 gelu derivative}", kind);
    R4D_REQUIRE(kind == 0 || second_d, "conv1d_bf16_dgrad: kind %d needs the second buffer", kind);
    return launch_gemm_b1(s3_args(dy_d, wt_bf16_d, nullptr, kind ? second_d : nullptr, M, out_features, in_features,
                                  kind == 2 ? EPI_GELU_GRAD : kind == 1 ? EPI_RESIDUAL : EPI_NONE, dx_d), (hipStream_t)stream);
}

// workspace of the single op: the slices' dW partials (64-float aligned), behind them their db partials
static size_t wgrad_bf16_part_floats(int rows, int I, int J, int* S) {
    *S = gemm_tn_slices(I, J, rows, 64);
    return *S > 1 ? ((size_t)*S * I * J + 63) / 64 * 64 : 0;
}
size_t r4d_weight_grad_bf16_workspace_bytes(int32_t rows, int32_t in_features, int32_t out_features) {
    if (!gemm_b1tn_supported(in_features, out_features, rows, in_features, out_features)) return 0;
    int S;
    const size_t part = wgrad_bf16_part_floats(rows, in_features, out_features, &S);
    return (part + (S > 1 ? (size_t)S * out_features : 0) + 64) * sizeof(float);
}

int r4d_weight_grad_bf16_f32(const float* x_d, int32_t ldx, const float* dy_d, int32_t ldy, int32_t rows, int32_t in_features,
                             int32_t out_features, float* dw_d, float* db_d, void* workspace_d, size_t workspace_bytes, void* stream) {
    R4D_REQUIRE(x_d && dy_d && dw_d, "weight_grad_bf16: null pointer");
    R4D_REQUIRE(gemm_b1tn_supported(in_features, out_features, rows, ldx, ldy),
                "weight_grad_bf16: unsupported shape rows=%d in=%d out=%d ldx=%d ldy=%d (in %% 128 == 0, out %% 256 == 0, rows >= 32 wanted)",
                rows, in_features, out_features, ldx, ldy);
    R4D_REQUIRE(workspace_d && ((uintptr_t)workspace_d % 16) == 0 &&
                workspace_bytes >= r4d_weight_grad_bf16_workspace_bytes(rows, in_features, out_features), "weight_grad_bf16: workspace too small");
    R4D_REQUIRE(!db_d || ((uintptr_t)db_d % 16) == 0, "weight_grad_bf16: db must be 16-byte aligned");
    int S;
    const size_t part = wgrad_bf16_part_floats(rows, in_features, out_features, &S);
    float* ws = (float*)workspace_d;
    bool db_done = false;
    const int rc = wgrad_b1tn(x_d, dy_d, dw_d, db_d, in_features, out_features, rows, ldx, ldy, ws, part, ws + part,
                              S > 1 ? (size_t)S * out_features : 0, &db_done, (hipStream_t)stream);
    if (rc) return rc;
    R4D_REQUIRE(!db_d || db_done, "weight_grad_bf16: the bias gradient was not formed");
    return R4D_OK;
}

int r4d_weight_grad_bf16_act_f32(const uint16_t* x_bf16_d, int32_t ldx, const float* dy_d, int32_t ldy, int32_t rows, int32_t in_features,
                                 int32_t out_features, float* dw_d, float* db_d, void* workspace_d, size_t workspace_bytes, void* stream) {
    R4D_REQUIRE(x_bf16_d && dy_d && dw_d, "weight_grad_bf16_act: null pointer");
    R4D_REQUIRE(gemm_b1tn_supported(in_features, out_features, rows, ldx, ldy) && ldx % 8 == 0,
                "weight_grad_bf16_act: unsupported shape rows=%d in=%d out=%d ldx=%d ldy=%d (in %% 128 == 0, out %% 256 == 0, rows >= 32, ldx %% 8 == 0 wanted)",
                rows, in_features, out_features, ldx, ldy);
    R4D_REQUIRE(workspace_d && ((uintptr_t)workspace_d % 16) == 0 &&
                workspace_bytes >= r4d_weight_grad_bf16_workspace_bytes(rows, in_features, out_features), "weight_grad_bf16_act: workspace too small");
    R4D_REQUIRE(!db_d || ((uintptr_t)db_d % 16) == 0, "weight_grad_bf16_act: db must be 16-byte aligned");
    int S;
    const size_t part = wgrad_bf16_part_floats(rows, in_features, out_features, &S);
    float* ws = (float*)workspace_d;
    bool db_done = false;
    const int rc = wgrad_b1tn(reinterpret_cast<const float*>(x_bf16_d), dy_d, dw_d, db_d, in_features, out_features, rows, ldx, ldy, ws, part,
                              ws + part, S > 1 ? (size_t)S * out_features : 0, &db_done, (hipStream_t)stream, true);
    if (rc) return rc;
    R4D_REQUIRE(!db_d || db_done, "weight_grad_bf16_act: the bias gradient was not formed");
    return R4D_OK;
}

size_t r4d_gpt2_train_workspace_bytes(const r4d_gpt2_config* cfg, int32_t n_groups, const int32_t* Bs, const int32_t* Ts) {
    if (!cfg || n_groups <= 0 || n_groups > ATT_MAXG || !Bs || !Ts) return 0;
    for (int g = 0; g < n_groups; ++g)
        if (Bs[g] <= 0 || Ts[g] <= 0) return 0;
    const TrainModes md = train_modes();
    if (!train_modes_ok(md)) return 0;                            // train-attention-fused without train-attention-bf16
    return gpt2_train_workspace_floats(cfg, n_groups, Bs, Ts, md) * sizeof(float) + 256;
}

int r4d_gpt2_train_forward_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, int32_t n_groups,
                               const int64_t* const* ids_d, const int32_t* Bs, const int32_t* Ts, float* out_meanpool_d,
                               const r4d_train_dropout* dropout, void* workspace_d, size_t workspace_bytes, void* stream) {
    R4D_REQUIRE(out_meanpool_d, "gpt2 train: null pointer");
    return gpt2_train_forward(cfg, w, n_groups, ids_d, Bs, Ts, out_meanpool_d, nullptr, dropout, workspace_d, workspace_bytes, train_modes(),
                              (hipStream_t)stream);
}

int r4d_gpt2_train_backward_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_gpt2_grads* gr,
                                int32_t n_groups, const int64_t* const* ids_d, const int32_t* Bs, const int32_t* Ts,
                                const float* d_meanpool_d, const r4d_train_dropout* dropout, void* workspace_d,
                                size_t workspace_bytes, void* stream) {
    R4D_REQUIRE(d_meanpool_d, "gpt2 train backward: null pointer");
    return gpt2_train_backward(cfg, w, gr, n_groups, ids_d, Bs, Ts, d_meanpool_d, nullptr, dropout, workspace_d, workspace_bytes, train_modes(),
                               (hipStream_t)stream);
}

}  // extern "C"

namespace r4d {

size_t gpt2_train_workspace_floats(const r4d_gpt2_config* cfg, int n_groups, const int32_t* Bs, const int32_t* Ts, TrainModes md) {
    std::vector<TrainGroup> gs((size_t)n_groups);
    for (int g = 0; g < n_groups; ++g) gs[g] = TrainGroup{nullptr, Bs[g], Ts[g], 0, 0, 0};
    return layout(cfg, gs.data(), n_groups, md).total;
}

// One block of the training forward: x_in[l] -> x_in[l + 1] (x_out behind the last one), layer 0 from the token ids.
// `again` (activations recompute mode, called by the backward): x_in[l] is there; the launches from ln_1 to c_fc (+ GELU) run on
// it once more with the forward's arguments and dropout sites, into the set all layers share, and the MLP projection is left out.
// It borrows the backward temporaries dy (branch of the residual dropout) and dP / pA (attention scratch) like the forward.
static int layer_forward(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, int l, const TrainLayout& t,
                         const std::vector<TrainGroup>& gs, const RowGroups& R, const DropCtx& dc, float* ws,
                         const int64_t* const* ids_d, const int32_t* Bs, const int32_t* Ts, const SpliceIn* sp, bool again,
                         TrainModes md, hipStream_t s) {
    const int bf16 = md.bf16;
    const int d = cfg->n_embd, H = cfg->n_head, M = (int)t.M;
    const r4d_gpt2_layer& Lw = w->layers[l];
    R4D_REQUIRE(Lw.ln_1_w && Lw.c_attn_w && Lw.attn_proj_w && Lw.ln_2_w && Lw.c_fc_w && Lw.mlp_proj_w, "gpt2 train: null weight in layer %d", l);
    const Conv1DW Wqkv = conv1d_w(Lw, C_ATTN, d), Wo = conv1d_w(Lw, ATTN_PROJ, d), Wfc = conv1d_w(Lw, C_FC, d), Wp = conv1d_w(Lw, MLP_PROJ, d);
    const Conv1DOpts fwd{nullptr, false, bf16 ? BF16_TRAIN : BF16_OFF};
    // the blocks kept as bf16 (r4d_set_train_act_bf16; the layout's own rule): their consumers read a bf16 A operand
    const bool ln1_bf = t.bf(ACT_LN1, l), ln2_bf = t.bf(ACT_LN2, l), f_bf = t.bf(ACT_F, l);
    Conv1DOpts fwd_ln1 = fwd, fwd_ln2 = fwd, fwd_f = fwd;
    fwd_ln1.x_bf16 = ln1_bf; fwd_ln2.x_bf16 = ln2_bf; fwd_f.x_bf16 = f_bf;
    R4D_REQUIRE(!ln1_bf || Lw.c_attn_w3, "gpt2 train: train-act-bf16 keeps layer %d's ln1 as bf16, but the layer carries no c_attn_w3 planes", l);
    R4D_REQUIRE(!ln2_bf || Lw.c_fc_w3, "gpt2 train: train-act-bf16 keeps layer %d's ln2 as bf16, but the layer carries no c_fc_w3 planes", l);
    R4D_REQUIRE(!f_bf || Lw.mlp_proj_w3, "gpt2 train: train-act-bf16 keeps layer %d's f as bf16, but the layer carries no mlp_proj_w3 planes", l);
    float *x_in = ws + t.x_in[l], *ln1 = ws + t.ln1[l], *qkv = ws + t.qkv[l], *att = ws + t.att[l];
    float *x_mid = ws + t.x_mid[l], *ln2 = ws + t.ln2[l], *pre = ws + t.pre[l], *f = ws + t.f[l];
    int rc = R4D_OK;
    if (l == 0 && again)                                         // x_in (after its dropout) and its ln1 are layer 0's own blocks:
        rc = R4D_OK;                                             // kept, not formed again (the fused kernels below made them)
    else if (l == 0 && sp)                                       // cat(wte[tok[:, :2]], fused, wte[tok[:, 2:]]) + wpe
        rc = launch_splice_embed_ln(ids_d[0], sp->fused, sp->r, w->wte, w->wpe, cfg->vocab, Bs[0], Ts[0], d, Lw.ln_1_w, Lw.ln_1_b,
                                    cfg->ln_eps, x_in, ln1, s);
    else if (l == 0)
        rc = launch_embed_layernorm_groups(R, w->wte, w->wpe, cfg->vocab, d, Lw.ln_1_w, Lw.ln_1_b, cfg->ln_eps, x_in, ln1, s);
    else if (ln1_bf)
        rc = launch_layernorm_bf16(x_in, Lw.ln_1_w, Lw.ln_1_b, M, d, cfg->ln_eps, (unsigned short*)ln1, s);
    else
        rc = launch_layernorm(x_in, Lw.ln_1_w, Lw.ln_1_b, M, d, cfg->ln_eps, ln1, s);
    if (rc) return rc;
    if (l == 0 && !again && dc.embd_p > 0.f) {                   // self.drop(inputs_embeds + position_embeds), :427
        if ((rc = launch_dropout(x_in, nullptr, (long long)M * d, x_in, dc.embd_p, dc.key, R4D_DROPOUT_SITE_EMBD, 0, s))) return rc;
        if ((rc = launch_layernorm(x_in, Lw.ln_1_w, Lw.ln_1_b, M, d, cfg->ln_eps, ln1, s))) return rc;
    }
    if ((rc = conv1d(Wqkv, ln1, nullptr, M, EPI_NONE, qkv, s, fwd_ln1))) return rc;
    for (const TrainGroup& G : gs) {
        if (t.fused)                                             // (row0 H: the group's first (sequence, head, query) of lse [M H])
            rc = launch_attn_train_fused_fwd(qkv + G.row0 * 3 * d, G.B, G.T, H, d, att + G.row0 * d, ws + t.lse[l] + G.row0 * H, dc.attn_p,
                                             dc.key, 4u * l + 0u, G.p0, s);
        else
            rc = attn_fwd(HeadDims(G.B, G.T, H, d), qkv + G.row0 * 3 * d, t.recompute ? ws + t.pA : ws + t.P[l] + G.p0,
                          att + G.row0 * d, md.attn_bf16, s, dc.attn_p, dc.key, 4u * l + 0u, G.p0, ws + t.dP);
        if (rc) return rc;
    }
    float* branch = ws + t.dy;                                   // a backward temporary, free during the forward
    if (dc.resid_p > 0.f) {                                      // x + resid_dropout(c_proj(a)), :194,229
        if ((rc = conv1d(Wo, att, nullptr, M, EPI_NONE, branch, s, fwd))) return rc;
        if ((rc = launch_dropout(branch, x_in, (long long)M * d, x_mid, dc.resid_p, dc.key, 4u * l + 1u, 0, s))) return rc;
    } else if ((rc = conv1d(Wo, att, x_in, M, EPI_RESIDUAL, x_mid, s, fwd))) return rc;
    if ((rc = ln2_bf ? launch_layernorm_bf16(x_mid, Lw.ln_2_w, Lw.ln_2_b, M, d, cfg->ln_eps, (unsigned short*)ln2, s)
                     : launch_layernorm(x_mid, Lw.ln_2_w, Lw.ln_2_b, M, d, cfg->ln_eps, ln2, s))) return rc;
    if (train_fuse_gelu() && conv1d_fuses_gelu_keep(Wfc, M, fwd.bf16)) {
        // one launch: f = gelu_new(v) and the pre-activation v (kept for the backward pass) both leave the GEMM's epilogue
        if ((rc = conv1d(Wfc, ln2, pre, M, f_bf ? EPI_GELU_KEEP_BF16 : EPI_GELU_KEEP, f, s, fwd_ln2))) return rc;
    } else {
        if ((rc = conv1d(Wfc, ln2, nullptr, M, EPI_NONE, pre, s, fwd_ln2))) return rc;
        if ((rc = f_bf ? launch_gelu_fwd_bf16(pre, (long long)M * 4 * d, (unsigned short*)f, s)
                       : launch_gelu_fwd(pre, (long long)M * 4 * d, f, s))) return rc;
    }
    if (again) return R4D_OK;                                    // the MLP projection's output, x_in[l + 1], is there already
    float* x_next = l + 1 < cfg->n_layer ? ws + t.x_in[l + 1] : ws + t.x_out;
    if (dc.resid_p > 0.f) {                                      // x + dropout(c_proj(act(c_fc(x)))), :212,233
        if ((rc = conv1d(Wp, f, nullptr, M, EPI_NONE, branch, s, fwd_f))) return rc;
        if ((rc = launch_dropout(branch, x_mid, (long long)M * d, x_next, dc.resid_p, dc.key, 4u * l + 2u, 0, s))) return rc;
    } else if ((rc = conv1d(Wp, f, x_mid, M, EPI_RESIDUAL, x_next, s, fwd_f))) return rc;
    return R4D_OK;
}

// The training forward; its output is EITHER the mean pool per sequence (retriever) OR the ln_f output per row (LM head)
int gpt2_train_forward(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, int n_groups, const int64_t* const* ids_d,
                       const int32_t* Bs, const int32_t* Ts, float* out_meanpool_d, float* out_hidden_d,
                       const r4d_train_dropout* dropout, void* workspace_d, size_t workspace_bytes, TrainModes md, hipStream_t s,
                       const SpliceIn* sp) {
    R4D_REQUIRE(train_modes_ok(md), "gpt2 train: train-attention-fused needs train-attention-bf16 (a '+attn' precision)");
    std::vector<TrainGroup> gs;
    int rc = check_groups(cfg, n_groups, ids_d, Bs, Ts, gs);
    if (rc) return rc;
    R4D_REQUIRE(!sp || n_groups == 1, "gpt2 train: a spliced input is one batch");
    DropCtx dc;
    if ((rc = drop_ctx(dropout, dc))) return rc;
    R4D_REQUIRE(w && w->wte && w->wpe && w->ln_f_w && w->ln_f_b && w->layers && (out_meanpool_d || out_hidden_d), "gpt2 train: null pointer");
    const TrainLayout t = layout(cfg, gs.data(), n_groups, md);
    if (!workspace_d || workspace_bytes < t.total * sizeof(float)) {
        set_error("gpt2 train: workspace %zu bytes < required %zu", workspace_bytes, t.total * sizeof(float));
        return R4D_ERR_WORKSPACE;
    }
    float* ws = (float*)workspace_d;
    g_last_fwd.ws = workspace_d; g_last_fwd.modes = md; g_last_fwd.shared_layer = cfg->n_layer - 1;
    const int d = cfg->n_embd;
    const RowGroups R = row_groups_of(gs);
    for (int l = 0; l < cfg->n_layer; ++l)
        if ((rc = layer_forward(cfg, w, l, t, gs, R, dc, ws, ids_d, Bs, Ts, sp, false, md, s))) return rc;
    return launch_lnf_meanpool_groups(R, ws + t.x_out, w->ln_f_w, w->ln_f_b, d, cfg->ln_eps, out_hidden_d, out_meanpool_d,
                                      ws + t.pool_scratch, s);
}

// Backward of gpt2_train_forward from EITHER d(mean pool) [sum B, d] OR d(ln_f output) [rows, d]
int gpt2_train_backward(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_gpt2_grads* gr, int n_groups,
                        const int64_t* const* ids_d, const int32_t* Bs, const int32_t* Ts, const float* d_meanpool_d,
                        const float* d_hidden_d, const r4d_train_dropout* dropout, void* workspace_d, size_t workspace_bytes,
                        TrainModes md, hipStream_t s, const SpliceIn* sp, float* d_fused) {
    R4D_REQUIRE(train_modes_ok(md), "gpt2 train backward: train-attention-fused needs train-attention-bf16 (a '+attn' precision)");
    std::vector<TrainGroup> gs;
    int rc = check_groups(cfg, n_groups, ids_d, Bs, Ts, gs);
    if (rc) return rc;
    DropCtx dc;
    if ((rc = drop_ctx(dropout, dc))) return rc;
    R4D_REQUIRE(w && w->layers && (d_meanpool_d || d_hidden_d) && (!sp || n_groups == 1) && (!d_fused || sp) &&
                (gr ? gr->layers && gr->wte && gr->wpe && gr->ln_f_w && gr->ln_f_b : d_fused != nullptr),
                "gpt2 train backward: null pointer");
    const bool after_fwd = workspace_d == g_last_fwd.ws;             // the workspace of the most recent forward
    for (const TrainModeRow& row : kTrainModes)
        R4D_REQUIRE(!after_fwd || !row.guarded || md.*row.field == g_last_fwd.modes.*row.field,
                    "gpt2 train backward: this workspace was filled by a forward with %s %d, the current value is %d", row.name,
                    g_last_fwd.modes.*row.field, md.*row.field);
    const TrainLayout t = layout(cfg, gs.data(), n_groups, md);
    if (!workspace_d || workspace_bytes < t.total * sizeof(float)) {
        set_error("gpt2 train backward: workspace %zu bytes < required %zu", workspace_bytes, t.total * sizeof(float));
        return R4D_ERR_WORKSPACE;
    }
    float* ws = (float*)workspace_d;
    const int d = cfg->n_embd, H = cfg->n_head, M = (int)t.M, L = cfg->n_layer;
    float *dx = ws + t.dx, *dy = ws + t.dy, *dbig = ws + t.dbig, *dqkv = ws + t.dqkv, *xT = ws + t.xT, *red = ws + t.red;
    const RowGroups R = row_groups_of(gs);
    // mean over T -> ln_f (or the caller's per-row gradient of the ln_f output)
    if (d_meanpool_d) {
        for (const TrainGroup& G : gs)
            if ((rc = launch_meanpool_bwd(d_meanpool_d + G.seq0 * d, (long long)G.B * G.T, G.T, d, dy + G.row0 * d, s))) return rc;
    }
    const float* dlnf = d_meanpool_d ? dy : d_hidden_d;
    const bool frozen = gr == nullptr;                               // data gradients only (RAG generator under --freeze)
    if ((rc = launch_ln_bwd(ws + t.x_out, w->ln_f_w, dlnf, nullptr, M, d, cfg->ln_eps, dx, frozen ? nullptr : gr->ln_f_w,
                            frozen ? nullptr : gr->ln_f_b, red, 0, s))) return rc;
    for (int l = L - 1; l >= 0; --l) {
        const r4d_gpt2_layer& Lw = w->layers[l];
        static const r4d_gpt2_layer_grads kNone{};
        const r4d_gpt2_layer_grads& Lg = frozen ? kNone : gr->layers[l];
        R4D_REQUIRE(frozen || Lg.ln_1_w && Lg.ln_1_b && Lg.c_attn_w && Lg.c_attn_b && Lg.attn_proj_w && Lg.attn_proj_b && Lg.ln_2_w &&
                    Lg.ln_2_b && Lg.c_fc_w && Lg.c_fc_b && Lg.mlp_proj_w && Lg.mlp_proj_b, "gpt2 train backward: null gradient in layer %d", l);
        const Conv1DW Wqkv = conv1d_w(Lw, C_ATTN, d), Wo = conv1d_w(Lw, ATTN_PROJ, d), Wfc = conv1d_w(Lw, C_FC, d), Wp = conv1d_w(Lw, MLP_PROJ, d);
        float *x_in = ws + t.x_in[l], *ln1 = ws + t.ln1[l], *qkv = ws + t.qkv[l], *att = ws + t.att[l];
        float *x_mid = ws + t.x_mid[l], *ln2 = ws + t.ln2[l], *pre = ws + t.pre[l], *f = ws + t.f[l];
        // activations recompute: this layer's ln1 .. f (and P) into the shared set again, by the forward's launches on x_in[l].
        // dx holds the live d(x_out) and is not touched; dy, dP and pA, which the launches borrow, are dead here.  The set still
        // holds the last layer's activations when this backward follows its forward directly: nothing to run again then.
        if (t.act_recompute && !(after_fwd && g_last_fwd.shared_layer == l)) {
            if (after_fwd) g_last_fwd.shared_layer = -1;
            if ((rc = layer_forward(cfg, w, l, t, gs, R, dc, ws, ids_d, Bs, Ts, sp, true, md, s))) return rc;
            if (after_fwd) g_last_fwd.shared_layer = l;
        }
        // ---- MLP: x_out = x_mid + gelu(ln_2(x_mid) Wfc + bfc) Wp + bp ;  dx holds d(x_out)
        const float* dbr = dx;                                       // gradient of the branch output: through its dropout mask
        if (dc.resid_p > 0.f) {
            if ((rc = launch_dropout(dx, nullptr, (long long)M * d, dy, dc.resid_p, dc.key, 4u * l + 2u, 0, s))) return rc;
            dbr = dy;
        }
        if (!frozen && (rc = weight_grad(f, dbr, Lg.mlp_proj_w, Lg.mlp_proj_b, 4 * d, d, M, 4 * d, d, xT, red, s, md.bf16, t.bf(ACT_F, l)))) return rc;
        if (train_fuse_gelu() && dgrad_route(Wp, M, md.bf16) != ROUTE_DGRAD_F32) {
            // d(pre) = (d(branch) . Wp^T) * gelu_new'(pre): the derivative is applied in the GEMM's epilogue
            if ((rc = data_grad(Wp, dbr, M, dbig, nullptr, pre, s, md.bf16))) return rc;
        } else {
            if ((rc = data_grad(Wp, dbr, M, dbig, nullptr, nullptr, s, md.bf16))) return rc;                  // d(f)
            if ((rc = launch_gelu_bwd(pre, dbig, (long long)M * 4 * d, dbig, s))) return rc;              // d(pre), in place
        }
        if (!frozen && (rc = weight_grad(ln2, dbig, Lg.c_fc_w, Lg.c_fc_b, d, 4 * d, M, d, 4 * d, xT, red, s, md.bf16, t.bf(ACT_LN2, l)))) return rc;
        if ((rc = data_grad(Wfc, dbig, M, dy, nullptr, nullptr, s, md.bf16))) return rc;                      // d(ln_2 out)
        if ((rc = launch_ln_bwd(x_mid, Lw.ln_2_w, dy, dx, M, d, cfg->ln_eps, dx, Lg.ln_2_w, Lg.ln_2_b, red, 0, s))) return rc;   // dx = d(x_mid)
        // ---- attention: x_mid = x_in + attn(ln_1(x_in)) Wo + bo
        dbr = dx;
        if (dc.resid_p > 0.f) {                                      // dbig (M x 4d) is free here
            if ((rc = launch_dropout(dx, nullptr, (long long)M * d, dbig, dc.resid_p, dc.key, 4u * l + 1u, 0, s))) return rc;
            dbr = dbig;
        }
        if (!frozen && (rc = weight_grad(att, dbr, Lg.attn_proj_w, Lg.attn_proj_b, d, d, M, d, d, xT, red, s, md.bf16))) return rc;
        if ((rc = data_grad(Wo, dbr, M, dy, nullptr, nullptr, s, md.bf16))) return rc;                        // d(att), merged heads
        for (const TrainGroup& G : gs) {                             // stored mode: the kept P, and no block A (pA does not exist)
            if (t.fused)
                rc = launch_attn_train_fused_bwd(qkv + G.row0 * 3 * d, att + G.row0 * d, ws + t.lse[l] + G.row0 * H, dy + G.row0 * d, G.B, G.T,
                                                 H, d, dqkv + G.row0 * 3 * d, ws + t.attD + G.row0 * H, dc.attn_p, dc.key, 4u * l + 0u, G.p0, s);
            else
                rc = attn_bwd(HeadDims(G.B, G.T, H, d), qkv + G.row0 * 3 * d, t.recompute ? nullptr : ws + t.P[l] + G.p0,
                              dy + G.row0 * d, dqkv + G.row0 * 3 * d, t.recompute ? ws + t.pA : nullptr, ws + t.dP, ws + t.PT, md.attn_bf16, s,
                              dc.attn_p, dc.key, 4u * l + 0u, G.p0);
            if (rc) return rc;
        }
        if (!frozen && (rc = weight_grad(ln1, dqkv, Lg.c_attn_w, Lg.c_attn_b, d, 3 * d, M, d, 3 * d, xT, red, s, md.bf16, t.bf(ACT_LN1, l)))) return rc;
        if ((rc = data_grad(Wqkv, dqkv, M, dy, nullptr, nullptr, s, md.bf16))) return rc;                     // d(ln_1 out)
        if ((rc = launch_ln_bwd(x_in, Lw.ln_1_w, dy, dx, M, d, cfg->ln_eps, dx, Lg.ln_1_w, Lg.ln_1_b, red, 0, s))) return rc;    // dx = d(x_in)
    }
    // embeddings: x_in[0] = drop(wte[ids] + wpe[0..T-1])
    if (dc.embd_p > 0.f && (rc = launch_dropout(dx, nullptr, (long long)M * d, dx, dc.embd_p, dc.key, R4D_DROPOUT_SITE_EMBD, 0, s)))
        return rc;
    if (d_fused)                                                     // rows 2 .. 2 + r - 1 of every spliced sequence
        R4D_HIP(hipMemcpy2DAsync(d_fused, (size_t)sp->r * d * sizeof(float), dx + 2 * (size_t)d, (size_t)gs[0].T * d * sizeof(float),
                                 (size_t)sp->r * d * sizeof(float), (size_t)gs[0].B, hipMemcpyDeviceToDevice, s));
    if (frozen) return R4D_OK;
    // deterministic sums (train_ops.hip): tokens through a 64-bit fixed-point table (negative ids -- the spliced rows -- add
    // nothing), positions as ordered column sums
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(ws + t.emb_acc);
    R4D_HIP(hipMemsetAsync(acc, 0, ((size_t)cfg->vocab * d + 2) * sizeof(unsigned long long), s));       // table + poison word + max word
    R4D_HIP(hipMemsetAsync(gr->wpe, 0, (size_t)cfg->n_positions * d * sizeof(float), s));
    if ((rc = launch_embedding_absmax(dx, (long long)M * d, acc, (long long)cfg->vocab * d, s))) return rc;      // the scale follows the data
    for (const TrainGroup& G : gs)
        if ((rc = launch_embedding_bwd(dx + G.row0 * d, G.ids, G.B, G.T, d, cfg->vocab, acc, gr->wpe, 0, (long long)M, s))) return rc;
    return launch_embedding_fix_to_f32(acc, (long long)cfg->vocab * d, (long long)M, gr->wte, s);
}

}  // namespace r4d
