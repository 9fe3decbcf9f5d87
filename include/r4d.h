/*
 * r4d.h -- C ABI of librag4dyg_hip.so: the MI355X (gfx950) encode-and-retrieve hot path of RAG4DyG.
 *
 * The reference (YuxiaWu/RAG4DyG) is 100 % Python and has no FFI/plugin layer;
 * each entry point below cites the reference Python call surface it replaces.  Conventions:
 *   - extern "C", plain pointers and sizes, no torch / C++ types;
 *   - every pointer named *_d / documented "device" is a caller-owned HBM pointer (e.g. torch
 *     tensor.data_ptr()); the library never allocates device memory: scratch comes from an explicit
 *     caller-provided workspace whose size is returned by the matching *_workspace_bytes query;
 *   - kernels are enqueued on the caller's stream (a hipStream_t passed as void*; NULL = default
 *     stream) and the call returns without synchronising (graph-capturable);
 *   - return value: 0 = R4D_OK, negative = error; the message is available from r4d_last_error()
 *     (thread-local).  No exceptions cross the ABI;
 *   - all floating-point data is fp32 (the reference computes in fp32), Jaccard ratios are f64
 *     (python floats), indices are int32 / int64 as stated;
 *   - PROCESS MODEL: one process drives ONE device (one process per GPU, torch.distributed over RCCL between them).  A few
 *     launch parameters are latched per process the first time a kernel family runs (occupancy of the scan kernels, the
 *     > 64 KB dynamic-LDS attribute of the LDS-DMA scan forms, the persistent GEMM's ticket slots), i.e. for the device that was
 *     current then; a process that switched devices afterwards would get R4D_ERR_HIP from the first such launch on the second
 *     device (loud, never a wrong result).  The arithmetic switches (r4d_set_gemm_split3, r4d_set_attention_fused) are
 *     process-wide too: the ranks of a sharded job must select the same Conv1D arithmetic, or the merged per-shard top-k differs
 *     from the one-GPU result in the last bits of the scores.
 */
#ifndef R4D_H
#define R4D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define R4D_OK 0
#define R4D_ERR_INVALID (-1)      /* bad argument / unsupported shape */
#define R4D_ERR_HIP (-2)          /* a HIP runtime call or kernel launch failed */
#define R4D_ERR_WORKSPACE (-3)    /* workspace too small */

#define R4D_ABI_VERSION 6

/* ABI version of the loaded library. */
int r4d_abi_version(void);
/* 0 for a product build.  Non-zero when the library was compiled with one of the kernel-ablation macros of
 * tools/kc_ablate.sh (bit 0 KC_DBG, bit 1 ATT_DBG, bit 2 SK_DBG, bit 3 JAC_DBG, bit 4 SCAN_DBG, bit 5 S3_DBG, bit 6 H2_DBG): such a build
 * computes WRONG results by construction and the Python binding refuses to load it outside tools/. */
int r4d_build_flags(void);
/* Message of the last failing call on this thread ("" if none). */
const char* r4d_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * GPT-2 encoder (SimpleDyG backbone).
 * Replaces GPT2Model.forward  models/modeling_gpt2.py:357-509 (== models/modeling_rag.py:412-564)
 * and its callees Block :224-235, Attention :140-197, MLP :209-212, Conv1D modeling_utils.py:1267-1271,
 * plus the retriever's mean-pool  train/train_retriever.py:419-420,430-432.
 * Weight pointers use the reference checkpoint layout (Conv1D weights are [in,out]).
 * ---------------------------------------------------------------------------------------------- */
typedef struct r4d_gpt2_config {
    int32_t n_layer;
    int32_t n_head;
    int32_t n_embd;        /* d; d % 64 == 0, (d / n_head) % 16 == 0 */
    int32_t vocab;         /* rows of wte (len(tokenizer) after resize_token_embeddings) */
    int32_t n_positions;   /* rows of wpe (1024) */
    float   ln_eps;        /* layer_norm_epsilon (1e-5) */
} r4d_gpt2_config;

typedef struct r4d_gpt2_layer {   /* device pointers, one struct per transformer.h.<i> */
    const float* ln_1_w;      const float* ln_1_b;        /* [d] */
    const float* c_attn_w;    const float* c_attn_b;      /* [d,3d], [3d] */
    const float* attn_proj_w; const float* attn_proj_b;   /* [d,d],  [d]  */
    const float* ln_2_w;      const float* ln_2_b;        /* [d] */
    const float* c_fc_w;      const float* c_fc_b;        /* [d,4d], [4d] */
    const float* mlp_proj_w;  const float* mlp_proj_b;    /* [4d,d], [d]  */
    /* OPTIONAL transposed copies of the four static Conv1D weights ([out,in] row-major, i.e. K contiguous), made
     * once by the host when the checkpoint is loaded; NULL = not provided.  With them every GEMM operand is
     * k-contiguous and the faster b128-LDS kernel runs (same values up to fp32 summation order). */
    const float* c_attn_wT;   const float* attn_proj_wT;  /* [3d,d], [d,d]  */
    const float* c_fc_wT;     const float* mlp_proj_wT;   /* [4d,d], [d,4d] */
    /* OPTIONAL bf16x3 planes of the same four weights (r4d_split3_planes_bf16: uint16 [3][out][in], hi / mid / lo), made
     * once per checkpoint; NULL = not provided.  With them (and r4d_set_gemm_split3 != 0, the default) the four Conv1D
     * GEMMs of a block run on the bf16 matrix cores at fp32 accuracy (r4d_conv1d_s3_f32) in the encoder calls (the cached
     * decode step keeps its weight-stream kernels); everything else about the call is unchanged. */
    const uint16_t* c_attn_w3;  const uint16_t* attn_proj_w3;
    const uint16_t* c_fc_w3;    const uint16_t* mlp_proj_w3;
    /* TRAINING only, optional: the planes of the same weights as the operand of the data-gradient GEMMs dx = dy . W^T
     * (r4d_split3_planes_bf16(w, K = out, N = in, transposed = 1): uint16 [3][in][out]); NULL = exact-f32 kernel.  Like the
     * wT copies, every plane set must be refreshed by the caller after each optimizer step. */
    const uint16_t* c_attn_w3t; const uint16_t* attn_proj_w3t;
    const uint16_t* c_fc_w3t;   const uint16_t* mlp_proj_w3t;
    /* DECODE only, optional (ABI v4): LayerNorm pre-folded into the two projections that read it (r4d_fold_layernorm_f32 on
     * c_attn_wT with ln_1, on c_fc_wT with ln_2): *_wTg [out,in] = gain[in] * W^T, *_lnc [2][out] = (sum_in gain W, sum_in shift W).
     * With them the cached decode step (d in {512, 768}, batch <= 32) evaluates LN(x) W as rstd (x W'^T - mean c1) + c2 without
     * loading the gain / shift or forming c1 / c2 per launch; NULL = it forms them from ln_1 / ln_2 and *_wT as before. */
    const float* c_attn_wTg;    const float* c_attn_lnc;
    const float* c_fc_wTg;      const float* c_fc_lnc;
    /* OPTIONAL f16x2 planes of the four weights (ABI v5; r4d_split2_planes_f16: uint16 [out][in/32][2][32], hi and 2^11-scaled lo
     * as fp16), made once per checkpoint; NULL = not provided.  With them and r4d_set_gemm_split3(2) the four Conv1D GEMMs of a
     * block run on the fp16 matrix cores with THREE products per fp32 product at fp32 accuracy (r4d_conv1d_h2_f32; csrc/gemm_h2.hip
     * for the error analysis and the operand range: |activation| < 2^18, |weight| < 6e4). */
    const uint16_t* c_attn_h2;  const uint16_t* attn_proj_h2;
    const uint16_t* c_fc_h2;    const uint16_t* mlp_proj_h2;
    /* (ABI v6: r4d_gpt2_train_forward_f32 uses the *_h2 planes too in mode 2 -- the FORWARD GEMMs of a training step on the fp16
     * matrix cores; every gradient GEMM keeps bf16x3: a gradient operand needs fp32's exponent range.  Refreshed by the caller
     * after each optimizer step, like every plane set.) */
} r4d_gpt2_layer;

typedef struct r4d_gpt2_weights {
    const float* wte;                /* device [vocab,d]  transformer.wte.weight */
    const float* wpe;                /* device [n_positions,d] */
    const float* ln_f_w;             /* device [d] */
    const float* ln_f_b;
    const r4d_gpt2_layer* layers;    /* HOST array [n_layer] of device-pointer structs */
    const float* lm_head;            /* device [vocab,d] lm_head.weight, or NULL when it is tied to wte
                                      * (modeling_utils.py:155-181).  The reference UNTIES the two whenever it replaces
                                      * transformer.wte or model.transformer without re-tying (hepth node-feature injection,
                                      * utils/tokenizer.py:56-66; load_and_freeze_params, utils/model.py:71-78), so trained
                                      * generator checkpoints carry two different tensors.  Read by the greedy step only. */
} r4d_gpt2_weights;

/*
 * WHAT A BUFFER MAY HOLD ON ENTRY (every entry point of this header).
 * Workspace (workspace_d / *_ws_d), output (out_*_d, loss_d, perm_d, ...) and gradient memory (r4d_gpt2_grads, head_grad_d,
 * d_fused_d, dw_d / db_d / dx_d) may hold ANYTHING when a call is made -- stale values of another shape or another entry point,
 * NaN, huge values, non-zero counters: the library never needs such memory zeroed, writes every byte it later reads (padding of
 * contraction ranges, split-K and top-k ticket counters, fixed-point accumulation tables included: each call clears or
 * overwrites its own), and one workspace may be shared, grow-only, by any sequence of calls on one stream.  Gradients are
 * OVERWRITTEN, never accumulated into.  tests/test_gpu_workspace_poison.py runs every entry point on memory filled with NaN
 * bytes, 0x7F bytes and the word 1 and asserts the bits of a run on zeroed memory.
 * The exceptions are caller STATE, which a call reads as documented at its entry:
 *   - the key/value cache rows BELOW pos (r4d_gpt2_decode_step_f32, the greedy entries); rows at and past pos are never read;
 *   - the optimizer's m / v and sumsq[0] (r4d_adamw_step_f32, r4d_sumsq_accumulate_f32; sumsq[1..] is scratch);
 *   - a training workspace BETWEEN r4d_gpt2_train_forward*_f32 and the backward of the same step (the saved activations);
 *   - operands described as zero-padded by their entry (the rows of r4d_lm_head.wte_pad past vocab);
 *   - the sticky range-guard word (r4d_set_range_flag) and the greedy loop state (r4d_greedy_state);
 *   - the sampled loop state (r4d_sample_state) and the seen bitmap of r4d_sample_logits_f32;
 *   - the beam loop state (r4d_beam_state: the fields marked in/out; its candidate and hypothesis buffers are scratch until written).
 */

/* Scratch bytes r4d_gpt2_encode_f32 needs for a [B,T] batch. */
size_t r4d_gpt2_workspace_bytes(const r4d_gpt2_config* cfg, int32_t B, int32_t T);

/*
 * One encoder forward over a right-padded batch.
 *   ids_d           device int64 [B,T] token ids, or NULL when inputs_embeds_d is given
 *   inputs_embeds_d device f32 [B,T,d] (generator-style call, modeling_rag.py:460-461,517-524) or NULL
 *   out_hidden_d    device f32 [B,T,d]  ln_f output ("hidden_states"), or NULL
 *   out_meanpool_d  device f32 [B,d]    mean over ALL T padded positions (train_retriever.py:420), or NULL
 *   out_layers_d    device f32 [n_layer,B,T,d] residual stream ENTERING each block (debug/parity), or NULL
 *   out_qkv_d       device f32 [n_layer,B,T,3d] c_attn outputs ("presents" source, modeling_gpt2.py:187), or NULL
 * Position ids are 0..T-1 (modeling_gpt2.py:420-423); dropout is the identity (eval).
 */
int r4d_gpt2_encode_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w,
                        const int64_t* ids_d, const float* inputs_embeds_d, int32_t B, int32_t T,
                        float* out_hidden_d, float* out_meanpool_d, float* out_layers_d, float* out_qkv_d,
                        void* workspace_d, size_t workspace_bytes, void* stream);

/*
 * Several right-padded batches in ONE launch sequence (throughput form of the call above; same values).
 * The reference encodes one 32-sequence batch per model call (train_retriever.py:414-432); a batch's
 * embeddings depend on its own padding (mean over padded positions, :420), so batches are NOT merged -- but
 * the row-wise work (LayerNorm, Conv1D GEMMs) of all batches runs over their concatenated rows, while the
 * embedding/positions, attention and mean-pool stay per batch.
 *   ids_d  HOST array [n_groups] of device int64 [Bs[g], Ts[g]] pointers;  Bs, Ts HOST arrays
 *   out_meanpool_d device f32 [sum(Bs), d], batches in order
 */
size_t r4d_gpt2_groups_workspace_bytes(const r4d_gpt2_config* cfg, int32_t n_groups, const int32_t* Bs,
                                       const int32_t* Ts);
int r4d_gpt2_encode_groups_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, int32_t n_groups,
                               const int64_t* const* ids_d, const int32_t* Bs, const int32_t* Ts,
                               float* out_meanpool_d, void* workspace_d, size_t workspace_bytes, void* stream);

/* The same launch sequence with every output of r4d_gpt2_encode_f32: batches given as ids (ids_d) OR as embeddings
 * (embeds_d: HOST array of device f32 [Bs[g], Ts[g], d] pointers), exactly one of the two non-NULL.  Rows of all
 * batches are concatenated in order (batch g starts at row sum_{j<g} Bs[j]*Ts[j]):
 *   out_hidden_d   f32 [rows, d] or NULL     out_meanpool_d f32 [sum(Bs), d] or NULL (at least one of the two)
 *   out_qkv_d      f32 [n_layer, rows, 3d] or NULL (c_attn output per layer: the K / V rows a decode cache starts from)
 * Used to prefill a RAGGED set of prompts grouped by length: a causal model never lets right-padding reach a real
 * position, so each group only needs padding to its own longest member. */
int r4d_gpt2_encode_groups_ex_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, int32_t n_groups,
                                  const int64_t* const* ids_d, const float* const* embeds_d, const int32_t* Bs,
                                  const int32_t* Ts, float* out_hidden_d, float* out_meanpool_d, float* out_qkv_d,
                                  void* workspace_d, size_t workspace_bytes, void* stream);

/*
 * Incremental decode with a key/value cache -- the model's `past` mechanism (`layer_past` concatenation,
 * modeling_gpt2.py:177-197; `past` / `presents`, :400-509), which the reference's greedy loops never use
 * (utils/Evaluation_generator.py:153-167 and Evaluation_SimpleDyG.py:126-134 re-run the FULL forward per token).
 * One call = one new position for each of B independent sequences:
 *   ids_d            device int64 [B] new token ids, or NULL when inputs_embeds_d is given
 *   inputs_embeds_d  device f32 [B,d] or NULL
 *   pos_d            device int32 [B]: position of the new token = number of positions already cached for that
 *                    sequence (position embedding wpe[pos]; must be < t_cap and < n_positions, else the row is NaN)
 *   kv_cache_d       device f32 [n_layer, B, t_cap, 2*d]: per position the K row then the V row of every head.
 *                    Rows [0, pos) of each sequence must hold its history (fill them from r4d_gpt2_encode_f32's
 *                    out_qkv_d: columns d..3d of c_attn); row pos is WRITTEN by this call.
 *   out_hidden_d     device f32 [B,d]: ln_f output of the new position (feed r4d_lm_logits_f32)
 * Same values as the last row of a full forward over the extended sequence, up to fp32 summation order.
 */
size_t r4d_gpt2_decode_workspace_bytes(const r4d_gpt2_config* cfg, int32_t B);
int r4d_gpt2_decode_step_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const int64_t* ids_d,
                             const float* inputs_embeds_d, const int32_t* pos_d, float* kv_cache_d, int32_t B,
                             int32_t t_cap, float* out_hidden_d, void* workspace_d, size_t workspace_bytes,
                             void* stream);

/*
 * Greedy decoding with the loop state ON THE DEVICE -- the reference's greedy loops (utils/Evaluation_SimpleDyG.py:126-145,
 * utils/Evaluation_generator.py:153-175: argmax of the last position's logits, append, stop rules) as one launch
 * sequence per token with no host round trip, so that a step can be captured once and replayed as a HIP graph
 * (a cached step is launch-latency-bound: ~70 small kernels).  One step =
 *     logits = last . wte^T  ->  per sequence: v = argmax (lowest index among equal maxima);
 *     if active: out_tokens[b][gen_len++] = v;  active &= !(gen_len >= max_gen || v in eos || gen_len >= out_cap
 *                                                          || lens + 1 >= min(len_limit, t_cap))
 *     next = v;  pos = active ? lens : 0;  lens += active        (finished sequences keep their slot and are ignored)
 *     last = r4d_gpt2_decode_step_f32(ids = next, pos)
 * All arrays are device memory owned by the caller and must stay valid (and in place) for the life of a graph:
 *   last_d [B,d] f32 in/out (ln_f row of the newest position)   logits_d [B,V] f32 scratch (the step's logits)
 *   next_d [B] i64   lens_d [B] i32 (positions cached; in/out)   pos_d [B] i32   active_d [B] i32 (in/out, 1 = running)
 *   gen_len_d [B] i32 (in/out)   out_tokens_d [B,out_cap] i32   params_d int32[8] (below)
 */
typedef struct r4d_greedy_state {
    float* last_d;
    float* logits_d;
    int64_t* next_d;
    int32_t* lens_d;
    int32_t* pos_d;
    int32_t* active_d;
    int32_t* gen_len_d;
    int32_t* out_tokens_d;
    const int32_t* params_d; /* device int32[8], read every step (so one captured graph serves every batch):
                              *   [0] max_gen    stop after this many generated tokens
                              *   [1] len_limit  stop once lens + 1 >= min(len_limit, t_cap) (the cache row written next is lens)
                              *   [2] n_eos 0..4, [3..6] eos ids: stop after generating any of them;  [7] reserved */
    int32_t out_cap;         /* row length of out_tokens_d */
} r4d_greedy_state;
typedef struct r4d_decode_graph r4d_decode_graph;      /* opaque: a captured, instantiated greedy step */

size_t r4d_gpt2_greedy_workspace_bytes(const r4d_gpt2_config* cfg, int32_t B);
/* one step, launched kernel by kernel on `stream` */
int r4d_gpt2_greedy_step_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_greedy_state* st,
                             float* kv_cache_d, int32_t B, int32_t t_cap, void* workspace_d, size_t workspace_bytes,
                             void* stream);
/* capture the same step into a HIP graph (nothing runs); every pointer reachable from the arguments is baked in */
int r4d_gpt2_greedy_graph_create(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_greedy_state* st,
                                 float* kv_cache_d, int32_t B, int32_t t_cap, void* workspace_d, size_t workspace_bytes,
                                 r4d_decode_graph** out_graph);
/* replay it n_steps times on `stream` (asynchronous) */
int r4d_decode_graph_launch(r4d_decode_graph* graph, int32_t n_steps, void* stream);
void r4d_decode_graph_destroy(r4d_decode_graph* graph);

/*
 * Sampled decoding (additive ABI v6 entries): the choice of the next token of the reference's generate()
 * (models/modeling_utils.py:608-927: enforce_repetition_penalty_, / temperature, top_k_top_p_filtering, multinomial) as ONE
 * kernel in the greedy bookkeeping kernel's place -- one workgroup per sequence, no hand-off between workgroups.  Per row x[0..V):
 *   1. repetition penalty r >= 1: for every id whose bit is set in `seen`, x = x < 0 ? x * r : x / r; the chosen id's bit is set
 *      afterwards (seen_d NULL: no penalty, nothing set);
 *   2. do_sample == 0: the argmax of the penalised row, lowest index among equal maxima; else
 *   3. y = x / temperature in fp32 (only when temperature != 1);
 *   4. top_k > 0: k' = min(max(top_k, 1), V), thr = the k'-th largest y; every y < thr is dropped (ties at thr are all kept);
 *   5. top_p < 1: the survivors in the order (value descending, index ascending), weights w = exp(y - max); the i-th is kept iff
 *      i == 0 or the weight of the i before it is <= top_p * (the weight of all survivors);
 *   6. u = (word >> 8) * 2^-24 in [0, 1), word = the first output of Philox-4x32-10 with counter (step, stream, 0,
 *      R4D_SAMPLE_PHILOX_SITE) and key (seed_lo, seed_hi); the token is the LOWEST kept index whose inclusive weight prefix in
 *      INDEX order exceeds u * Z, Z the weight of the kept set.
 * Weights are summed as 64-bit fixed point (floor(expf(y - max) * 2^40), integer additions): every sum is exact in that unit
 * and independent of the order it was taken in, so the token depends on (row values, seen bits, parameters, seed, stream, step)
 * alone -- not on B, on the row's place in the batch, or on a graph replay.  NaN counts as -inf (it is chosen only when no entry
 * is above -inf); a row without an entry above -inf gives id 0; a row whose maximum is +inf gives the lowest-indexed +inf entry
 * (for both, the kept set is that one id).  Any V >= 1.
 *   fparams_d  device float[4]  {temperature > 0, top_p in [0,1], repetition_penalty >= 1, reserved}
 *   iparams_d  device int32[4]  {do_sample, top_k >= 0, seed_lo, seed_hi}     both read by the kernel at every launch
 */
#define R4D_SAMPLE_PHILOX_SITE 0x53414d50u        /* "SAMP" */
/* The single operation on logits_d [B,V]: step_d, stream_d device int32 [B]; seen_d device uint32 [B, ceil(V/32)] in/out or NULL;
 * out_token_d device int64 [B]; out_keep_d device uint32 [B, ceil(V/32)] or NULL: bit j%32 of word j/32 = id j is in the kept set
 * (every word written, bits past V clear; do_sample == 0: the chosen id alone); out_u_d device float [B] or NULL.  No workspace. */
int r4d_sample_logits_f32(const float* logits_d, int32_t B, int32_t V, uint32_t* seen_d, const int32_t* step_d,
                          const int32_t* stream_d, const float* fparams_d, const int32_t* iparams_d, int64_t* out_token_d,
                          uint32_t* out_keep_d, float* out_u_d, void* stream);
/* The loop state of the sampled step: r4d_greedy_state's fields with its conventions (the step counter of the draw is gen_len_d
 * BEFORE the step increments it), plus the sampler's own.  Caller state like the greedy one: seen_d is read and updated. */
typedef struct r4d_sample_state {
    float* last_d;
    float* logits_d;
    int64_t* next_d;
    int32_t* lens_d;
    int32_t* pos_d;
    int32_t* active_d;
    int32_t* gen_len_d;
    int32_t* out_tokens_d;
    const int32_t* params_d;
    int32_t out_cap;
    uint32_t* seen_d;          /* device uint32 [B, ceil(V/32)] or NULL */
    const int32_t* stream_d;   /* device int32 [B] */
    const float* fparams_d;    /* device float[4], read every step (so one captured graph serves every call) */
    const int32_t* iparams_d;  /* device int32[4], read every step */
} r4d_sample_state;
/* One step = the LM head on the greedy step's route, the choice above, r4d_gpt2_decode_step_f32 on the chosen ids.  The graph is an
 * r4d_decode_graph: r4d_decode_graph_launch / _destroy serve it. */
size_t r4d_gpt2_sample_workspace_bytes(const r4d_gpt2_config* cfg, int32_t B);
int r4d_gpt2_sample_step_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_sample_state* st,
                             float* kv_cache_d, int32_t B, int32_t t_cap, void* workspace_d, size_t workspace_bytes,
                             void* stream);
int r4d_gpt2_sample_graph_create(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_sample_state* st,
                                 float* kv_cache_d, int32_t B, int32_t t_cap, void* workspace_d, size_t workspace_bytes,
                                 r4d_decode_graph** out_graph);

/*
 * Beam search (additive ABI v6 entries): the reference's greedy beam search (models/modeling_utils.py:929-1153, BeamHypotheses
 * :1205-1252; do_sample False) with the beam step on the device.  2 <= n_beams <= R4D_BEAM_MAX beams per prompt; the rows of
 * every per-row array are R = B0 * n_beams, rows b n .. b n + n - 1 the beams of prompt b.  V >= 2 and n V < 2^31.
 *
 * Candidates of a row x[0..V) with beam score s (one workgroup per row):
 *   1. the repetition penalty of the sampled step (its rule 1) through `seen`; NaN counts as -inf;
 *   2. m = max x, lse = logf(sum expf(x - m)), score_j = ((x_j - m) - lse) + s, each an IEEE fp32 operation in that order; the sum
 *      is taken in an order that the workgroup's shape alone fixes, so a row's scores depend on the row, not on R or its place;
 *      a score that comes out NaN counts as -inf (a row without a finite maximum: every score is -inf);
 *   3. the row's min(2n, V) best in the order (score descending, id ascending).
 * Candidates of a prompt: its n lists merged into the 2n best in the order (score descending, flat index beam * V + id ascending)
 * -- the tie rule that torch.topk leaves open.
 *   fparams_d  device float[4]  {length_penalty > 0, repetition_penalty >= 1, reserved, reserved}     read at every launch
 */
#define R4D_BEAM_MAX 16
/* The selection alone.  logits_d [R,V]; beam_scores_d [R]; seen_d uint32 [R, ceil(V/32)] or NULL (read only);
 * cand_scores_d float / cand_ids_d int32 [R, 2n]: the rows' lists (entries past min(2n, V): -inf / -1);
 * out_scores_d float / out_index_d int32 [B0, 2n]: the prompts' candidates, index = beam * V + id.  No workspace. */
int r4d_beam_select_f32(const float* logits_d, const float* beam_scores_d, const uint32_t* seen_d, const float* fparams_d,
                        int32_t B0, int32_t n_beams, int32_t V, float* cand_scores_d, int32_t* cand_ids_d, float* out_scores_d,
                        int32_t* out_index_d, void* stream);
/* Reorder a key/value cache [n_layer, R = B0 n, t_cap, 2d] in place: for every group b with active_d[b] != 0 (active_d NULL: every
 * group) and every position p in [lo_d[b], hi_d[b]) (clipped to [0, t_cap)), row b n + i receives the K | V line of row
 * src_row_d[b n + i].  A source outside the group's own rows is never read: the receiving row's lines are filled with NaN.  Groups
 * whose permutation is the identity are skipped; only rows whose source differs are stored.  No workspace, no second cache.
 * The copy moves 2 * n_layer * (rows that move) * (hi - lo) * 2d * 4 bytes. */
int r4d_kv_cache_reorder_f32(float* kv_cache_d, const int32_t* src_row_d, const int32_t* lo_d, const int32_t* hi_d,
                             const int32_t* active_d, int32_t n_layer, int32_t B0, int32_t n, int32_t t_cap, int32_t d,
                             void* stream);
/* The loop state of the beam step: r4d_greedy_state's fields PER ROW with its conventions, then the beams' own.  At the start of
 * a step, per prompt (modeling_utils.py:1032-1075):
 *     done |= hyp_count >= n && worst >= best candidate score / (T + max_gen - 1) ** length_penalty    (the reference's max_length - 1)
 *     done: the prompt's rows go inactive and its state is no longer touched; else the 2n candidates are walked in order:
 *       an eos id: the hypothesis (the source beam's ids so far, score = candidate score / (T + gen_len) ** length_penalty, in
 *         double from the fp32 score) joins the list while it holds fewer than n, or when it beats `worst`: the entry with the
 *         lowest (score, list position) leaves and worst becomes the lowest score that stays;
 *       any other id becomes the next beam, until n are found (fewer than n: status bit 0, the reference's "Beam should always be full").
 *     beam_scores, next, beam_idx (source row), pos, lens, active, gen_len are written; the prompt's rows of out_tokens and seen are
 *     reordered in place and receive the new id; the rows stop after max_gen ids or at the cache's end, as the greedy rows do.
 * params_d as in r4d_greedy_state, with [7] = T, the prompt length shared by all rows.  The caller starts a generation with
 * beam_scores = {0, -1e9, ...} per prompt (:956-959), done = hyp_count = hyp_added = status = 0, hyp_worst = 1e9, active = 1, gen_len = 0.
 * Nothing else needs a defined content on entry: candidates and hypotheses are written before they are read. */
typedef struct r4d_beam_state {
    float* last_d;
    float* logits_d;
    int64_t* next_d;
    int32_t* lens_d;
    int32_t* pos_d;
    int32_t* active_d;
    int32_t* gen_len_d;
    int32_t* out_tokens_d;
    const int32_t* params_d;
    int32_t out_cap;
    int32_t n_beams;
    uint32_t* seen_d;           /* device uint32 [R, ceil(V/32)] or NULL; reordered with the beams */
    const float* fparams_d;     /* device float[4], read every step */
    float* beam_scores_d;       /* [R] in/out */
    int32_t* beam_idx_d;        /* [R] out: the row each row continues (this step's src_row of the cache reorder) */
    float* cand_scores_d;       /* [R, 2n] scratch */
    int32_t* cand_ids_d;        /* [R, 2n] scratch */
    int32_t* lo_d;              /* [B0] out: the reorder's range of this step, [T, positions cached) */
    int32_t* hi_d;              /* [B0] out */
    int32_t* group_active_d;    /* [B0] out: 1 = the prompt took new beams at this step */
    int32_t* done_d;            /* [B0] in/out */
    int32_t* hyp_count_d;       /* [B0] in/out: hypotheses held, <= n */
    int32_t* hyp_added_d;       /* [B0] in/out: hypotheses ever added (hyp_seq_d counts with it) */
    int32_t* status_d;          /* [B0] in/out: bit 0 = a step found fewer than n beams */
    double* hyp_worst_d;        /* [B0] in/out */
    double* hyp_score_d;        /* [B0, n] */
    int32_t* hyp_len_d;         /* [B0, n] generated ids of the hypothesis (the prompt not counted) */
    int32_t* hyp_seq_d;         /* [B0, n] order of arrival: the reference's list position is the rank of this number */
    int32_t* hyp_ids_d;         /* [B0, n, out_cap] the generated ids */
} r4d_beam_state;
/* One step = the LM head on the greedy step's route (R rows), the candidates, the walk, r4d_kv_cache_reorder_f32 over
 * [T, positions cached) by beam_idx_d -- valid because the n rows of a group are prefilled from one prompt and hold identical
 * bits below T -- and r4d_gpt2_decode_step_f32 on the chosen ids.  kv_cache_d [n_layer, R, t_cap, 2d].  The graph is an
 * r4d_decode_graph: r4d_decode_graph_launch / _destroy serve it. */
size_t r4d_gpt2_beam_workspace_bytes(const r4d_gpt2_config* cfg, int32_t B0, int32_t n_beams);
int r4d_gpt2_beam_step_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_beam_state* st, float* kv_cache_d,
                           int32_t B0, int32_t t_cap, void* workspace_d, size_t workspace_bytes, void* stream);
int r4d_gpt2_beam_graph_create(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_beam_state* st, float* kv_cache_d,
                               int32_t B0, int32_t t_cap, void* workspace_d, size_t workspace_bytes, r4d_decode_graph** out_graph);

/* lm_logits = hidden @ wte^T  (tied lm_head, modeling_gpt2.py:585; modeling_rag.py:675).
 * hidden_d [M,d], wte_d [V,d] -> logits_d [M,V]. */
int r4d_lm_logits_f32(const float* hidden_d, const float* wte_d, int32_t M, int32_t V, int32_t d,
                      float* logits_d, void* stream);

/* Attention implementation switch: -1 = auto (default) / 1 = fused flash-style kernels wherever instantiated
 * (head_dim in {32,64}: key-split kernel; {96,128,256}: column-split kernel; scores never leave the CU),
 * 0 = three launches (batched Q.K^T GEMM, causal softmax weights, P.V GEMM; also the fallback for other head dims) and a small
 * fourth that divides the output rows by the softmax row sums,
 * 2 = fused with the key-split kernel forced at head_dim 96/128/256 (A/B tuning).  Same results to fp32 rounding. */
int r4d_set_attention_fused(int32_t mode);

/* f16x2 attention (ABI v5, additive): in gemm mode 2 (f16x2) r4d_gpt2_encode_* runs head_dim 32 / 64 / 96 / 128 / 256 attention on the fp16
 * matrix cores (csrc/attention_h2.hip) -- the c_attn GEMM then writes its result as "h2 words" (uint32 per element:
 * fp16 hi | fp16 lo' << 16 of value / 4, value = hi + 2^-11 lo' to 2^-22 relative; csrc/h2.h) instead of fp32, and the attention
 * kernel consumes them without conversion.  Not used when the caller asks for the qkv tensor (out_qkv_d) and for other head
 * dims; |q|, |k|, |v| < 2^18.  r4d_set_attention_h2(0) keeps the exact-f32 attention kernels in every mode (returns the previous
 * setting; process-wide like r4d_set_gemm_split3: ranks must agree).
 * r4d_pack_h2_words_f32: x_d fp32 [n] -> words_d uint32 [n] (what the GEMM epilogue writes; for tests and external producers).
 * r4d_attention_h2_f32: r4d_attention_f32 on words: qkv_words_d [B*T, 3d] -> a_d fp32 [B*T, d]; head_dim 32 / 64 / 96 / 128 / 256
 * (any other head_dim, B < 1 or T < 1 is refused). */
int r4d_set_attention_h2(int32_t on);
/* KEY-BLOCKED K (round 5): row-major K costs every K load instruction of the attention 32 cache lines (each lane
 * its own key row, 32 bytes of each line used); in the key-blocked image -- [ceil(rows / 32)][n_head][head_dim / 8][2][32][4] uint32:
 * for every 32 consecutive token rows, head and 8-element step one contiguous 1 KB chunk [half][row & 31][4 words] -- the same
 * instruction reads 8-10 whole lines (a fifth off the head_dim-256 launch in the bench step; every head_dim the f16x2 attention serves).  Inside the encoder the LDS-DMA c_attn GEMM writes the
 * image directly (r4d_set_attention_kblk(0) keeps row-major K; returns the previous setting; env R4D_ATT_KBLK=0 does the same).
 * r4d_pack_kblk_words builds it from row-major qkv words (tests, external producers); r4d_attention_h2_kblk_f32 is
 * r4d_attention_h2_f32 reading K from it (the K columns of qkv_words_d are not read) -- bit-identical results. */
int r4d_set_attention_kblk(int32_t on);
/* LAYER 0's REPEATED PAD ROWS.  In layer 0 the c_attn row of a position depends on (token, position) only, and the reference's
 * batching makes most rows of a call [PAD] rows (70 % in the bench step).  On the path above (f16x2 lines, h2 words, the
 * key-blocked image, ids given, qkv not handed out) the layer-0 c_attn GEMM therefore skips every 32-row block (by global row
 * index) whose rows all carry one candidate token -- the most frequent last-position token of the call, found on the device --
 * and a copy kernel fills those rows from round_up(Tmax, 32) table rows (token, p) that the same launch computes: the bits of
 * every row are those of the full GEMM.  r4d_set_layer0_pad_rows(0) keeps the full GEMM (returns the previous setting; env
 * R4D_LAYER0_PAD_ROWS=0 does the same; process-wide).  Either way the encoder workspaces hold the table rows and the plan:
 * with Mp = round_up(rows, 32), Tcap = round_up(Tmax, 32), x, the LayerNorm rows, qkv and the key-blocked image have Mp + Tcap
 * rows, and 8 + 2 Tcap + 2 Mp + round_up(Mp / 32 + Tcap / 32, 4) + Mp / 32 + vocab 32-bit words follow the key-blocked image.
 * r4d_gpt2_layer0_pad_rows_offset (tests): the byte offset of those words in a workspace of r4d_gpt2_groups_workspace_bytes;
 * word 0 = listed blocks, 1 = dropped blocks, 2 = the token, 3 / 4 = the word offsets of the two block lists. */
int r4d_set_layer0_pad_rows(int32_t on);
size_t r4d_gpt2_layer0_pad_rows_offset(const r4d_gpt2_config* cfg, int32_t n_groups, const int32_t* Bs, const int32_t* Ts);
int r4d_pack_kblk_words(const uint32_t* qkv_words_d, int64_t rows, int32_t n_head, int32_t d, uint32_t* kblk_d, void* stream);
int r4d_attention_h2_kblk_f32(const uint32_t* qkv_words_d, const uint32_t* kblk_d, int32_t B, int32_t T, int32_t n_head, int32_t d,
                              float* a_d, void* stream);
int r4d_pack_h2_words_f32(const float* x_d, int64_t n, uint32_t* words_d, void* stream);
int r4d_attention_h2_f32(const uint32_t* qkv_words_d, int32_t B, int32_t T, int32_t n_head, int32_t d, float* a_d, void* stream);

/* Pre-split activations (ABI v6, additive; csrc/gemm_h2p.hip).  In gemm mode 2 (f16x2) r4d_gpt2_encode_* keeps the INPUT rows of c_attn,
 * c_fc and mlp.c_proj as "f16x2 lines" -- uint16 [rows][K/32][2][32]: per row and 32 consecutive k one 128-byte line of 32 hi = RN16(x/4)
 * then 32 lo' = RN16((x/4 - hi) 2^11), the layout r4d_split2_planes_f16 gives the weights, 4 bytes per element like fp32 -- written by
 * their producers (the LayerNorm kernels, the c_fc GELU epilogue), and both GEMM operands travel global -> LDS by DMA.  The results are
 * those of the register-staged f16x2 GEMM bit for bit; r4d_set_gemm_h2p(0) selects that one again (returns the previous setting;
 * process-wide like r4d_set_gemm_split3).  n_embd % 256 == 0, else the register-staged path.
 * r4d_split2_lines_f16: x_d fp32 [rows,K] -> lines (tests, external producers).
 * r4d_conv1d_h2p_f32: r4d_conv1d_h2_f32 with x given as lines; out_lines != 0 (epilogue 1 = gelu only): y_d receives lines [M][N/32][2][32].
 * r4d_layernorm_lines_f32: r4d_layernorm_f32 whose output rows are lines (d % 256 == 0; what the encoder launches in this mode). */
int r4d_set_gemm_h2p(int32_t on);
int r4d_layernorm_lines_f32(const float* x_d, const float* w_d, const float* b_d, int32_t rows, int32_t d, float eps,
                            uint16_t* y_lines_d, void* stream);
int r4d_split2_lines_f16(const float* x_d, int64_t rows, int32_t K, uint16_t* lines_d, void* stream);
int r4d_conv1d_h2p_f32(const uint16_t* x_lines_d, const uint16_t* planes_d, const float* bias_d, const float* residual_d, int32_t M,
                       int32_t K, int32_t N, int32_t epilogue, int32_t out_lines, void* y_d, void* stream);

/* Range guard (ABI v6, additive).  The f16x2 arithmetic has fp16's exponent range: an activation, q, k or v of magnitude >= 2^18
 * becomes inf in its first fp16 term and every hidden state downstream of it NaN -- and NaN scores are ordered below everything by
 * the selection, i.e. an ordinary-looking top-k of garbage.  r4d_set_range_flag registers ONE caller-owned
 * device word for the process (one process per device; NULL unregisters; the library never clears it).  While registered:
 *   bit 0 (R4D_RANGE_NONFINITE_HIDDEN) is OR-ed in by the ln_f / mean-pool kernel of r4d_gpt2_encode_* for every row of the
 *         final residual stream that is non-finite or whose variance overflowed (any arithmetic; in f16x2 mode this is how an
 *         out-of-range activation surfaces);
 *   bit 1 (R4D_RANGE_BAD_NORM) by r4d_normalize_rows_f32 for every row whose norm is NaN, inf or zero;
 *   bit 2 (R4D_RANGE_BAD_LABEL) by r4d_lm_ce_f32 / r4d_gpt2_lm_train_step_f32 for a label outside [0, V) that is not the
 *         ignore_index -100 (such a row is not counted; torch's cross_entropy would raise).
 * The calls stay asynchronous: the caller reads the word at its own synchronisation points.  What the Python host mirror does
 * with it (rag4dyg_amd/ops.py, retrieval.py, gpt2.py): retrieval.encode_batches and GPT2Model.forward re-run an f16x2 call whose
 * bit 0 came up ONCE under bf16x3 (fp32's exponent range) with a warning and raise R4DError if the bit comes up again;
 * PoolIndex and search raise R4DError on either bit before any top-k result is handed out; bench.py reports the word of the
 * whole timed region.  encode_* called directly leave the check to the caller (ops.take_range_flag). */
#define R4D_RANGE_NONFINITE_HIDDEN 1u
#define R4D_RANGE_BAD_NORM 2u
#define R4D_RANGE_BAD_LABEL 4u
int r4d_set_range_flag(uint32_t* flag_d);

/* --- single ops, exported for per-op parity tests (same kernels the encoder launches) --- */
/* y = LayerNorm(x) over the last dim.  nn.LayerNorm, modeling_gpt2.py:219,221,339. */
int r4d_layernorm_f32(const float* x_d, const float* w_d, const float* b_d, int32_t rows, int32_t d,
                      float eps, float* y_d, void* stream);
/* y = epilogue(x[M,K] @ W[K,N] + bias[N]); epilogue: 0 none, 1 gelu_new (modeling_gpt2.py:206),
 * 2 add residual_d[M,N].  Conv1D.forward, modeling_utils.py:1267-1271. */
int r4d_conv1d_f32(const float* x_d, const float* w_d, const float* w_t_d /* optional [N,K] copy or NULL */,
                   const float* bias_d, const float* residual_d,
                   int32_t M, int32_t K, int32_t N, int32_t epilogue, float* y_d, void* stream);
/*
 * The same Conv1D on the bf16 matrix cores AT FP32 ACCURACY ("bf16x3" split): every fp32 operand is the exact sum of three
 * bf16 numbers (hi + mid + lo) and a product is evaluated as its six leading partial products
 * (v_mfma_f32_32x32x16_bf16, fp32 accumulation) -- 2.67x fewer matrix-pipe cycles than the exact-f32 MFMA at an error
 * against float64 that is no larger (shorter fp32 accumulation chains; acceptance table in profiles/).
 * r4d_split3_planes_bf16: the STATIC operand, once per checkpoint: w_d fp32 [K,N] (reference Conv1D layout; transposed != 0:
 * an [N,K] copy) -> planes_d bf16 [3][N][K] (hi, mid, lo planes, K contiguous; 6 * N * K bytes).
 * r4d_conv1d_s3_f32: y = epilogue(x[M,K] @ W + bias) with W given as those planes; x stays fp32 and is split on the fly.
 * K % 32 == 0; epilogue as r4d_conv1d_f32.
 */
int r4d_split3_planes_bf16(const float* w_d, int32_t K, int32_t N, int32_t transposed, uint16_t* planes_d, void* stream);
int r4d_conv1d_s3_f32(const float* x_d, const uint16_t* planes_d, const float* bias_d, const float* residual_d,
                      int32_t M, int32_t K, int32_t N, int32_t epilogue, float* y_d, void* stream);
/*
 * The same Conv1D on the FP16 matrix cores at fp32 accuracy with THREE products per fp32 product ("f16x2", ABI v5;
 * csrc/gemm_h2.hip): x = hi + 2^-11 lo' with hi = RN16(x), lo' = RN16((x - hi) 2^11) (the second term stays a normal fp16
 * number over the whole range), a.b = hi.hi + 2^-11 (lo'.hi + hi.lo') in two fp32 accumulator sets joined once; half the
 * matrix-pipe cycles of bf16x3 at an error against float64 no larger than bf16x3's or the exact-f32 MFMA's (acceptance table
 * in profiles/).  Operand range: |x| < 2^18 for the activation (pre-scaled by 2^-2 inside the kernel; full precision for elements >= 2.4e-4,
 * an absolute floor of 6e-11 below), |w| < 6e4 for the
 * weight; beyond it the result is inf / NaN, not a silently wrong number.
 * r4d_split2_planes_f16: w_d fp32 [K,N] (transposed != 0: [N,K]) -> planes_d fp16 [N][K/32][2][32] (4 * N * K bytes: per row and 32 consecutive k one 128-byte line of 32 hi then 32 lo'
 * values; K % 32 == 0), once per checkpoint.
 * r4d_conv1d_h2_f32: y = epilogue(x[M,K] @ W + bias), K % 32 == 0; epilogue as r4d_conv1d_f32.
 */
int r4d_split2_planes_f16(const float* w_d, int32_t K, int32_t N, int32_t transposed, uint16_t* planes_d, void* stream);
int r4d_conv1d_h2_f32(const float* x_d, const uint16_t* planes_d, const float* bias_d, const float* residual_d,
                      int32_t M, int32_t K, int32_t N, int32_t epilogue, float* y_d, void* stream);
/* Conv1D arithmetic of the encoder / training-forward GEMMs.  1 (default): bf16x3 where a layer carries its planes; 2: f16x2
 * where it carries those planes (bf16x3 where it only has the bf16 ones; the training GEMMs stay bf16x3); 0: exact-f32 MFMA
 * kernels everywhere (planes ignored).  PROCESS-WIDE (one process drives one device; ranks of a sharded job must agree, or the
 * merged shards differ from the one-GPU result in the last bits), not thread-safe against concurrent calls. */
/* Decode-only fold of a LayerNorm into the projection that reads it (ABI v4): wT_d [N,K] (k-contiguous weight), ln_w_d / ln_b_d [K]
 * -> wTg_d [N,K] = ln_w[k] * wT[n][k] and lnc_d [2][N] = (sum_k ln_w[k] wT[n][k], sum_k ln_b[k] wT[n][k]); the operands of
 * r4d_gpt2_layer's c_attn_wTg / c_attn_lnc (with ln_1) and c_fc_wTg / c_fc_lnc (with ln_2).  Once per checkpoint. */
int r4d_fold_layernorm_f32(const float* wT_d, const float* ln_w_d, const float* ln_b_d, int32_t N, int32_t K, float* wTg_d,
                           float* lnc_d, void* stream);
/* The weight-stream GEMM of the cached decode step and of the greedy loop's LM head, alone (additive ABI v6 entries;
 * csrc/gemm_skinny.hip): y[M,N] = epilogue(x'[M,K] . wT[N,K]^T + bias), 1 <= M <= 32 rows, K a multiple of 256, N >= 1, wT_d the
 * k-contiguous weight; epilogue as r4d_conv1d_f32 (residual_d with epilogue 2 and only with it; y_d may be residual_d).  The entry
 * launches what the decode step launches for the same arguments -- the kernel form follows K, N and the tuning word R4D_SKINNY16
 *  -- and adds no route.
 *   x' = x, or LayerNorm(x) in one of two forms, both for K = 512 or 768 only: ln_w_d / ln_b_d [K] (both or neither) -- the
 *   LayerNorm is formed in the launch; ln_fold_d [2][N] -- wT_d is the FOLDED weight and ln_fold_d its column constants, both from
 *   r4d_fold_layernorm_f32 (16-column kernels only: refused under R4D_SKINNY16=0).  The two forms exclude each other; a folded
 *   LayerNorm may carry a residual.
 *   workspace_d: r4d_conv1d_skinny_workspace_bytes(K, N) = 4 * (ceil(K / 256) * 32 * N + 256) bytes (0 for an unsupported K or N).  Its
 *   first 256 words are the split-K tickets: counters_zeroed = 0 -- the entry clears them where the chosen form reads them;
 *   counters_zeroed != 0 -- the caller promises that they are zero (a completed launch leaves them zero).  Nothing else in the
 *   workspace is read before it is written.
 * Only rows 0 .. M-1 of y_d are written.  x_d, wT_d, ln_w_d and ln_b_d 16-byte aligned.  R4D_ERR_INVALID for anything else above,
 * R4D_ERR_WORKSPACE for a short workspace; nothing is launched in either case. */
size_t r4d_conv1d_skinny_workspace_bytes(int32_t K, int32_t N);
int r4d_conv1d_skinny_f32(const float* x_d, const float* wT_d /* [N,K] */, const float* bias_d, const float* residual_d, int32_t M,
                          int32_t K, int32_t N, int32_t epilogue, const float* ln_w_d, const float* ln_b_d, float ln_eps,
                          const float* ln_fold_d, int32_t counters_zeroed, float* y_d, void* workspace_d, size_t workspace_bytes,
                          void* stream);
int r4d_set_gemm_split3(int32_t mode);
int r4d_get_gemm_split3(void);
/*
 * Plain bf16 arithmetic for the encoder FORWARD GEMMs (additive ABI v6 entries; csrc/gemm_b1.hip).  NOT fp32-accurate: both
 * operands are rounded to bf16 (8 significant bits, round to nearest even) and multiplied ONCE on v_mfma_f32_32x32x16_bf16 with
 * fp32 accumulation -- a sixth of the matrix-pipe work of bf16x3, a third of f16x2's.  bf16 has fp32's exponent range.
 * r4d_conv1d_bf16_f32: y = epilogue(RN_bf16(x)[M,K] @ RN_bf16(W) + bias) with W given as ONE k-contiguous bf16 plane
 * w_bf16_d [N][K] = plane 0 of r4d_split3_planes_bf16 (2 * N * K bytes); x stays fp32 and is rounded while it is staged.
 * K % 32 == 0, x_d and w_bf16_d 16-byte aligned (R4D_ERR_INVALID otherwise, nothing is launched); epilogue as r4d_conv1d_f32.
 * A row's result does not depend on M or on the other rows of the call.
 * r4d_set_encode_bf16(on != 0): while on, the four Conv1D GEMMs of a block run on that kernel in r4d_gpt2_encode_f32,
 * r4d_gpt2_encode_groups_f32 and r4d_gpt2_encode_groups_ex_f32 -- wherever the layer carries *_w3 planes and the shape qualifies,
 * WHATEVER r4d_set_gemm_split3 says -- with the structure of the bf16x3 path: fp32 activations, the exact-f32 attention kernels,
 * no f16x2 lines or h2 words.  Only plane 0 of *_w3 is read in this mode: a caller may pass a buffer that holds just that plane.
 * No other entry reads the switch (training forwards and steps, the cached decode step at any batch size, the greedy step and
 * graph, r4d_lm_logits_f32, r4d_conv1d_*, the scoring kernels: the same bits on as off).  Returns the previous setting; default 0;
 * process-wide like r4d_set_gemm_split3: ranks must agree.  r4d_get_encode_bf16 reads it.
 */
int r4d_conv1d_bf16_f32(const float* x_d, const uint16_t* w_bf16_d /* [N][K] */, const float* bias_d, const float* residual_d,
                        int32_t M, int32_t K, int32_t N, int32_t epilogue, float* y_d, void* stream);
int r4d_set_encode_bf16(int32_t on);
int r4d_get_encode_bf16(void);
/*
 * bf16 ATTENTION for the encoder forward under r4d_set_encode_bf16 (additive ABI v6 entries; csrc/attention_b1.hip).  NOT
 * fp32-accurate.  Per (sequence, head): q, k and v are rounded to bf16 (round to nearest even, v_cvt_pk_bf16_f32: the rounding of
 * r4d_conv1d_bf16_f32); S = q . k^T on ONE v_mfma_f32_32x32x16_bf16 per 16 k with fp32 accumulation, divided by sqrt(hd) in fp32;
 * the causal mask is by selection (a key right of the diagonal or at / past T contributes p = 0 exactly, whatever memory holds);
 * the online softmax is fp32; the UNNORMALISED p = exp(s - m) enters P . V rounded to bf16 while the row sum adds the unrounded
 * fp32 p; O is accumulated in fp32 and divided by the row sum at the end.  A (sequence, head)'s bits depend on its own operands
 * alone: not on the launch it travels in, on its neighbours, or on what lies past T.
 * r4d_set_encode_attention_bf16(on != 0) returns the previous setting; default 0; process-wide.  The switch is read by the
 * encoder entries only (those r4d_set_encode_bf16 names) and ONLY WHILE r4d_set_encode_bf16 is on: alone it changes nothing.
 * While both are on, a block whose c_attn runs on the plain-bf16 GEMM takes its attention on this kernel: c_attn writes RN(q|k|v) as
 * bf16 [M, 3d] (fp32 as before where the caller asked for qkv: the kernel then rounds while staging -- the same bits), the
 * attention writes RN(O) as bf16 [M, d] and attn.c_proj reads that.  Both fit the fp32 buffers of the workspace: no size query
 * changes.  Where the kernel does not serve a shape the block takes the route of r4d_set_encode_bf16 alone: through these entries
 * that is a head dim above 256 (a head dim off the multiples of 16, and more than 65,535 sequences in one launch, are refused by
 * the entries themselves whatever the switches say).  r4d_get_encode_attention_bf16 reads the switch.
 * r4d_attention_bf16_groups: the kernel alone over n_groups (1 .. 16) batches in ONE launch: batch g = Bs[g] sequences of Ts[g]
 * tokens whose first token row is row0s[g] of qkv_d [rows, 3d] / a_d [rows, d].  qkv_is_bf16 / out_is_bf16: the element type behind
 * the pointers (0 fp32, 1 bf16 bits).  head_dim = d / n_head a multiple of 16 in 16 .. 256, 1 <= T <= 1024, at most 65,535
 * sequences, both pointers 16-byte aligned; anything else is refused before any launch (R4D_ERR_INVALID).  Only the batches' own
 * rows of a_d are written.
 */
int r4d_set_encode_attention_bf16(int32_t on);
int r4d_get_encode_attention_bf16(void);
int r4d_attention_bf16_groups(const void* qkv_d, int32_t qkv_is_bf16, int32_t n_groups, const int32_t* Bs, const int32_t* Ts,
                              const int64_t* row0s, int32_t n_head, int32_t d, void* a_d, int32_t out_is_bf16, void* stream);
/*
 * bf16 STORE of the activations for the encoder forward under r4d_set_encode_bf16 (additive ABI v6 entries).  Changes NO output bit:
 * the plain-bf16 GEMM rounds its fp32 A operand to bf16 while staging it (round to nearest even, v_cvt_pk_bf16_f32); with this
 * switch the same rounding is applied ONCE where the activation is produced and the GEMM reads the bf16 rows as they are.
 * r4d_set_encode_act_bf16(on != 0) returns the previous setting; default 0; process-wide.  The switch is read by the encoder
 * entries only (those r4d_set_encode_bf16 names) and ONLY WHILE r4d_set_encode_bf16 is on: alone it changes nothing.  While both
 * are on, each of a block's three buffers is decided on its own: ln1 (every layer; layer 0's leaves the fused embedding kernel) is
 * bf16 [M, d] where c_attn runs on the plain-bf16 GEMM, ln2 [M, d] where c_fc does, the GELU output f [M, 4d] where c_fc AND
 * mlp.c_proj do (c_fc then writes RN(gelu_new(v)) and nothing else) -- and n_embd % 256 == 0 (the producers' 16-byte stores).  Any
 * other buffer stays fp32 and its launches are those of the switch off.  With r4d_set_encode_attention_bf16 on as well, c_attn
 * reads bf16 ln1 and writes bf16 q | k | v (fp32 where the caller asked for qkv, as before).  The bf16 rows occupy the first half of
 * the workspace's fp32 buffers and nothing reads the other half: no size query changes.  r4d_get_encode_act_bf16 reads the switch.
 * The kernels alone: r4d_layernorm_bf16_f32 and r4d_conv1d_bf16_act_f32 (kinds 3 and 4), further down.
 */
int r4d_set_encode_act_bf16(int32_t on);
int r4d_get_encode_act_bf16(void);
/* Causal multi-head attention on packed c_attn output qkv_d [B,T,3d] -> a_d [B,T,d] (heads merged).
 * Attention._attn + split/merge_heads, modeling_gpt2.py:140-175; scale = division by sqrt(hd) (:143).
 * scores_ws_d: device scratch of r4d_attention_workspace_bytes(B,H,T).  B >= 1, 1 <= T <= 1024, head_dim a multiple of 16;
 * anything else, or a shorter workspace, is refused before any launch. */
size_t r4d_attention_workspace_bytes(int32_t B, int32_t n_head, int32_t T);
int r4d_attention_f32(const float* qkv_d, int32_t B, int32_t T, int32_t n_head, int32_t d,
                      float* a_d, void* scores_ws_d, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Retrieval scoring.  Replaces train/train_retriever.py:433-438 (normalise, dot, (x+1)/2) and the
 * ranking of save_index_score :357-358 / the hit loop :461-467.
 * ---------------------------------------------------------------------------------------------- */
/* out[i,:] = x[i,:] / ||x[i,:]||_2 (no eps, train_retriever.py:433,436). */
int r4d_normalize_rows_f32(const float* x_d, int32_t n, int32_t d, float* out_d, void* stream);

size_t r4d_score_topk_workspace_bytes(int32_t Q, int32_t N, int32_t k);
/*
 * S = (q_hat @ pool_hat^T + 1) / 2 over one pool shard, then per-row top-k with the canonical order
 * (score descending, pool index ascending).
 *   q_hat_d [Q,d], pool_hat_d [N,d] row-normalised;  index_offset = global index of shard row 0
 *   out_val_d f32 [Q,k], out_idx_d int64 [Q,k] (global indices)        (k <= r4d_topk_max_k() = 2048, k <= N)
 * The scoring does not depend on k; beyond k = 64 the selection is r4d_topk_f32's second path (below).
 *   out_scores_d f32 [Q,N] full score rows (file-compat mode) or NULL
 */
int r4d_score_topk_f32(const float* q_hat_d, const float* pool_hat_d, int32_t Q, int32_t N, int32_t d,
                       int32_t k, int64_t index_offset, float* out_val_d, int64_t* out_idx_d,
                       float* out_scores_d, void* workspace_d, size_t workspace_bytes, void* stream);
/* Per-row top-k of an f32 matrix with the same canonical order (e.g. the ground-truth top-3 of the float32
 * Jaccard rows, train_retriever.py:461-462).  rows <= 65535, k <= min(r4d_topk_max_k(), n).
 * k <= 64: one launch for n <= 16384 * 1024 / k.  64 < k <= 2048: a workgroup per 16384 columns selects its k best by radix
 * select and sorts them (one launch), longer rows repeat that over the candidates -- no cross-workgroup hand-off.  The result is
 * the same at every k: values as order-preserving keys (NaN -> -inf, -0.0 -> +0.0), key descending, column ascending, the first
 * k; a NaN is reported as -inf.  A workspace size never shrinks from k = 64 to k = 65. */
int r4d_topk_max_k(void);                     /* 2048: the largest k of the three f32 entries (r4d_topk_f64: 64) */
size_t r4d_topk_f32_workspace_bytes(int32_t rows, int32_t n, int32_t k);
int r4d_topk_f32(const float* m_d, int32_t rows, int32_t n, int32_t k, float* out_val_d, int64_t* out_idx_d,
                 void* workspace_d, size_t workspace_bytes, void* stream);
/* Merge G per-shard candidate lists (after the RCCL all-gather): vals_d [G,Q,k], idx_d [G,Q,k]
 * -> out [Q,k], same canonical order; result == single-GPU top-k by construction.  Shards in ascending order of
 * their index ranges (rank order), every list sorted by (value desc, index asc) as r4d_score_topk_f32 emits them.
 * k <= r4d_topk_max_k(), Q <= 65535, G * k <= 2^30.  A shard shorter than k pads its list with (-inf, INT64_MAX); a pad is an
 * ordinary candidate at its list position (it can only surface where fewer than k real candidates exist).  k > 64 takes the
 * gathered lists through r4d_topk_f32's second path. */
size_t r4d_merge_topk_workspace_bytes(int32_t G, int32_t Q, int32_t k);
int r4d_merge_topk_f32(const float* vals_d, const int64_t* idx_d, int32_t G, int32_t Q, int32_t k,
                       float* out_val_d, int64_t* out_idx_d, void* workspace_d, size_t workspace_bytes, void* stream);
/* Full-row ranking (file-compat mode: the reference writes the whole permutation of the pool per query,
 * train_retriever.py:357-362; retrieval_data_annotation.py:88-93): perm_d int32 [rows,n] = stable argsort of -scores
 * (ties by ascending index) == np.argsort(-S, axis=1, kind='stable'); NaN last, -0.0 == +0.0.  Any n < 2^31 / 16:
 * chunks of 2048 (key, index) pairs are sorted in LDS, an element's rank is the sum of its binary-search ranks in the
 * sorted chunks of its row (O(n * n/2048 * 11) instead of O(n^2) compares).  elem_bytes = 4 (f32) or 8 (f64). */
size_t r4d_argsort_workspace_bytes(int32_t rows, int32_t n, int32_t elem_bytes);
int r4d_argsort_desc_f32(const float* scores_d, int32_t rows, int32_t n, int32_t* perm_d, void* workspace_d,
                         size_t workspace_bytes, void* stream);
int r4d_argsort_desc_f64(const double* scores_d, int32_t rows, int32_t n, int32_t* perm_d, void* workspace_d,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Jaccard pool annotation.  Replaces occurrence_matrix / co_occurrence_ratio,
 * retrieval_data_annotation.py:36-41 / :5-15, and np.fill_diagonal :172-173.
 * Sets are CSR: ptr int32 [n+1], idx int32 sorted-unique token ids in [0,vocab); *_nnz = ptr[n] = number of
 * idx elements (the idx buffers must hold at least one element even when every set is empty).
 * ---------------------------------------------------------------------------------------------- */
/* out_d f64 [na,nb] row-major: |A_i & B_j| / |A_i | B_j|, 0.0 when either set is empty;
 * zero_diag != 0 additionally writes 0.0 at i == j. */
int r4d_jaccard_f64(const int32_t* a_ptr_d, const int32_t* a_idx_d, int32_t na, int32_t a_nnz,
                    const int32_t* b_ptr_d, const int32_t* b_idx_d, int32_t nb, int32_t b_nnz,
                    int32_t vocab, int32_t zero_diag, double* out_d, void* stream);
/* The same matrix with the A rows VISITED in the order a_order_d (int32 [na], a permutation of 0..na-1; NULL = file
 * order).  Results land in their own rows; only the schedule changes: a wavefront walks the tokens of four A rows
 * jointly, to the longest of the four, so visiting rows of similar length together (longest first) saves the padding
 * steps -- 1.7x fewer token steps on log-normal input-set lengths.  Values are identical for every order.
 * DENSE TOKENS (a_dense_d / b_dense_d, both or neither; NULL = none): uint32 [na] / [nb], bit t of a set's word = "the
 * set contains dense token t".  The caller picks up to 32 tokens (the frequent ones: the <|timeK|> tokens that
 * get_input_seq keeps, retrieval_data_annotation.py:17-20) and REMOVES them from the CSR lists; the kernel adds
 * popcount(a_dense & b_dense) to the intersection and the popcounts to the set sizes: the same integers as the plain
 * CSR form, for two vector instructions per row and 64 pairs instead of 4.3 per token. */
int r4d_jaccard_ordered_f64(const int32_t* a_ptr_d, const int32_t* a_idx_d, int32_t na, int32_t a_nnz,
                            const int32_t* b_ptr_d, const int32_t* b_idx_d, int32_t nb, int32_t b_nnz,
                            int32_t vocab, int32_t zero_diag, const int32_t* a_order_d,
                            const uint32_t* a_dense_d, const uint32_t* b_dense_d, double* out_d, void* stream);
/* The same matrix with the schedule PREPARED ON THE DEVICE (round 5): the caller hands over the plain CSR sets and says
 * which of the two schedule aids it wants; nothing is computed on the host and no torch op runs.
 *   dense_split != 0: the 32 most frequent tokens -- counted over a strided sample of at most 2 x 512 sets, ties to the
 *     smaller token id -- leave the lists for one membership word per set (the a_dense_d / b_dense_d of the entry above);
 *     the remaining tokens are squeezed to the front of each set's own segment in a workspace copy of idx.
 *   sort_rows != 0: the A rows are visited longest (remaining) list first (a_order_d above; ties in no particular order).
 * Neither changes a value: out_d holds the bits r4d_jaccard_f64 writes.  The sets hold DISTINCT tokens (as
 * get_input_seq / get_target_seq build them, retrieval_data_annotation.py:17-34).  workspace_d from
 * r4d_jaccard_prepared_workspace_bytes (may be NULL when both flags are 0). */
size_t r4d_jaccard_prepared_workspace_bytes(int32_t na, int32_t a_nnz, int32_t nb, int32_t b_nnz, int32_t vocab);
int r4d_jaccard_prepared_f64(const int32_t* a_ptr_d, const int32_t* a_idx_d, int32_t na, int32_t a_nnz,
                             const int32_t* b_ptr_d, const int32_t* b_idx_d, int32_t nb, int32_t b_nnz,
                             int32_t vocab, int32_t zero_diag, int32_t dense_split, int32_t sort_rows,
                             double* out_d, void* workspace_d, size_t workspace_bytes, void* stream);
/* Per-row top-k (value descending, index ascending) of an f64 matrix: save_score_file_train,
 * retrieval_data_annotation.py:97-103 (topk=10).  ws from r4d_topk_f64_workspace_bytes. */
size_t r4d_topk_f64_workspace_bytes(int32_t rows, int32_t n, int32_t k);
int r4d_topk_f64(const double* m_d, int32_t rows, int32_t n, int32_t k, double* out_val_d,
                 int32_t* out_idx_d, void* workspace_d, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Retriever TRAINING step.  Replaces, for the encoder, what torch autograd does for the reference in
 * train/train_retriever.py:177-214: five forwards (anchor, positive, hard negative, two augmented views), loss.backward(),
 * clip_grad_norm_, AdamW.  The contrastive losses ([B,3B] / [2B,2B] similarity tables, :40-98) and their gradient on the
 * mean-pooled embeddings are r4d_retriever_losses_f32 below (round 3; a caller may still substitute its own).
 * ---------------------------------------------------------------------------------------------- */
typedef struct r4d_gpt2_layer_grads {   /* device pointers, same shapes as r4d_gpt2_layer's reference-layout tensors */
    float* ln_1_w;      float* ln_1_b;
    float* c_attn_w;    float* c_attn_b;      /* [d,3d], [3d] */
    float* attn_proj_w; float* attn_proj_b;   /* [d,d],  [d]  */
    float* ln_2_w;      float* ln_2_b;
    float* c_fc_w;      float* c_fc_b;        /* [d,4d], [4d] */
    float* mlp_proj_w;  float* mlp_proj_b;    /* [4d,d], [d]  */
} r4d_gpt2_layer_grads;
typedef struct r4d_gpt2_grads {
    float* wte;                           /* [vocab,d]        (zeroed, then scatter-added) */
    float* wpe;                           /* [n_positions,d]  (zeroed, then scatter-added) */
    float* ln_f_w;
    float* ln_f_b;
    const r4d_gpt2_layer_grads* layers;   /* HOST array [n_layer] */
} r4d_gpt2_grads;

/* nn.Dropout of the training forward (model.train(), train_retriever.py:161): embd_p after wte + wpe (modeling_gpt2.py:337,427),
 * attn_p on the attention probabilities (:153), resid_p on the two residual branches (:194, :212).  Masks come from a
 * counter-based generator (Philox-4x32-10 keyed by `seed`, counter = (element index / 4, site, step)): the SAME struct must be
 * passed to the forward and the backward call of a step; change `step` every step.  Sites: 4 * layer + {0: attention
 * probabilities, 1: attention branch, 2: MLP branch}, R4D_DROPOUT_SITE_EMBD for the embeddings; element index = offset in the
 * concatenated [rows, d] activations (rows of all batches in call order), for the probabilities the offset in the step's
 * [B*H, T, ceil128(T)] blocks laid end to end in batch order.  A null pointer (or all p == 0) is the identity (model.eval()). */
typedef struct {
    float embd_p, attn_p, resid_p;
    uint64_t seed, step;
} r4d_train_dropout;
#define R4D_DROPOUT_SITE_EMBD 65535u
/* out = (resid_d ? resid_d : 0) + dropout_p(x_d) for one site (per-op tests; the kernel the step launches).  n and
 * index_base multiples of 4; out_d may be x_d or resid_d. */
int r4d_dropout_f32(const float* x_d, const float* resid_d, int64_t n, float* out_d, float p, uint64_t seed, uint64_t step,
                    uint32_t site, uint64_t index_base, void* stream);

/* How the training steps keep the attention probabilities P (process-wide, like r4d_set_gemm_split3; additive ABI v6 entries).
 *   0 stored (default): the forward keeps P [B*H, T, ceil128(T)] of every layer and batch in the workspace;
 *   1 recompute:        no kept P -- the backward forms it again with the forward's own two launches and two fused row kernels
 *                       replace the element-wise passes around it.  Every GEMM reads the bits it reads in mode 0, so every
 *                       output and gradient is bit-identical; the workspace shrinks by (n_layer * sum P - max P) floats.
 * Any other value is R4D_ERR_INVALID.  The mode is read by the three workspace queries and by every training forward / backward /
 * step call: set it BEFORE the size query and keep it until the step's backward has been issued.  A backward on the workspace of
 * the most recent training forward under a different mode is refused (R4D_ERR_INVALID). */
int r4d_set_train_attention(int32_t mode);
int r4d_get_train_attention(void);

/* How the training steps keep the per-layer activations (process-wide; additive ABI v6 entries, independent of the switch above).
 *   0 stored (default): the forward keeps x_in, ln1, qkv, att, x_mid, ln2, pre, f of every layer (16 * rows * d floats each);
 *   1 recompute:        the forward keeps each layer's input x_in (and layer 0's ln1); ln1 .. f -- and, under stored attention,
 *                       ONE P block -- are a single set that all layers share.  The backward walks the layers downwards and,
 *                       ahead of each layer's backward, runs that layer's forward launches from ln_1 to c_fc (+ GELU) again on
 *                       x_in with the forward's arguments and dropout sites.  The same launches on the same bits: every output
 *                       and gradient is bit-identical to mode 0.  The weights, the token ids and the dropout descriptor must be
 *                       those of the forward until the backward has been issued (the three step calls guarantee it).
 * Any other value is R4D_ERR_INVALID and changes nothing.  Read like the attention mode: set it BEFORE the size query and keep it
 * until the step's backward has been issued; a backward on the workspace of the most recent training forward under a different
 * mode is refused (R4D_ERR_INVALID). */
int r4d_set_train_activations(int32_t mode);
int r4d_get_train_activations(void);

/* Mixed-precision training: plain bf16 operands for the twelve Conv1D GEMMs of every transformer block (process-wide; additive
 * ABI v6 entries; csrc/gemm_b1.hip, csrc/gemm_b1tn.hip).  NOT fp32-accurate: each operand of those GEMMs is rounded to bf16 (8
 * significant bits, round to nearest even) and multiplied ONCE on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.
 *   forward        y  = epilogue(RN(x) . RN(W) + b)          plane 0 of *_w3  (RN(W) as [out][in])
 *   data gradient  dx = RN(dy) . RN(W)^T                     plane 0 of *_w3t (RN(W) as [in][out])
 *   weight grad.   dW = RN(x)^T . RN(dy),  db = column sums of the UNROUNDED dy
 * Master weights, gradients, the optimizer, LayerNorm, softmax, GELU, the losses, the embedding scatter and every accumulator stay
 * fp32; the attention GEMMs stay exact f32 (their own switch: r4d_set_train_attention_bf16 below); the LM head's three GEMMs
 * read a switch of their own (r4d_set_train_head_bf16 below) and not this one; r4d_weight_grad_f32, the GCN projection of the RAG step
 * and every encoder / decode entry read none of the three.  A layer GEMM is switched in EVERY gemm mode (f32 included) whenever
 * the layer carries the plane and the shape is supported (K % 32 == 0; weight gradient: in % 128 == 0, out % 256 == 0, rows >=
 * 32); anything else keeps the gemm mode's kernel.  Only plane 0 of the plane sets is read by the switched GEMMs.
 * r4d_set_train_bf16(on != 0) returns the previous setting; default 0.  Read once by the three workspace queries and by every
 * training forward / backward / step call: set it BEFORE the size query and keep it until the step's backward has been issued.  A
 * backward on the workspace of the most recent training forward under the other setting is refused (R4D_ERR_INVALID): under
 * activation recompute its re-forward would differ from the forward. */
int r4d_set_train_bf16(int32_t on);
int r4d_get_train_bf16(void);
/* The single ops of that mode, exported for per-op tests and tools (the kernels the step launches; not read by the switch).
 * r4d_conv1d_bf16_keep_f32: the c_fc forward: pre_d [M,N] = RN(x) . W + b (the kept pre-activation), y_d [M,N] = gelu_new(pre).
 * r4d_conv1d_bf16_dgrad_f32: dx_d [M,in] = RN(dy_d [M,out]) . wt_bf16_d^T with wt_bf16_d [in][out] = plane 0 of the layer's *_w3t;
 *   kind 0 none, 1 dx = second_d + ..., 2 dx = (...) * gelu_new'(second_d) (second_d [M,in]).  out % 32 == 0.
 * r4d_weight_grad_bf16_f32: dw_d [in,out] = RN(x)^T . RN(dy), db_d [out] (nullable, 16-byte aligned) = column sums of dy, for
 *   x_d [rows, in] with row stride ldx and dy_d [rows, out] with row stride ldy (floats, multiples of 4, >= in / out).  in % 128
 *   == 0, out % 256 == 0, rows >= 32, else R4D_ERR_INVALID and nothing is launched (the size query returns 0).  The contraction
 *   is split over slices whose fp32 partials the workspace holds; they are written before they are summed, in slice order: the
 *   same bits on every run, whatever the workspace held. */
int r4d_conv1d_bf16_keep_f32(const float* x_d, const uint16_t* w_bf16_d /* [N][K] */, const float* bias_d, int32_t M, int32_t K,
                             int32_t N, float* pre_d, float* y_d, void* stream);
int r4d_conv1d_bf16_dgrad_f32(const float* dy_d, const uint16_t* wt_bf16_d /* [in][out] */, int32_t M, int32_t in_features,
                              int32_t out_features, int32_t kind, const float* second_d, float* dx_d, void* stream);
size_t r4d_weight_grad_bf16_workspace_bytes(int32_t rows, int32_t in_features, int32_t out_features);
int r4d_weight_grad_bf16_f32(const float* x_d, int32_t ldx, const float* dy_d, int32_t ldy, int32_t rows, int32_t in_features,
                             int32_t out_features, float* dw_d, float* db_d, void* workspace_d, size_t workspace_bytes, void* stream);

/* The attention products of the training steps on plain bf16 operands (process-wide; additive ABI v6 entries; csrc/gemm_b1h.hip).
 * A second, INDEPENDENT axis beside r4d_set_train_bf16, whose meaning and return values it leaves alone.  NOT fp32-accurate: while
 * on, both fp32 operands of the six per-head products of every block are rounded to bf16 (round to nearest even) where they are
 * staged and multiplied ONCE on v_mfma_f32_32x32x16_bf16 with fp32 accumulation in a fixed order:
 *   0  S  = RN(Q) . RN(K)^T / sqrt(hd)   (tiles above the diagonal skipped)      3  dQ = RN(dS) . RN(K)
 *   1  O  = RN(P) . RN(V)                (trimmed to the keys a row tile sees)   4  dK = RN(dS^T) . RN(Q)
 *   2  dP = RN(dO) . RN(V)^T                                                     5  dV = RN(Pd^T) . RN(dO)
 * in stored and recompute attention alike.  The scale division acts on the fp32 accumulator; softmax, its backward, dropout, the
 * transposes, P and every other buffer stay fp32, and nothing outside the training steps reads the switch.
 * r4d_set_train_attention_bf16(on != 0) returns the previous setting; default 0.  Read like r4d_set_train_bf16: set it BEFORE the
 * size query (the sizes do not depend on it) and keep it until the step's backward has been issued; a backward on the workspace of
 * the most recent training forward under the other setting is refused (R4D_ERR_INVALID). */
int r4d_set_train_attention_bf16(int32_t on);
int r4d_get_train_attention_bf16(void);
/* ONE of the six products above (which = 0 .. 5) over a [B, T] batch with H heads of d / H columns, for per-product tests and tools:
 * the launch the step issues, whatever the switch says.  a_d / b_d / c_d point at the first element of the (sequence 0, head 0)
 * block in the step's layouts: a Q / K / V slice of [B, T, 3d] (row stride 3d), merged heads [B, T, d], or a P-shaped block
 * [B*H, T, ld] with ld = r4d_train_attn_probs_ld(T) floats (T rounded up to 128):
 *   which   a_d            b_d          c_d              which   a_d             b_d           c_d
 *   0       Q slice        K slice      P-shaped         3       P-shaped dS     K slice       Q slice of dqkv
 *   1       P-shaped       V slice      merged           4       P-shaped dS^T   Q slice       K slice of dqkv
 *   2       merged dO      V slice      P-shaped         5       P-shaped Pd^T   merged dO     V slice of dqkv
 * Of a P-shaped OPERAND only columns [0, T) of its T rows are used, of every other operand only its T rows and its head's d / H
 * columns; whatever else that memory holds (NaN included) reaches no product.  Only C's [T, N] block per (sequence, head) is
 * written (product 0: the tiles that touch the lower triangle; the rest is the softmax's to fill).  head_dim % 16 == 0, T <= 1024,
 * B * H <= 65535; operands 16-byte aligned. */
size_t r4d_train_attn_probs_ld(int32_t T);
int r4d_train_attn_product_bf16_f32(int32_t which, const float* a_d, const float* b_d, float* c_d, int32_t B, int32_t T, int32_t H,
                                    int32_t d, void* stream);

/* FUSED attention of the training steps: no [T, T] block in memory (process-wide; additive ABI v6 entries;
 * csrc/attention_train_fused.hip).  A seventh switch.  It acts only TOGETHER with r4d_set_train_attention_bf16 -- the
 * arithmetic is that switch's: Q, K, V, dO, the probabilities and dS enter every product as bf16 (round to nearest even), one
 * v_mfma_f32_32x32x16_bf16 per k-step, fp32 accumulation, the softmax and dS arithmetic in fp32.  NOT fp32-accurate, and NOT
 * bit-identical to the six products: the forward rounds the UNNORMALISED probabilities exp(s - running max) and divides the
 * accumulated O by the row sum afterwards; the backward forms P = exp(s - lse) again, from the forward's row statistics.  While both switches are on
 *   - the forward writes att [B, T, d] and ONE fp32 log-sum-exp per (sequence, head, query), lse [B*H, T], per layer (one shared set
 *     under activations recompute, whose re-forward leaves the forward's bits);
 *   - the backward is three launches per batch (row sums D, dK / dV, dQ) that write this head's columns of dqkv [B, T, 3d];
 *   - the layout holds NO P block and none of the three P-shaped scratch blocks: the three size queries shrink accordingly, and
 *     r4d_set_train_attention (stored / recompute) changes neither a size nor a launch;
 *   - dropout on the probabilities drops exactly the elements the unfused step drops under the same r4d_train_dropout.
 * With this switch on and r4d_set_train_attention_bf16 off the three size queries return 0 and every training forward / backward /
 * step entry fails with R4D_ERR_INVALID ("train-attention-fused needs train-attention-bf16") before any launch.
 * r4d_set_train_attention_fused(0 | 1) returns R4D_OK; any other value is R4D_ERR_INVALID and changes nothing; default 0 (every
 * launch, size and bit as without these entries).  Read like r4d_set_train_bf16: set it BEFORE the size query and keep it until the
 * step's backward has been issued; a backward on the workspace of the most recent training forward under the other setting is
 * refused (R4D_ERR_INVALID).  Nothing outside the training steps reads it. */
int r4d_set_train_attention_fused(int32_t on);
int r4d_get_train_attention_fused(void);
/* The two launch sequences of that mode over ONE batch [B, T] with H heads, for per-op tests and tools (whatever the switches say).
 * qkv_d [B, T, 3d], att_d / dao_d [B, T, d] merged heads, lse_d [B*H, T], dqkv_out_d [B, T, 3d]; only the T rows' own-head columns
 * of the outputs are written, and nothing else of the inputs is read.  dropout: NULL or attn_p == 0 -> none; else the mask of
 * element (bh, i, j) is r4d_dropout_f32's at `site`, dropout->seed / step and index_base + (bh * T + i) * r4d_train_attn_probs_ld(T) + j
 * (index_base % 4 == 0).  The backward's workspace holds D [B*H, T] = rowsum(P o dP) (r4d_train_attn_fused_bwd_workspace_bytes; written before it
 * is read); att_d is part of the contract (the forward's output, non-null) and is not read.  head_dim % 16 == 0 in 16 .. 256, T in 1 .. 1024, B * H <= 65535, pointers 16-byte aligned; anything else is
 * R4D_ERR_INVALID (a short workspace: R4D_ERR_WORKSPACE) before any launch, and the size query returns 0. */
int r4d_train_attn_fused_fwd_f32(const float* qkv_d, int32_t B, int32_t T, int32_t H, int32_t d, float* att_out_d, float* lse_out_d,
                                 const r4d_train_dropout* dropout, uint32_t site, uint64_t index_base, void* stream);
size_t r4d_train_attn_fused_bwd_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t d);
int r4d_train_attn_fused_bwd_f32(const float* qkv_d, const float* att_d, const float* lse_d, const float* dao_d, int32_t B, int32_t T,
                                 int32_t H, int32_t d, float* dqkv_out_d, const r4d_train_dropout* dropout, uint32_t site,
                                 uint64_t index_base, void* workspace_d, size_t workspace_bytes, void* stream);

/* The LM head of the training steps on plain bf16 operands (process-wide; additive ABI v6 entries; csrc/lm_head.hip on
 * csrc/gemm_b1.hip and csrc/gemm_b1tn.hip).  A third, INDEPENDENT axis beside r4d_set_train_bf16 and r4d_set_train_attention_bf16: it
 * neither reads nor sets them, and they do not read it.  NOT fp32-accurate: while on, both fp32 operands of the head's three GEMMs
 * are rounded to bf16 (round to nearest even) where they are staged and multiplied ONCE on v_mfma_f32_32x32x16_bf16 with fp32
 * accumulation in a fixed order, per vocabulary chunk k of the r4d_lm_head operand -- rows [c0, c0 + Ck) of wte_pad; one chunk when ldV <= 15872:
 *   logits_k             = RN(h) . RN(wte_k)^T           plane 0 of the chunk's w3  (RN(wte_k) as [Ck][d])
 *   dh (+)=                RN(dlogits_k) . RN(wte_k)     plane 0 of the chunk's w3t (RN(wte_k) as [d][Ck]); chunks added in ascending order
 *   dwte[c0 : c0 + Ck]   = RN(dlogits_k)^T . RN(h)       no plane: both operands are rounded on the fly
 * The logits and their gradient in memory, the cross entropy, dh, dwte, the tied add into grads->wte and the master weights stay
 * fp32.  Only plane 0 of w3 / w3t is read, in the chunk layout r4d_lm_head describes; the planes are used in EVERY gemm mode (exact
 * f32 included) while the switch is on, and change no route while it is off.  Each product falls back on its own to the gemm mode's
 * kernel ("anything else keeps the gemm mode's kernel"): logits without w3 or with d % 32 != 0; dh without w3t or with B*T * Ck >= 2^29;
 * dwte with d % 256 != 0, fewer than 32 rows, or (B*T + 64) * Ck >= 2^29.  Both sweeps of the chunked head form a chunk's logits by the
 * same launch, so the gradient comes from the logits the statistics came from; no float atomics: the same bits on every launch.
 * A loss-only step call (grads == NULL && d_fused_d == NULL, the evaluation loss) reads the switch like any other: its loss equals
 * the training call's on the same inputs bit for bit, and differs from the loss with the switch off.
 * r4d_set_train_head_bf16(on != 0) returns the previous setting; default 0.  Read once at the top of r4d_gpt2_lm_train_step_f32,
 * r4d_rag_train_step_f32 and r4d_lm_head_train_f32; the workspace sizes do NOT depend on it (gemm_b1tn cuts its slices to the room
 * the gemm mode's weight gradient is given), so the size queries do not read it.  The retriever step has no LM head and does not read
 * it; nothing outside the training steps reads it (r4d_lm_logits_f32, the encoder and the decode step included). */
int r4d_set_train_head_bf16(int32_t on);
int r4d_get_train_head_bf16(void);

/* The saved activations of the bf16 training steps kept as bf16 in memory (process-wide; additive ABI v6 entries; csrc/train.hip,
 * csrc/gemm_b1.hip, csrc/gemm_b1tn.hip, csrc/encoder_ops.hip).  A fifth switch; it acts ONLY while r4d_set_train_bf16 is on, and
 * with that switch off it changes no byte of the layout and no launch.  While both are on, per transformer block
 *   ln1 [M, d]  (layers >= 1)   the LayerNorm output that c_attn and its weight gradient read
 *   ln2 [M, d]                  the LayerNorm output that c_fc and its weight gradient read
 *   f   [M, 4d]                 gelu_new(pre), which the MLP projection and its weight gradient read
 * are written by their producers as bf16 [M, width] (round to nearest even, the rounding gemm_b1 / gemm_b1tn apply to the fp32 form
 * while they stage it) and read by those GEMMs as a bf16 operand: the GEMMs form the operand bits they form with the switch off, so
 * every loss, output and gradient is BIT-IDENTICAL to the step with the switch off, and the accuracy statement of r4d_set_train_bf16
 * holds unchanged.  No launch is added or removed.  A block is bf16 where its shape qualifies -- d % 256 == 0, M >= 32 rows in the
 * step, and both consumers' shape contracts -- and stays fp32 otherwise (at d 64 nothing changes); where it qualifies the layer must
 * carry the consumer's *_w3 planes (R4D_ERR_INVALID from the forward otherwise).  Layer 0's ln1, att, x_in, x_mid, pre, qkv, P and
 * every gradient stay fp32.  The workspace of the three size queries shrinks by (12 * n_layer - 2) * M * d bytes in stored
 * mode, and by 10 * M * d (+ 2 * M * d when n_layer >= 2) bytes under activations recompute.
 * r4d_set_train_act_bf16(0 | 1) returns the previous setting; default 0; any other value is R4D_ERR_INVALID and changes nothing.
 * Read like r4d_set_train_bf16: set it BEFORE the size query and keep it until the step's backward has been issued; a backward on the
 * workspace of the most recent training forward under the other setting is refused (R4D_ERR_INVALID). */
int r4d_set_train_act_bf16(int32_t on);
int r4d_get_train_act_bf16(void);
/* The single ops of that store, for per-op tests and tools (the kernels the step launches; not read by the switch).
 * r4d_layernorm_bf16_f32: y_bf16_d [rows, d] = RN(LayerNorm(x)) with r4d_layernorm_f32's statistics; d % 256 == 0, 16-byte aligned.
 * r4d_conv1d_bf16_act_f32: r4d_conv1d_bf16_f32 on x_bf16_d [M, K] bf16 (K % 32 == 0).  kind 0: y_d f32 [M,N]; 1: y_d = second_d + ...;
 *   2: second_d f32 [M,N] <- the pre-activation, y_d bf16 [M,N] <- RN(gelu_new(pre)) (N even).
 *   The encoder's r4d_set_encode_act_bf16 adds two kinds without a second buffer (second_d ignored), N even:
 *   3: y_d bf16 [M,N] <- RN(gelu_new(v)), no pre-activation kept (c_fc); 4: y_d bf16 [M,N] <- RN(v) (c_attn under bf16 attention).
 * r4d_weight_grad_bf16_act_f32: r4d_weight_grad_bf16_f32 on x_bf16_d [rows, in] bf16 with row stride ldx (bf16 elements, a multiple
 *   of 8); the same workspace (r4d_weight_grad_bf16_workspace_bytes). */
int r4d_layernorm_bf16_f32(const float* x_d, const float* w_d, const float* b_d, int32_t rows, int32_t d, float eps,
                           uint16_t* y_bf16_d, void* stream);
int r4d_conv1d_bf16_act_f32(const uint16_t* x_bf16_d, const uint16_t* w_bf16_d /* [N][K] */, const float* bias_d, int32_t M, int32_t K,
                            int32_t N, int32_t kind, float* second_d, void* y_d, void* stream);
int r4d_weight_grad_bf16_act_f32(const uint16_t* x_bf16_d, int32_t ldx, const float* dy_d, int32_t ldy, int32_t rows,
                                 int32_t in_features, int32_t out_features, float* dw_d, float* db_d, void* workspace_d,
                                 size_t workspace_bytes, void* stream);

/* Scratch of one step: the activations the backward pass needs (16 * rows * d floats per layer + the attention
 * probabilities in stored mode) and the backward temporaries.  The SAME buffer goes to the forward and to the backward call. */
size_t r4d_gpt2_train_workspace_bytes(const r4d_gpt2_config* cfg, int32_t n_groups, const int32_t* Bs, const int32_t* Ts);
/* Forward over up to 16 right-padded id batches (one launch sequence over their concatenated rows) that keeps every
 * activation the backward pass reads.  The optional wT copies of the layers are USED when present (faster forward GEMMs): the
 * caller must refresh them after every optimizer step; the backward pass reads the reference layout only.  out_meanpool_d f32 [sum(Bs), d] = torch.mean(h, dim=1) per sequence. */
int r4d_gpt2_train_forward_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, int32_t n_groups,
                               const int64_t* const* ids_d, const int32_t* Bs, const int32_t* Ts, float* out_meanpool_d,
                               const r4d_train_dropout* dropout, void* workspace_d, size_t workspace_bytes, void* stream);
/* Backward of the call above (same arguments, same workspace contents): d_meanpool_d f32 [sum(Bs), d] = dLoss / d(embeddings)
 * -> every gradient of `grads` is OVERWRITTEN with dLoss / d(parameter) (lm_head is not on this path: the retriever discards
 * the logits, train_retriever.py:177-179). */
int r4d_gpt2_train_backward_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_gpt2_grads* grads,
                                int32_t n_groups, const int64_t* const* ids_d, const int32_t* Bs, const int32_t* Ts,
                                const float* d_meanpool_d, const r4d_train_dropout* dropout,
                                void* workspace_d, size_t workspace_bytes, void* stream);
/* The step's loss head on the device (train/train_retriever.py:40-98,196): emb_d f32 [5,B,d] = the mean-pooled embeddings of
 * anchors, positives, hard negatives and the two augmented views (r4d_gpt2_train_forward_f32's output); t_*_d f32 [B] the query
 * times of the three sequence families.  losses_d f32[3] <- { CLtime_loss, alpha * info_nce, their sum };  d_emb_d (nullable)
 * f32 [5,B,d] <- grad_scale * d(sum)/d(emb): what r4d_gpt2_train_backward_f32 takes as d_meanpool_d.  Fixed summation order
 * (the same bits on every launch and rank).  cosine_similarity clamps each norm at 1e-8 like torch. */
size_t r4d_retriever_losses_workspace_bytes(int32_t B);
int r4d_retriever_losses_f32(const float* emb_d, const float* t_anchor_d, const float* t_pos_d, const float* t_neg_d, int32_t B,
                             int32_t d, float temperature, float lambda_decay, float alpha, float grad_scale, float* losses_d,
                             float* d_emb_d, void* workspace_d, size_t workspace_bytes, void* stream);
/* ------------------------------------------------------------------------------------------------
 * SimpleDyG LM TRAINING (additive ABI v6 entries): the LM head logits = h . wte^T over every position, the shifted cross
 * entropy of models/modeling_gpt2.py:604-615 (labels == inputs) and its gradient back into the tied wte and into h.
 * ---------------------------------------------------------------------------------------------- */
/* r4d_gpt2_train_forward_f32 / _backward_f32 with a per-row output: out_hidden_d f32 [sum(Bs*Ts), d] = the ln_f output of every
 * position (rows of all batches in call order); the backward takes d_hidden_d of the same shape.  Same workspace query. */
int r4d_gpt2_train_forward_hidden_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, int32_t n_groups,
                                      const int64_t* const* ids_d, const int32_t* Bs, const int32_t* Ts, float* out_hidden_d,
                                      const r4d_train_dropout* dropout, void* workspace_d, size_t workspace_bytes, void* stream);
int r4d_gpt2_train_backward_hidden_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_gpt2_grads* grads,
                                       int32_t n_groups, const int64_t* const* ids_d, const int32_t* Bs, const int32_t* Ts,
                                       const float* d_hidden_d, const r4d_train_dropout* dropout,
                                       void* workspace_d, size_t workspace_bytes, void* stream);
/* Fused shifted cross entropy over logits_d f32 [N, ldV] (N = B*T rows, columns [V, ldV) padding, ldV % 4 == 0, V <= ldV).
 * Label of row (b, t): src[b, t + 1] with src = labels_d when given (int64 [B, T]) else ids_d (int64 [B, T]); row t = T - 1 has
 * none; a label outside [0, V) (ignore_index -100) is not counted; any other such label also raises R4D_RANGE_BAD_LABEL.  loss_d f32[1] <- mean over the counted rows (the count is
 * taken on the device: NaN when no row counts, as torch); logits_d is OVERWRITTEN with grad_scale * (softmax - onehot) / n_counted,
 * exact zeros in uncounted rows and pad columns.  Fixed-order sums: the same bits on every launch.
 * ldV <= 15872: one launch, the row staged in LDS.  Larger ldV: the row is walked in column ranges of r4d_lm_head_chunk_rows(ldV)
 * columns -- one launch per range folds its max and sum of exponentials into the row's running pair (an online softmax), one
 * launch per range writes the gradient; the workspace (the same query, whatever ldV) carries the rows' (max, sum, label logit). */
size_t r4d_lm_ce_workspace_bytes(int32_t N);
int r4d_lm_ce_f32(float* logits_d, int32_t N, int32_t V, int32_t ldV, const int64_t* ids_d, const int64_t* labels_d, int32_t T,
                  float grad_scale, float* loss_d, void* workspace_d, size_t workspace_bytes, void* stream);
/* The tied LM head operand: wte_pad_d f32 [ldV, d] = wte in rows [0, V), ZERO rows up to ldV (ldV = V rounded up to 128); the
 * optional planes of it (r4d_split3_planes_bf16 / r4d_split2_planes_f16 of wte_pad_d): w3_d [3][ldV][d] (transposed = 1) and
 * h2_d [ldV][d/32][2][32] for the logits GEMM, w3t_d [3][d][ldV] (wte_pad_d as a [K = ldV, N = d] weight, transposed = 0) for
 * dh = dlogits . wte.  Refresh them with the layer planes after every optimizer step.
 * ldV > 15872 (the chunked head): with C = r4d_lm_head_chunk_rows(ldV), chunk k holds the rows [k C, k C + Ck) of wte_pad_d,
 * Ck = min(C, ldV - k C) (the last chunk may be shorter; still a multiple of 128).  wte_pad_d and h2_d are row-major over the
 * vocabulary rows and stay as above; w3_d and w3t_d are laid CHUNK BY CHUNK, chunk k at element offset 3 * k C * d:
 *   w3_d  chunk k: [3][Ck][d] = r4d_split3_planes_bf16(wte_pad_d + k C d, K = d,  N = Ck, transposed = 1)
 *   w3t_d chunk k: [3][d][Ck] = r4d_split3_planes_bf16(wte_pad_d + k C d, K = Ck, N = d,  transposed = 0)
 * so the total sizes are unchanged.  ldV <= 15872 is the one-chunk case of the same rule (C = ldV). */
int32_t r4d_lm_head_chunk_rows(int32_t ldV);       /* ldV when ldV <= 15872, else the library's chunk rows C (C % 128 == 0, C <= 15872) */
typedef struct {
    const float* wte_pad;
    int32_t ldV;
    const uint16_t* w3;
    const uint16_t* w3t;
    const uint16_t* h2;
} r4d_lm_head;
/* One SimpleDyG training step on one right-padded id batch ids_d int64 [B, T] (labels == inputs): forward_hidden -> logits (the
 * forward GEMM family of the current r4d_set_gemm_split3 mode) -> r4d_lm_ce_f32 -> dh = dlogits . wte (bf16x3 like every data
 * gradient) and dwte_head = dlogits^T . h (the weight-gradient GEMM) -> backward_hidden (the three head GEMMs on plain bf16 under
 * r4d_set_train_head_bf16).  grads->wte = embedding scatter +
 * dwte_head, added in that fixed order.  loss_d f32[1] stays on the device.  grad_scale scales every gradient (1 / accumulation
 * steps), not the loss.
 * ldV > 15872: the logits exist one vocabulary chunk [B*T, C] at a time (r4d_lm_head above): a first sweep over the chunks forms
 * the loss, a second forms each chunk's logits again and feeds dh and dwte_head.  The workspace holds one chunk of logits, so
 * beyond dwte_head [ldV, d] it does not grow with V.  B*T * C and ldV * d must stay below 2^31 (R4D_ERR_INVALID otherwise). */
size_t r4d_gpt2_lm_train_workspace_bytes(const r4d_gpt2_config* cfg, int32_t B, int32_t T, int32_t ldV);
int r4d_gpt2_lm_train_step_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_gpt2_grads* grads,
                               const r4d_lm_head* head, const int64_t* ids_d, int32_t B, int32_t T, float grad_scale, float* loss_d,
                               const r4d_train_dropout* dropout, void* workspace_d, size_t workspace_bytes, void* stream);
/* The head of the two steps alone, for per-op tests and tools: exactly the call they make, in the current r4d_set_gemm_split3 mode and
 * r4d_set_train_head_bf16 setting.  h_d f32 [N, d] (N = B * T rows: the ln_f output); labels_src_d int64 [N]: the label of row r is
 * labels_src_d[r + 1] within a sequence of T rows (the last row of a sequence has none; -100 is not counted), as in r4d_lm_ce_f32.
 * loss_d f32[1] <- the mean over the counted rows; dh_d (nullable) f32 [N, d] <- grad_scale * dLoss/dh; dwte_d (nullable) f32
 * [ldV, d] <- grad_scale * dlogits^T . h (rows [V, ldV) exact zeros).  dh_d == dwte_d == NULL: loss only, the same loss bits.
 * ldV % 128 == 0, ldV >= V, d % 4 == 0, N % T == 0; N * r4d_lm_head_chunk_rows(ldV), ldV * d and N * d below 2^31; every pointer
 * 16-byte aligned.  The workspace size depends on neither switch.  On return the workspace BEGINS with the last chunk's dlogits f32
 * [N, Ck] (the whole [N, ldV] gradient of the logits when ldV <= 15872; after a loss-only call of the chunked head: that chunk's
 * logits), for tests that want the device's own operand of dh and dwte. */
size_t r4d_lm_head_train_workspace_bytes(int32_t N, int32_t d, int32_t ldV);
int r4d_lm_head_train_f32(const float* h_d /* [N,d] */, int32_t N, int32_t V, int32_t d, const r4d_lm_head* head,
                          const int64_t* labels_src_d, int32_t T, float grad_scale, float* loss_d, float* dh_d /* nullable */,
                          float* dwte_d /* nullable, [ldV,d] */, void* workspace_d, size_t workspace_bytes, void* stream);
/* ------------------------------------------------------------------------------------------------
 * RAG generator training (train/train_generator.py, utils/model.py:105-224; csrc/rag_train.hip).  One step on a SPLICED batch:
 * aug_ids_d int64 [B, Ta] holds the token ids with -100 at the r fused positions 2 .. 2 + r - 1 of every sequence (Ta = T + r);
 * the input rows there are fused_d f32 [B, r, d] instead of wte rows.  aug_ids_d is also the label array of the shifted cross
 * entropy (ignore_index -100) and the index array of the wte scatter (negative ids add nothing).
 *   grads == NULL: the transformer is FROZEN -- no weight GEMM, no LayerNorm gain / shift sums, no embedding scatter; the data
 *                  gradients still run down to the embeddings.
 *   head_mode:     where dW_head = dlogits^T . h goes: R4D_HEAD_GRAD_UNTIED -> head_grad_d f32 [V, d] (overwritten);
 *                  R4D_HEAD_GRAD_TIED -> added into grads->wte after the token scatter; R4D_HEAD_GRAD_NONE -> nowhere.
 *                  `head` is the padded operand of the head in use (lm_head.weight when untied), as r4d_lm_head describes.
 *   d_fused_d:     (nullable) f32 [B, r, d] <- the gradient of the spliced rows (behind the embedding dropout's mask).
 *   hidden_out_d:  (nullable) f32 [B * Ta, d] <- the ln_f output rows (the logits are overwritten by their gradient).
 * grads == NULL and d_fused_d == NULL: forward and loss only (the evaluation loss).  loss_d f32[1] stays on the device;
 * grad_scale scales every gradient, not the loss.  Same bits on every launch. */
#define R4D_HEAD_GRAD_UNTIED 0
#define R4D_HEAD_GRAD_TIED 1
#define R4D_HEAD_GRAD_NONE 2
size_t r4d_rag_train_workspace_bytes(const r4d_gpt2_config* cfg, int32_t B, int32_t Ta, int32_t ldV);
int r4d_rag_train_step_f32(const r4d_gpt2_config* cfg, const r4d_gpt2_weights* w, const r4d_gpt2_grads* grads, const r4d_lm_head* head,
                           int32_t head_mode, float* head_grad_d, const int64_t* aug_ids_d, const float* fused_d, int32_t B, int32_t Ta,
                           int32_t r, float grad_scale, float* loss_d, float* d_fused_d, float* hidden_out_d,
                           const r4d_train_dropout* dropout, void* workspace_d, size_t workspace_bytes, void* stream);
/* Weighted bags (the one-layer GCN's mean pool, c^T X): out_d f32 [n_bags, d] row q = sum over j in [offsets_d[q], offsets_d[q+1])
 * of weights_d[j] * table_d[ids_d[j]], j ascending per a fixed split; d % 4 == 0.  No atomics. */
int r4d_weighted_bag_f32(const float* table_d, int32_t vocab, int32_t d, const int64_t* ids_d, const float* weights_d,
                         const int32_t* offsets_d, int32_t n_bags, float* out_d, void* stream);
/* Deterministic scatter into a token table: out_d f32 [vocab, d] (OVERWRITTEN) row v = sum over k with ids_d[k] == v of
 * weights_d[k] * src_d[row_of_d[k]] (weights_d NULL: 1; row_of_d NULL: row k), through a 64-bit fixed-point table whose scale
 * follows max |term| (the embedding backward's sums): the same bits whatever the order.  A NaN / Inf term makes out_d NaN. */
size_t r4d_embedding_scatter_workspace_bytes(int32_t vocab, int32_t d);
int r4d_embedding_scatter_f32(const float* src_d, const int32_t* row_of_d, const float* weights_d, const int64_t* ids_d, int32_t n,
                              int32_t d, int32_t vocab, float* out_d, void* workspace_d, size_t workspace_bytes, void* stream);
/* Single backward ops, exported for per-op parity tests (the kernels the step launches). */
/* Conv1D parameter gradients (modeling_utils.py:1267-1271 under autograd): dw_d [in,out] = x^T . dy, db_d [out] (nullable) =
 * column sums of dy, for x_d [rows,in] and dy_d [rows,out]; in / out multiples of 4. */
size_t r4d_weight_grad_workspace_bytes(int32_t rows, int32_t in_features, int32_t out_features);
int r4d_weight_grad_f32(const float* x_d, const float* dy_d, int32_t rows, int32_t in_features, int32_t out_features, float* dw_d,
                        float* db_d, void* workspace_d, size_t workspace_bytes, void* stream);
size_t r4d_layernorm_bwd_workspace_bytes(int32_t rows, int32_t d);
/* dx = dLayerNorm/dx (+ add_d when given; add_d may be dx_d), dw / db = gains' and shifts' gradients (overwritten). */
int r4d_layernorm_bwd_f32(const float* x_d, const float* w_d, const float* dy_d, const float* add_d, int32_t rows, int32_t d,
                          float eps, float* dx_d, float* dw_d, float* db_d, void* workspace_d, size_t workspace_bytes,
                          void* stream);
int r4d_gelu_new_f32(const float* pre_d, int64_t n, float* y_d, void* stream);                     /* modeling_gpt2.py:25 */
int r4d_gelu_new_bwd_f32(const float* pre_d, const float* dy_d, int64_t n, float* dx_d, void* stream);   /* dx may be dy */
/* p_d [nbh,T,ld] causal probabilities (zero right of the diagonal), dp_d [nbh,T,ld] = dLoss/dP on entry and
 * dLoss/d(raw Q.K^T logits) on return (the logits were divided by scale_div before the softmax, modeling_gpt2.py:143);
 * columns right of the diagonal are written as zero. */
int r4d_causal_softmax_bwd_f32(const float* p_d, float* dp_d, int32_t nbh, int32_t T, int32_t ld, float scale_div, void* stream);
/* The two row kernels of r4d_set_train_attention(1), exported like the ops above.  p_d [nbh,T,ld] as above, ld % 32 == 0,
 * ld <= 1024; the dropout mask of element (bh, i, j) is that of r4d_dropout_f32 at index_base + (bh * T + i) * ld + j (attn_p == 0:
 * the identity); index_base % 4 == 0.
 * (a) dp_d <- dS = softmax backward of (mask * dp_d / (1 - attn_p)), in place, zeros right of the diagonal up to ld;
 *     dst_d [nbh,T,ld] <- its transpose: row j holds dS[.][j] in columns [0, T) and zeros in [T, ld).
 * (b) out_d [nbh,T,ld] <- the transpose of mask * p_d / (1 - attn_p), zeros in columns [T, ld); p_d 16-byte aligned. */
int r4d_softmax_dropout_bwd_transpose_f32(const float* p_d, float* dp_d, float* dst_d, int32_t nbh, int32_t T, int32_t ld, float scale_div,
                                          float attn_p, uint64_t seed, uint64_t step, uint32_t site, uint64_t index_base, void* stream);
int r4d_dropout_transpose_f32(const float* p_d, float* out_d, int32_t nbh, int32_t T, int32_t ld, float attn_p, uint64_t seed,
                              uint64_t step, uint32_t site, uint64_t index_base, void* stream);
/* accum_d[0] += sum x^2 (total gradient norm of clip_grad_norm_, train_retriever.py:210; zero accum_d[0] first).  accum_d is
 * f32[R4D_SUMSQ_FLOATS]: element 0 the running total, the rest scratch of the two-stage sum (no atomics: the same bits on
 * every data-parallel rank). */
#define R4D_SUMSQ_FLOATS 1025
int r4d_sumsq_accumulate_f32(const float* x_d, int64_t n, float* accum_d, void* stream);
/* One transformers.AdamW update of a flat tensor (utils/model.py:80-93; decoupled weight decay applied after the step,
 * bias correction on): step >= 1 is the update count; grad_sumsq_d (nullable) with max_grad_norm > 0 clips the gradient
 * by min(1, max_grad_norm / (sqrt(sum) + 1e-6)) on the fly (torch.nn.utils.clip_grad_norm_). */
int r4d_adamw_step_f32(float* p_d, const float* g_d, float* m_d, float* v_d, int64_t n, double lr, double beta1, double beta2,
                       double eps, double weight_decay, int32_t step, const float* grad_sumsq_d, float max_grad_norm,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * Measurement hooks (bench.py): when enabled, every kernel launch is bracketed by HIP events on the
 * launch stream and accumulated per kernel class together with its ALGORITHMIC work (flop for the
 * MFMA-bound classes, bytes for the HBM-bound ones; definitions in DESIGN.md).  Off by default;
 * not graph-capturable while on.
 * ---------------------------------------------------------------------------------------------- */
int r4d_profile_enable(int32_t on);          /* also clears the accumulated records */
int r4d_profile_num_classes(void);
const char* r4d_profile_class_name(int32_t cls);
/* Synchronises the recorded events; total_ms / launches / work summed over the launches of `cls`. */
int r4d_profile_read(int32_t cls, double* total_ms, int64_t* launches, double* work);

/* Dispatcher-branch coverage: every host-side decision that selects a kernel variant (tile shape, template instantiation,
 * split-K form, fallback) counts its launches under a name.  Tests enumerate the table and assert that each branch ran
 * (names starting with "tuning:" are reachable through environment switches only). */
int r4d_dispatch_num_branches(void);
const char* r4d_dispatch_branch_name(int32_t i);
int64_t r4d_dispatch_branch_hits(int32_t i);      /* launches through branch i since load / the last reset */
int r4d_dispatch_reset(void);
/* Which kernel a Conv1D GEMM WOULD take (additive, ABI 6; read-only: launches nothing, needs no device, reads the current
 * r4d_set_gemm_split3 mode and nothing else).  The precedence is csrc/conv1d_route.h (DESIGN.md "Conv1D routing").
 *   kind   0 encoder call, 1 cached decode step, 2 training forward: y[M, N] = epilogue(x[M, K] . W[K, N] + b);
 *          3 data gradient of a Conv1D, 4 of the LM head (K = d, N = ldV): dx[M, K] = dy[M, N] . W^T;
 *          5 weight gradient dW[K, N] = x[M, K]^T . dy[M, N] (dense rows)
 *   have   what the caller carries of the weight: bit 0 the [N, K] copy wT, 1 the planes w3, 2 the planes w3t, 3 the planes h2,
 *          4 (kind 1) the decode step's split-K scratch, i.e. batch <= 32
 *   bf16   the kind's precision switch: r4d_set_encode_bf16 (kind 0), r4d_set_train_bf16 (kinds 2, 3, 5); ignored otherwise.
 *          2 (kinds 2, 4, 5): the LM head under r4d_set_train_head_bf16 -- its logits (N = a vocabulary chunk), its dh (kind 4 then
 *          takes plane 0 of w3t), its dwte (K = the chunk, N = d)
 * Returns a route id, or -1 for an unknown kind or M, K or N <= 0; r4d_conv1d_route_name gives its name ("unknown" outside the table). */
int32_t r4d_conv1d_route(int32_t kind, int32_t M, int32_t K, int32_t N, int32_t epilogue, uint32_t have, int32_t bf16);
const char* r4d_conv1d_route_name(int32_t route);

#ifdef __cplusplus
}
#endif
#endif /* R4D_H */
