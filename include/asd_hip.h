/*
 * asd_hip.h -- C ABI of libasd_hip.so: the MI355X (gfx950) draft-verify / accept /
 * optimal-stopping hot path behind the reference's Python API.
 *
 * The reference (sa2shun/adaptive-speculative-decoding) is 100 % Python and has no FFI of its
 * own, so every entry point below cites the reference *Python* symbol whose
 * arithmetic it replaces.  The reference-side binding a maintainer would add is a ctypes stub;
 * it is shown in INTEGRATION.md and shipped as asd_amd/_binding.py.
 *
 * Conventions
 *   - every function returns an asd_status (0 = ok, negative = error); nothing throws, nothing
 *     allocates device memory, nothing synchronises the device or the stream;
 *   - every pointer except the ones marked "host" is a DEVICE pointer on the current HIP
 *     device; `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *   - there is no CPU mode: the library only launches gfx950 kernels.  The CPU restatement
 *     lives in oracle/ and is test infrastructure only.
 *   - rows: a "row" is one verified position r = b*K + k of sequence b, draft position k.
 */
#ifndef ASD_HIP_H
#define ASD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASD_VERSION_MAJOR 0
#define ASD_VERSION_MINOR 3
#define ASD_VERSION_PATCH 0

typedef enum asd_status {
    ASD_OK = 0,
    ASD_ERR_INVALID_ARG = -1, /* NULL pointer, negative size, length mismatch (reference: ValueError, dp_solver.py:34-35) */
    ASD_ERR_UNSUPPORTED = -2, /* K > 64, L > 16, unknown dtype, ... */
    ASD_ERR_WORKSPACE = -3,   /* workspace too small or misaligned */
    ASD_ERR_HIP = -4,         /* a HIP runtime call failed (launch error, no device) */
    ASD_ERR_ALIGNMENT = -5    /* an operand pointer violates its element alignment */
} asd_status;

typedef enum asd_dtype {
    ASD_DTYPE_F32 = 0,
    ASD_DTYPE_BF16 = 1,
    ASD_DTYPE_F16 = 2
} asd_dtype;

/* limits enforced by the launchers */
#define ASD_MAX_DRAFT_LEN 64   /* K: one ballot word per sequence */
#define ASD_MAX_STOP_IDS 8     /* stop (EOS) token ids of asd_commit_step_stop */
#define ASD_MAX_STOP_SEQS 16   /* stop sequences one row may own in asd_commit_step_finish */
#define ASD_MAX_STOP_SEQ_LEN 8 /* tokens per stop sequence of asd_commit_step_finish */
#define ASD_MAX_TOP_LOGPROBS 8 /* N of asd_top_logprobs: the most likely tokens listed per row */
#define ASD_MAX_LOGIT_EDITS 1024 /* entries one row may own in asd_logit_edit_rows */
#define ASD_MAX_BAD_WORDS 256  /* words one row may own in asd_bad_words_rows */
#define ASD_MAX_BAD_WORD_LEN 8 /* tokens per word of asd_bad_words_rows */
#define ASD_MAX_NGRAM 8        /* largest n of asd_no_repeat_ngram_rows */
#ifndef ASD_NGRAM_SLICE        /* (tools/bench_no_repeat_ngram.py builds the kernel once more with one slice for any history) */
#define ASD_NGRAM_SLICE 2048   /* n-gram starts one workgroup of asd_no_repeat_ngram_rows scans */
#endif
#define ASD_MAX_STAGES 16      /* L: tiers in the DP rule */
#define ASD_MAX_SPLITS 64      /* vocab splits per row inside one launch */
#define ASD_MAX_MLP_DIM 1024   /* predictor input / hidden width */
#define ASD_NUM_LP_STATS 5     /* mean, std, min, q25, median */

/* version = major*10000 + minor*100 + patch */
int asd_version(void);
/* host: static string for a status code */
const char* asd_status_string(int status);
/* host: number of compute units of HIP device `device` (cached); <0 = asd_status */
int asd_device_cu_count(int device);

/* ------------------------------------------------------------------------------------------
 * A5 / A6  token-level verify + accept.
 *
 * Replaces the per-token loop `probs = F.softmax(score[0]); logprob = torch.log(probs[token_id])`
 * of src/training/generate_training_data.py:128-136 (one token at a time, 3 launches + a D2H
 * sync each) with ONE streaming pass over [B,K,V], and adds the speculative-sampling test the
 * north star names (no reference symbol exists for it):
 *
 *   lse[b,k]    = log sum_v exp(logits[b,k,v])                (logits / T with asd_verify_accept_ex)
 *   lp_t[b,k]   = logits[b,k,tok[b,k]] - lse[b,k]          (tok outside [0,V) => -inf)
 *   accept[b,k] = log(u[b,k]) <= lp_t[b,k] - lp_d[b,k]     (== u <= min(1, p_t/p_d))
 *   bits[b]     = sum_k accept[b,k] << k
 *   n_acc[b]    = number of leading 1 bits of bits[b] (length of the accepted prefix)
 *
 * logits: [B*K rows][V] of `dtype`, consecutive rows `ld_row` ELEMENTS apart (ld_row >= V).
 * workspace: >= asd_verify_accept_workspace_bytes(B,K,V,dtype) bytes, 256-byte aligned, and
 * zero-initialised ONCE with asd_workspace_init before its first use; the kernel leaves it
 * ready for the next call (tickets are reset by the last arriver), so one workspace serves any
 * number of stream-ordered calls.  Two calls that may run CONCURRENTLY need two workspaces.
 * ---------------------------------------------------------------------------------------- */
size_t asd_verify_accept_workspace_bytes(int B, int K, int V, int dtype);
int asd_workspace_init(void* workspace, size_t workspace_bytes, void* stream);

/* Sticky status of a workspace (verify, residual-sample and draft-sample workspaces alike): its FIRST 32-bit word.  The
 * kernels hand results across workgroups through self-tagging words of the workspace and wait for them with a bounded poll;
 * a word that never arrives poisons what depended on it (lp_target = NaN and reject; score = NaN, k* = L - 1, stop = 0;
 * tok = -1, lp = NaN) -- never a silently wrong value -- and or-s ASD_WS_LOST_HANDOFF into this word.  The word is cleared
 * only by asd_workspace_init.  A workspace whose status is non-zero MUST be re-initialised before its next use: the late
 * word was never handed back empty, so the workspace is no longer all-zero between calls.  (The reference's error
 * convention on this path: log, count, re-raise -- src/serving/pipeline.py:133-136; SURVEY.md section 8b: "return 0 on
 * success, negative asd_status on error; never throw".  A launch cannot return what its kernel finds out later: the status
 * word is that return channel.)
 * asd_workspace_status copies the word to *status_host and WAITS for `stream` (the one synchronising call of this library);
 * a caller that synchronises anyway may instead read the word from the buffer itself. */
#define ASD_WS_LOST_HANDOFF 0x1u
int asd_workspace_status(const void* workspace, uint32_t* status_host /*host, out*/, void* stream);

int asd_verify_accept(const void* logits, int dtype, int64_t ld_row,
                      const int32_t* tok /*[B,K]*/, const float* lp_draft /*[B,K]*/,
                      const float* u /*[B,K]*/, int B, int K, int V,
                      float* lp_target /*[B,K] out*/, uint8_t* accept /*[B,K] out*/,
                      int32_t* n_acc /*[B] out*/, uint64_t* accept_bits /*[B] out, may be NULL*/,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Options of asd_verify_accept_ex (host struct; NULL = all defaults). */
typedef struct asd_verify_options {
    float inv_temperature; /* > 0.  Logits are multiplied by it INSIDE the streaming pass (it only changes the
                              per-element FMA constant), i.e. the test is run on softmax(logits / T) without a
                              separate scaling pass over [B,K,V].  1.0f = logits as given.  The reference samples
                              at temperature 0.7 (generate_training_data.py:110-119, pipeline.py:94). */
    int splits;            /* launch geometry for tuning sweeps: workgroups per row in [1,ASD_MAX_SPLITS]; 0 = heuristic */
    int threads;           /* 256 | 512 | 1024 lanes per workgroup; 0 = heuristic */
    int unroll;            /* tile size in KiB a wave claims at a time: 2 | 3 | 4 | 8; 0 = heuristic */
    int nontemporal;       /* 0 | 1; -1 = heuristic */
} asd_verify_options;

int asd_verify_accept_ex(const void* logits, int dtype, int64_t ld_row,
                         const int32_t* tok, const float* lp_draft, const float* u,
                         int B, int K, int V,
                         float* lp_target, uint8_t* accept, int32_t* n_acc, uint64_t* accept_bits,
                         void* workspace, size_t workspace_bytes,
                         const asd_verify_options* opt /*host, may be NULL*/, void* stream);

/* N1, the A14 half: the verify pass that also emits, per verified position, what the missing
 * FeatureExtractor of docs/guides/RESEARCH_PROTOCOL.md:378-400 derives from per-token log-prob lists on the host:
 *   row_max_lp[b,k]  = max_v log softmax(logits[b,k]/T)[v]   (the doc's np.max(lp); free: it is -ln s of the running pair)
 *   row_entropy[b,k] = -sum_v p_v ln p_v  of that softmax      (the doc's -sum exp(lp) * lp taken over the WHOLE vocabulary
 *                      instead of the top-k list vLLM returns; one more FMA per element in the streaming loop)
 * Either may be NULL (both NULL == asd_verify_accept_ex with inv_temperature).  With row_entropy the launch is one
 * workgroup per row whatever the batch and K <= 32 (ASD_ERR_UNSUPPORTED otherwise).  A row without any finite logit
 * reports NaN for both. */
int asd_verify_accept_stats(const void* logits, int dtype, int64_t ld_row,
                            const int32_t* tok, const float* lp_draft, const float* u, int B, int K, int V,
                            float* lp_target, uint8_t* accept, int32_t* n_acc, uint64_t* accept_bits,
                            float* row_max_lp /*[B,K] out, may be NULL*/, float* row_entropy /*[B,K] out, may be NULL*/,
                            void* workspace, size_t workspace_bytes, float inv_temperature, void* stream);

/* Vocab-sharded target (lm_head split over ranks): each rank reduces its [B,K,V_shard] slice,
 * whose first column is global vocab id `v_offset`, to msg[b,k,:] = (m2, s, g) with
 *   sum_v exp(x_v) = s * 2^m2   (log2 domain: m2 = log2(e) * max_v x up to rounding, which cancels),
 *   g = x[tok - v_offset] if the token lies in this shard, else -inf.
 * One all-gather of msg ([B,K,3] f32 per rank) is the only exchange step. */
int asd_lse_partial(const void* logits_shard, int dtype, int64_t ld_row,
                    const int32_t* tok /*[B,K] GLOBAL ids*/, int B, int K, int V_shard,
                    int64_t v_offset, float inv_temperature, float* msg /*[B,K,3] out*/,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Combine the all-gathered partials (fixed shard order => identical on every rank) and run the
 * acceptance test.  msg_all: [n_shards][B][K][3]. */
int asd_accept_from_partials(const float* msg_all, int n_shards,
                             const float* lp_draft, const float* u, int B, int K, float inv_temperature,
                             float* lp_target, uint8_t* accept, int32_t* n_acc,
                             uint64_t* accept_bits, void* stream);

/* ------------------------------------------------------------------------------------------
 * N2  lm_head projection fused with the verify pass.  The reference materialises
 * logits = lm_head(hidden) and then gathers log-probs from them
 * (src/training/generate_training_data.py:128-136 via model.generate(output_scores=True));
 * here  logits[b,k,v] = sum_d hidden[b,k,d] * weight[v,d]  live only in MFMA accumulators (f32)
 * and are reduced on chip to the same (m2, s, g) partials as asd_lse_partial, one per 128-column
 * vocabulary block, then combined and tested exactly like asd_accept_from_partials.
 * hidden [B*K][ld_h], weight [V][ld_w] (the nn.Linear / HF lm_head layout), both bf16 or both f16 (dtype =
 * ASD_DTYPE_BF16 | ASD_DTYPE_F16 -- the reference loads its models in fp16, generate_training_data.py:79-85; f32:
 * ASD_ERR_UNSUPPORTED), D % 64 == 0, ld % 8 == 0, 16-byte aligned bases.
 * The log-sum-exp is over UNROUNDED f32 logits, i.e. closer to the exact product than the
 * bf16-materialised path: results agree with asd_verify_accept on bf16(hidden @ weight.T) to the
 * bf16 rounding of the logits, not bit for bit (tests/test_gpu_lm_head.py states the tolerance).
 * Workspace: asd_lm_head_verify_workspace_bytes(B, K, V), no initialisation needed. */
size_t asd_lm_head_verify_workspace_bytes(int B, int K, int V);
int asd_lm_head_verify(const void* hidden, int64_t ld_h, const void* weight, int64_t ld_w, int dtype, int D,
                       const int32_t* tok, const float* lp_draft, const float* u, int B, int K, int V,
                       float inv_temperature, float* lp_target, uint8_t* accept, int32_t* n_acc,
                       uint64_t* accept_bits, void* workspace, size_t workspace_bytes, void* stream);
/* The same call with the row arg-max: argmax_out[b,k] = argmin-id argmax_v logits[b,k,v] (ties -> lowest id,
 * NaN logits never win, -1 if the row has no logit > -inf; may be NULL).  greedy != 0 replaces the sampling
 * test by greedy verification, accept[b,k] = (tok[b,k] == argmax_out[b,k]); lp_draft and u are then unused
 * (may be NULL) and lp_target is still the draft token's log-prob under the target.  With the arg-max a
 * hidden-state tier needs no logits row for greedy decoding: the correction token after the accepted
 * prefix is argmax_out[b, n_acc[b]], the bonus token the arg-max of an extra row. */
int asd_lm_head_verify_ex(const void* hidden, int64_t ld_h, const void* weight, int64_t ld_w, int dtype, int D,
                          const int32_t* tok, const float* lp_draft, const float* u, int B, int K, int V,
                          float inv_temperature, int greedy, float* lp_target, uint8_t* accept, int32_t* n_acc,
                          uint64_t* accept_bits, int32_t* argmax_out /*[B,K] out, may be NULL*/,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Optional one-time re-layout of an lm_head matrix for the three calls above and below (like asd_mlp_pack_weights for
 * the predictor): [V][ld_w] bf16 -> tile-major [ceil(V/256)][D/64][256 rows][64 columns], rows past V zero.  A column
 * block's 64-deep reduction step is then ONE contiguous 32 KiB run instead of 256 lines that sit D*2 bytes apart (each
 * in another DRAM page).  Pass the packed image as `weight` with ld_w = 0; results are bit-identical to the unpacked call.
 * For a vocabulary shard (asd_lm_head_partial) pack the shard's rows.  packed: asd_lm_head_packed_bytes(V, D) bytes. */
size_t asd_lm_head_packed_bytes(int V, int D);
int asd_lm_head_pack_weights(const void* weight, int64_t ld_w, int dtype, int V, int D, void* packed /*out*/,
                             size_t packed_bytes, void* stream);

/* Tensor-parallel lm_head (weight split over ranks along the vocabulary): this rank's [V_shard, D] slice,
 * whose row 0 is global vocabulary id v_offset, reduced straight to the asd_lse_partial message
 * msg[b,k,:] = (m2, s, g); all-gather the messages and finish with asd_accept_from_partials.  The
 * logits of the shard are never formed; [B,K,3] floats per rank is the only exchange. */
int asd_lm_head_partial(const void* hidden, int64_t ld_h, const void* weight_shard, int64_t ld_w, int dtype, int D,
                        const int32_t* tok /*[B,K] GLOBAL ids*/, int B, int K, int V_shard, int64_t v_offset,
                        float inv_temperature, float* msg /*[B,K,3] out*/, void* workspace, size_t workspace_bytes,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * X3 (callers' side of the path)  y[M][N] = x[M][D] . w[N][D]^T (+ bias[N]): the nn.Linear projections of the
 * decoder layers the reference runs through transformers / vLLM (third party there: src/serving/real_model_pipeline.py:135,
 * src/models/stage.py) -- the step that produces the hidden states asd_lm_head_verify consumes and, for the draft tier, the
 * logits asd_draft_sample consumes.  The lm_head kernels' main loops with a STORE epilogue; narrow matrices are cut into
 * reduction slices whose f32 partials meet in `workspace` and are added in slice order (bit-reproducible).
 * x, w, bias (may be NULL), y: all bf16 or all f16 (dtype); f32 accumulation, ONE rounding at the store.
 * D % 64 == 0, N % 4 == 0, x / w 16-byte aligned with ld % 8 == 0, y 8-byte aligned with ld_y % 4 == 0.
 * ld_w == 0: w is the tile-major image asd_lm_head_pack_weights(w, ld, dtype, N, D, ...) writes (asd_lm_head_packed_bytes(N, D)
 * bytes: N * D * 2 when N % 256 == 0, so a matrix can be re-laid in its own storage); same results, bit for bit.
 * workspace: asd_linear_workspace_bytes(M, N, D) bytes (no initialisation needed; may be shared by calls on one stream). */
size_t asd_linear_workspace_bytes(int M, int N, int D);
int asd_linear(const void* x, int64_t ld_x, const void* w, int64_t ld_w, const void* bias, int dtype, int M, int N, int D,
               void* y /*[M][ld_y] out*/, int64_t ld_y, void* workspace, size_t workspace_bytes, void* stream);
/* ... + residual[M][ld_res] (may be NULL; may alias y: y = y + x . w^T, the decoder layer's residual connection) */
int asd_linear_ex(const void* x, int64_t ld_x, const void* w, int64_t ld_w, const void* bias, const void* residual,
                  int64_t ld_res, int dtype, int M, int N, int D, void* y /*[M][ld_y] out*/, int64_t ld_y, void* workspace,
                  size_t workspace_bytes, void* stream);
/* Building block of asd_decoder_forward: as asd_linear_ex, but a plan with reduction slices stops after the product --
 * *k_slices > 1 on return means y was NOT written: the f32 partials lie in `workspace` as [k_slices][M][N] and the caller's
 * next kernel adds them in slice order, then the bias, then the residual (the order asd_linear_ex uses: same bits).
 * *k_slices == 1: y is complete. */
int asd_linear_partial(const void* x, int64_t ld_x, const void* w, int64_t ld_w, const void* bias, const void* residual,
                       int64_t ld_res, int dtype, int M, int N, int D, void* y, int64_t ld_y, void* workspace,
                       size_t workspace_bytes, void* stream, int* k_slices /*out*/);
/* host: the number of reduction slices the launcher uses for this product (1 = unsliced; 0 = unsupported shape) */
int asd_linear_slices(int M, int N, int D);

/* ------------------------------------------------------------------------------------------
 * X3, continued: the rest of a decoder layer around the projections, for the M = B * T positions a tier is fed in one pass
 * (row m = b * T + t), over a per-sequence KV cache.  bf16 only; head_dim 128 (every Qwen2.5 shape).
 *   asd_rmsnorm        out = x * rsqrt(mean(x^2) + eps) * weight, f32 arithmetic, one rounding; D % 4 == 0, D <= 8192
 *   asd_rope_kv_store  qkv [M][ld] = q heads | k heads | v heads: rotary embedding (half-split pairs (i, i + 64), angle
 *                      pos[m] * inv_freq[i]) of q IN PLACE and of k INTO the cache; v into the TRANSPOSED cache
 *                        k_cache  [cache rows][KVH][t_max][128]      vt_cache [cache rows][KVH][128][t_max]
 *                      cache row of sequence b: rows[b] (rows == NULL: b); pos is clamped to [0, t_max - 1]; t_max % 32 == 0
 *   asd_attn_ragged    out[m][head] = softmax_j<=pos[m] (q . k_j / sqrt(128)) v_j over the cache of sequence m / T (grouped
 *                      queries: head / (H / KVH) picks the kv head); MFMA flash-decode, both cache operands read in operand
 *                      layout straight from global memory (that is what the transposed V cache is for)
 *   asd_silu_mul       act[m][i] = silu(gate_up[m][i]) * gate_up[m][I + i]
 *   asd_decoder_forward  n_layers x (rmsnorm, qkv, rope + cache write, attention, o + residual, rmsnorm, gate | up, silu * up,
 *                      down + residual) on x [M][ld_x] in place -- nine launches per layer, all issued by this one call.
 * Entries of the caches past a sequence's committed length are rewritten before they are read (KV rollback = a length
 * update, asd_commit_step).  CONTRACT of the caches (X3 is plumbing around the path, third party in the reference):
 *   - they must hold FINITE values from the start (zero-fill them once): asd_attn_ragged masks keys beyond pos by giving them
 *     probability 0, but still feeds the whole 32-key tile through the MFMA, and 0 * NaN = NaN;
 *   - positions are clamped into [0, t_max - 1] by BOTH kernels; slot t_max - 1 is therefore a TRASH slot (the padding
 *     behind a ragged feed lands there, several rows may write it): size t_max at least one slot beyond the longest real
 *     sequence (serving/hierarchy.py does) and never pass a negative position for a row whose result is used. */
typedef struct asd_layer {
    const void* ln1_w;      /* [hidden] */
    const void* qkv_w;      /* [hidden + 2 * KVH * 128][hidden]: q | k | v projection rows */
    const void* qkv_b;      /* [hidden + 2 * KVH * 128] or NULL */
    const void* o_w;        /* [hidden][hidden] */
    const void* ln2_w;      /* [hidden] */
    const void* gate_up_w;  /* [2 * intermediate][hidden]: gate rows, then up rows */
    const void* down_w;     /* [hidden][intermediate] */
    void* k_cache;
    void* vt_cache;
    int weights_packed;     /* != 0: the four matrices are tile-major images (asd_lm_head_pack_weights of each, see asd_linear) */
} asd_layer_t;
typedef struct asd_decoder_shape {
    int hidden, heads, kv_heads, head_dim, intermediate;
    float rms_eps;
    const float* inv_freq;  /* [64] f32, device: theta^(-2 i / 128) */
    int t_max;              /* positions per cache row */
} asd_decoder_shape_t;
int asd_rmsnorm(const void* x, int64_t ld_x, const void* weight, float eps, int dtype, int M, int D, void* out /*[M][ld_out]*/,
                int64_t ld_out, void* stream);
int asd_rope_kv_store(void* qkv /*[B*T][ld_qkv] in/out*/, int64_t ld_qkv, const int32_t* pos /*[B*T]*/,
                      const int32_t* rows /*[B] or NULL*/, const float* inv_freq /*[64]*/, int dtype, int B, int T, int H, int KVH,
                      int head_dim, void* k_cache, void* vt_cache, int t_max, void* stream);
int asd_attn_ragged(const void* qkv, int64_t ld_qkv, const void* k_cache, const void* vt_cache, const int32_t* pos,
                    const int32_t* rows, int dtype, int B, int T, int H, int KVH, int head_dim, int t_max,
                    void* out /*[B*T][ld_out], H * 128 wide*/, int64_t ld_out, void* stream);
int asd_silu_mul(const void* gate_up /*[M][ld_gu], 2 I wide*/, int64_t ld_gu, int dtype, int M, int I, void* act /*[M][ld_act]*/,
                 int64_t ld_act, void* stream);
size_t asd_decoder_scratch_bytes(const asd_decoder_shape_t* shape, int M);
/* final_norm_w / normed_out (both or neither): the model's last RMSNorm, applied to the final x into normed_out [B*T][ld_normed]
 * (fused with the last layer's residual connection).  Where a projection is cut into reduction slices, the kernel that follows
 * it adds the slices' partials itself (asd_linear_partial), so a layer is nine launches whatever the plans are. */
int asd_decoder_forward(const asd_layer_t* layers, int n_layers, const asd_decoder_shape_t* shape, void* x /*[B*T][ld_x] in/out*/,
                        int64_t ld_x, const int32_t* pos, const int32_t* rows, int B, int T, const void* final_norm_w,
                        void* normed_out, int64_t ld_normed, void* scratch /*256-byte aligned*/, size_t scratch_bytes,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * N3  commit / KV rollback bookkeeping of one token-level step, on the device.
 * The reference's src/serving/cache_manager.py:149-190 `truncate_at_stage` trims a dict of strings;
 * with a per-sequence KV cache the rollback after a rejection is a length update.  Row b of the token
 * buffer `out_tokens` ([B][ld_out] i32) receives tok[b, 0..n_acc[b]) followed by drawn[b] (the residual /
 * bonus token of asd_residual_sample) at index seq_len[b]; seq_len[b] += n_acc[b] + 1, clamped to
 * max_len (tokens past max_len are dropped); n_commit[b] (may be NULL) = tokens appended.  n_acc is
 * clamped to [0, K].  No host synchronisation is needed to learn n_acc. */
int asd_commit_step(const int32_t* tok /*[B,K]*/, const int32_t* n_acc /*[B]*/, const int32_t* drawn /*[B]*/,
                    int B, int K, int32_t* seq_len /*[B] in/out*/, int32_t* out_tokens /*[B][ld_out]*/,
                    int64_t ld_out, int32_t* n_commit /*[B] out, may be NULL*/, int32_t max_len, void* stream);
/* asd_commit_step with a second scatter: the per-token log-probs a stage returns (stage.generate(..., return_logprobs=True),
 * src/serving/pipeline.py:204-231) follow the tokens into out_lp ([B][ld_out] f32, the geometry of out_tokens):
 * out_lp[b, len + k] = lp_tok[b, k] for k < n_acc[b] (the verify's lp_target), out_lp[b, len + n_acc[b]] = lp_drawn[b]
 * (asd_residual_sample_lp), under the same clamp to max_len; the bits are copied.  K = 0 (tok and lp_tok may be NULL): every
 * sequence appends drawn / lp_drawn -- plain sampled decoding.  Status codes: those of asd_commit_step. */
int asd_commit_step_lp(const int32_t* tok /*[B,K]*/, const float* lp_tok /*[B,K]*/, const int32_t* n_acc /*[B]*/,
                       const int32_t* drawn /*[B]*/, const float* lp_drawn /*[B]*/, int B, int K,
                       int32_t* seq_len /*[B] in/out*/, int32_t* out_tokens /*[B][ld_out]*/, float* out_lp /*[B][ld_out]*/,
                       int64_t ld_out, int32_t* n_commit /*[B] out, may be NULL*/, int32_t max_len, void* stream);
/* asd_commit_step_lp that ends a sequence at a stop (EOS) token: what HF `generate`'s EOS handling does behind the reference's
 * stage.generate (src/serving/pipeline.py:204-209), decided on the device so that a step still reads nothing back.
 * Row b, na = clamp(n_acc[b], 0, K), len = seq_len[b], candidates c_0..c_na = tok[b, 0..na) ++ drawn[b]:
 *   finished[b] != 0 on entry: the row is left alone (seq_len, finished, *n_finished unchanged), n_commit[b] = 0.
 *   otherwise fit = min(na + 1, max(max_len - len, 0)); j* = the smallest j < fit with c_j in stop_ids[0..n_stop);
 *   appended = j* + 1 if j* exists, else fit.  The first `appended` candidates and their log-probs go to index len.. as in
 *   asd_commit_step_lp (bits copied), seq_len[b] = len + appended, n_commit[b] = appended.  The stop token itself is committed;
 *   a rejected draft token (index >= na) and a stop token cut off by max_len never stop a row.
 *   finished[b] = 1 (stop) if j* exists -- also when it lands on the last free slot --, else 2 (length) if
 *   len + appended >= max_len (a row that enters full included), else it stays 0.  A row going 0 -> non-zero adds 1 to
 *   *n_finished (may be NULL) with a global atomic: the host reads that one counter to leave its loop.
 * n_stop == 0 (stop_ids may be NULL) with all flags zero: tokens, log-probs, seq_len and n_commit are asd_commit_step_lp's.
 * Status codes: those of asd_commit_step_lp; finished == NULL, n_stop < 0, n_stop > 0 with stop_ids == NULL: invalid argument;
 * n_stop > ASD_MAX_STOP_IDS: unsupported. */
int asd_commit_step_stop(const int32_t* tok /*[B,K]*/, const float* lp_tok /*[B,K]*/, const int32_t* n_acc /*[B]*/,
                         const int32_t* drawn /*[B]*/, const float* lp_drawn /*[B]*/, int B, int K,
                         const int32_t* stop_ids /*[n_stop]*/, int n_stop, int32_t* seq_len /*[B] in/out*/,
                         int32_t* out_tokens /*[B][ld_out]*/, float* out_lp /*[B][ld_out]*/, int64_t ld_out,
                         int32_t* n_commit /*[B] out, may be NULL*/, int32_t* finished /*[B] in/out: 0, 1 stop, 2 length*/,
                         int32_t* n_finished /*[1] in/out, may be NULL*/, int32_t max_len, void* stream);
/* asd_commit_step_stop with multi-token stop sequences, a list of sequences per row and a length limit per row: how a serving
 * request ends (stop strings, the reference's per-request GenerationRequest.max_tokens, src/serving/server.py:43), decided on the
 * device inside the step's commit.  A step commits up to K + 1 tokens, so a sequence may end in the middle of the accepted
 * prefix, on the drawn token, or begin in tokens an earlier step committed.
 * seq_tok [n_seq][ASD_MAX_STOP_SEQ_LEN] holds the sequences, seq_n [n_seq] their lengths; slots behind a sequence's length are
 * ignored, a sequence whose length lies outside [1, ASD_MAX_STOP_SEQ_LEN] never matches.  Row b owns sequences
 * row_first[b] .. row_first[b+1] - 1 (row_first [B+1], non-decreasing, inside [0, n_seq]); row_first == NULL: every row owns all
 * n_seq.  A row owns at most ASD_MAX_STOP_SEQS sequences: the kernel IGNORES the ones behind the first ASD_MAX_STOP_SEQS of a
 * row's list (and any part of a list that lies outside [0, n_seq)); the caller checks its lists.
 * Row b, na = clamp(n_acc[b], 0, K), len = seq_len[b], candidates c_0..c_na = tok[b, 0..na) ++ drawn[b]:
 *   finished[b] != 0 on entry: the row is left alone (seq_len, finished, *n_finished, matched[b] unchanged), n_commit[b] = 0.
 *   otherwise limit = max_len when row_max_len == NULL, else min(max_len, max(row_max_len[b], 0)) (a position, prompt included,
 *   like max_len); fit = min(na + 1, max(limit - len, 0)).  The row's stream is out_tokens[b, 0..len) followed by
 *   c_0..c_{fit-1}.  Sequence s of length m ENDS AT candidate j < fit when stream positions len + j - m + 1 .. len + j equal
 *   s[0..m) and len + j - m + 1 >= start (`start`: the first generated position, the prompt length -- no token of a match lies
 *   in the prompt; positions in front of `start` are never read).  j* = the smallest j at which any owned sequence ends;
 *   appended = j* + 1 if j* exists, else fit.  The first `appended` candidates and their log-probs go to index len.. as in
 *   asd_commit_step_lp (bits copied), seq_len[b] = len + appended, n_commit[b] = appended: the matched tokens are committed.
 *   A rejected draft token (index >= na, other than drawn) and anything cut off by `limit` never take part in a match.
 *   finished[b] = 1 (stop) if j* exists -- also when it lands on the last free slot --, else 2 (length) if
 *   len + appended >= limit, else it stays 0.  A row going 0 -> non-zero adds 1 to *n_finished (may be NULL) with a global atomic.
 *   matched[b] (may be NULL) = the index, within the row's own list, of the first owned sequence that ends at j*; written only
 *   when j* exists.
 * row_first == NULL, row_max_len == NULL and every sequence of length 1: every output is asd_commit_step_stop's with those ids,
 * byte for byte, for any start <= every seq_len.
 * Status codes: those of asd_commit_step_stop (negative B / K / max_len / n_seq: invalid argument; B == 0: ASD_OK;
 * K > ASD_MAX_DRAFT_LEN: unsupported; NULL operands, finished == NULL, ld_out < max_len: invalid argument); start < 0, n_seq > 0
 * with seq_tok == NULL or seq_n == NULL: invalid argument; row_first == NULL with n_seq > ASD_MAX_STOP_SEQS: unsupported. */
int asd_commit_step_finish(const int32_t* tok /*[B,K]*/, const float* lp_tok /*[B,K]*/, const int32_t* n_acc /*[B]*/,
                           const int32_t* drawn /*[B]*/, const float* lp_drawn /*[B]*/, int B, int K,
                           const int32_t* seq_tok /*[n_seq][ASD_MAX_STOP_SEQ_LEN]*/, const int32_t* seq_n /*[n_seq]*/, int n_seq,
                           const int32_t* row_first /*[B+1] or NULL*/, const int32_t* row_max_len /*[B] or NULL*/,
                           int32_t start /*first generated position*/, int32_t* seq_len /*[B] in/out*/,
                           int32_t* out_tokens /*[B][ld_out]*/, float* out_lp /*[B][ld_out]*/, int64_t ld_out,
                           int32_t* n_commit /*[B] out, may be NULL*/, int32_t* finished /*[B] in/out: 0, 1 stop, 2 length*/,
                           int32_t* n_finished /*[1] in/out, may be NULL*/, int32_t* matched /*[B] in/out, may be NULL*/,
                           int32_t max_len, void* stream);

/* ------------------------------------------------------------------------------------------
 * Greedy decoding (temperature 0): arg-max verify and commit token in one launch, no random numbers.
 * The reference accepts temperature 0 (src/serving/server.py:44,67; src/core/types.py:240,267).
 * logits: sequence b owns K + 1 rows, row (b, k) starts at element b*ld_seq + k*ld_row: rows 0..K-1 score the draft tokens
 * tok[b, k], row K is the bonus row (the row convention of asd_lm_head_verify_ex; a target's [B, K+1, V] output is read in
 * place).  K == 0: one row per sequence, the plain greedy step.  Any V >= 1 and any element-aligned row base (16-byte loads
 * where the address allows, scalar head and tail); ld_row >= V, ld_seq >= (K+1)*ld_row; the padding is never read.
 * Per row: argmax = the lowest id among the maxima; a NaN logit never wins; -1 if the row has no logit above -inf.
 *   lp_argmax = x[argmax]*inv_temperature - lse(x*inv_temperature), NaN where argmax == -1.
 * Per sequence: accept[b,k] = (argmax[b,k] >= 0 && tok[b,k] == argmax[b,k]); n_acc[b] = length of the accepted prefix;
 *   drawn[b] = argmax[b, n_acc[b]], lp_drawn[b] = that row's lp_argmax; lp_target[b,k] = x[tok]*inv_temperature - lse (what
 *   asd_verify_accept reports), -inf for tok outside [0,V); on an accepted position it has the bits of lp_argmax[b,k].
 * splits: workgroups per row in [1, ASD_MAX_SPLITS], 0 = heuristic (asd_device_cu_count).  A geometry gives the same bits on
 * every run.  Nothing in the kernel waits, so there is no status word; the launcher zeroes the tickets (hipMemsetAsync) ahead
 * of every launch: the workspace needs no asd_workspace_init, calls in stream order may share one, calls in flight together
 * need one each.
 * Status: NULL n_acc / drawn / lp_drawn, inv_temperature not > 0 (both before the empty-batch return), negative sizes, V == 0,
 * NULL logits / workspace, tok == NULL with K > 0, ld_row < V, ld_seq < (K+1)*ld_row: invalid argument; K > ASD_MAX_DRAFT_LEN,
 * unknown dtype, splits outside [0, ASD_MAX_SPLITS], a row of 2 GiB or more: unsupported; workspace misaligned (256) or too
 * small: workspace; B == 0: ASD_OK, nothing launched.
 * ---------------------------------------------------------------------------------------- */
size_t asd_verify_greedy_workspace_bytes(int B, int K, int V, int dtype);   /* sized for ASD_MAX_SPLITS; a multiple of 256 */
int asd_verify_greedy(const void* logits, int dtype, int64_t ld_seq, int64_t ld_row,
                      const int32_t* tok /*[B,K]; may be NULL when K == 0*/, int B, int K, int V,
                      float inv_temperature, int splits /*workgroups per row, 0 = heuristic*/,
                      int32_t* argmax_out /*[B,K+1] out, may be NULL*/, float* lp_argmax /*[B,K+1] out, may be NULL*/,
                      float* lp_target /*[B,K] out, may be NULL*/, uint8_t* accept /*[B,K] out, may be NULL*/,
                      int32_t* n_acc /*[B] out*/, int32_t* drawn /*[B] out*/, float* lp_drawn /*[B] out*/,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Top-N log-probs per row: the table behind SamplingParams(logprobs=N) of the stage specification
 * (docs/guides/RESEARCH_PROTOCOL.md:272-277), which its FeatureExtractor consumes (:366-409).
 * logits: B sequences of K1 rows, row (b, j) starts at element b*ld_seq + j*ld_row and is read in place (asd_verify_greedy's
 * addressing with K1 = K + 1; K1 == 1 is a [B, V] matrix).  Any V >= 1 and any element-aligned row base; ld_row >= V,
 * ld_seq >= K1*ld_row; the padding is never read.
 * Per row, the N entries with the largest logits, 1 <= N <= ASD_MAX_TOP_LOGPROBS, as pairs (top_id, top_lp):
 *   order: value descending, then id ascending -- a total order, so the ids do not depend on the launch geometry, and slot 0
 *   is asd_verify_greedy's argmax.  A NaN logit is never listed; a logit of -inf is never listed.
 *   top_lp = x[id]*inv_temperature - lse(x*inv_temperature) over the WHOLE vocabulary (asd_verify_greedy's lp_argmax
 *   arithmetic; slot 0 has its bits).  A row that holds a NaN has NaN log-probs; its ids are listed all the same.
 *   A slot that cannot be filled (V < N, or fewer than N logits above -inf) holds id -1 and lp -inf.
 * splits: workgroups per row in [1, ASD_MAX_SPLITS], 0 = heuristic (asd_verify_greedy's).  Nothing in the kernel waits, so
 * there is no status word; the launcher zeroes the tickets (hipMemsetAsync) ahead of every launch: the workspace needs no
 * asd_workspace_init, calls in stream order may share one, calls in flight together need one each.
 * Status, in this order: NULL top_id / top_lp, inv_temperature not > 0 (both before the empty-batch return), negative sizes:
 * invalid argument; B == 0: ASD_OK, nothing launched; V == 0, K1 < 1, N < 1: invalid argument; K1 > ASD_MAX_DRAFT_LEN + 1,
 * N > ASD_MAX_TOP_LOGPROBS, unknown dtype, splits outside [0, ASD_MAX_SPLITS]: unsupported; NULL logits / workspace,
 * ld_row < V, ld_seq < K1*ld_row: invalid argument; logits not aligned to the element size: alignment; workspace misaligned
 * (256): workspace; a row of 2 GiB or more: unsupported; workspace too small: workspace.
 * ---------------------------------------------------------------------------------------- */
size_t asd_top_logprobs_workspace_bytes(int B, int K1, int N);   /* sized for ASD_MAX_SPLITS; a multiple of 256; 256 when B <= 0 */
int asd_top_logprobs(const void* logits, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V,
                     float inv_temperature, int N, int splits /*workgroups per row, 0 = heuristic*/,
                     int32_t* top_id /*[B,K1,N] out*/, float* top_lp /*[B,K1,N] out*/,
                     void* workspace, size_t workspace_bytes, void* stream);
/* asd_top_logprobs_rows: asd_top_logprobs with one temperature per SEQUENCE (per-request sampling parameters, below):
 * inv_temperature is a DEVICE array [B]; the rows of sequence b are scaled by c2 = (float)(log2(e) * (double)inv_temperature[b]),
 * formed on the device by the one f64 product the host forms it with, so a sequence returns the bits asd_top_logprobs returns
 * for it with that scalar at the same `splits`.  The values cannot be checked by the launcher: every one must be finite and
 * > 0.  NULL inv_temperature (with B > 0): invalid argument, reported where asd_top_logprobs reports a bad scalar; every other
 * argument, status code and the workspace are asd_top_logprobs'. */
int asd_top_logprobs_rows(const void* logits, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V,
                          const float* inv_temperature /*[B], device*/, int N, int splits,
                          int32_t* top_id /*[B,K1,N] out*/, float* top_lp /*[B,K1,N] out*/,
                          void* workspace, size_t workspace_bytes, void* stream);
/* ------------------------------------------------------------------------------------------
 * Prompt log-probs (SamplingParams(prompt_logprobs=N); OpenAI's echo + logprobs): per row of [B, T, V] logits the log-prob and
 * the rank of ONE GIVEN token, and optionally the row's top-N table, in asd_top_logprobs' one streaming pass.
 * logits: element (b, t, v) at b*ld_seq + t*ld_row + v (asd_top_logprobs' addressing), read in place, never written; any
 * T >= 1 (no ASD_MAX_DRAFT_LEN limit; B*T*splits <= INT32_MAX).  target[b*ld_target + t] is the token row (b, t) scores.
 * first: DEVICE array [B], or NULL for 0 everywhere.  Row (b, t) is SCORED when t >= first[b]; with x the stored row and
 * g = target[b, t]:
 *   lp[b,t]   = x[g]*inv_temperature - lse(x*inv_temperature): the operations of a table slot, so where the table lists g the
 *               bits are equal.
 *   rank[b,t] = 1 + #{v : x[v] > x[g], or x[v] == x[g] and v < g} over the stored values -- the table's total order (value
 *               descending, then id ascending); exact, the same in every launch geometry.  A NaN element is never counted; a
 *               -inf element takes part like any other value.  For x[g] > -inf: rank <= N  <=>  top_id[b,t,rank-1] == g, and
 *               top_lp[b,t,rank-1] has lp's bits (the table itself never lists a -inf logit).
 *   top_id / top_lp [b,t,:N]: what asd_top_logprobs writes for the row at the same inv_temperature, N and split count, bit
 *               for bit.  N == 0: no table is kept or written; top_id / top_lp may be NULL.
 *   g outside [0, V) is never dereferenced: lp = NaN, rank = 0, the table is written all the same.  A NaN x[g]: lp = NaN,
 *   rank = 0.
 * A SKIPPED row (t < first[b]: left-padding) costs no pass over its logits: lp = 0, rank = 0, ids -1, table log-probs -inf.
 * splits: workgroups per row in [1, ASD_MAX_SPLITS], 0 = heuristic (asd_verify_greedy's).  The workspace is sized for the split
 * count the launch USES (with splits == 0 the heuristic's choice on the current device; a host without a device counts 256
 * CUs): asd_prompt_logprobs_workspace_bytes takes the same five values; whole rows (one slice) need 256 bytes.  Tickets are
 * zeroed by the launcher ahead of every launch, as in asd_top_logprobs.
 * Status, in this order: NULL lp / rank (NULL top_id / top_lp with N > 0), inv_temperature not > 0, negative sizes: invalid
 * argument; B == 0 or T == 0: ASD_OK, nothing launched; V == 0: invalid argument; unknown dtype: unsupported;
 * N > ASD_MAX_TOP_LOGPROBS, splits outside [0, ASD_MAX_SPLITS]: unsupported; NULL logits / target / workspace, ld_row < V,
 * ld_seq < T*ld_row, ld_target < T: invalid argument; a row of 2 GiB or more: unsupported; logits not aligned to the element
 * size: alignment; workspace misaligned (256): workspace; B*T*splits > INT32_MAX: unsupported; workspace too small: workspace.
 * ---------------------------------------------------------------------------------------- */
size_t asd_prompt_logprobs_workspace_bytes(int B, int T, int V, int dtype, int splits);   /* a multiple of 256; 256 for empty or invalid sizes */
int asd_prompt_logprobs(const void* logits, int dtype, int64_t ld_seq, int64_t ld_row, int B, int T, int V,
                        const int32_t* target /*[B, ld_target]: target[b*ld_target + t] is the token row (b, t) scores*/,
                        int64_t ld_target, const int32_t* first /*[B], or NULL: 0 for every sequence*/,
                        float inv_temperature, int N /*0..ASD_MAX_TOP_LOGPROBS*/, int splits /*0 = heuristic*/,
                        float* lp /*[B,T]*/, int32_t* rank /*[B,T]*/,
                        int32_t* top_id /*[B,T,N]; may be NULL when N == 0*/, float* top_lp /*likewise*/,
                        void* workspace, size_t workspace_bytes, void* stream);
/* ------------------------------------------------------------------------------------------
 * Token statistics: per row of a step's [B, K1, V] logits that may be COMMITTED, the rank of the committed token, the arg-max
 * and its log-prob, the entropy of the row's softmax and optionally the row's top-N table, in asd_top_logprobs' one streaming
 * pass.  All figures are of the UNTRUNCATED softmax of x * inv_temperature over the whole vocabulary.
 * logits: asd_top_logprobs' addressing, read in place, never written; 1 <= K1 <= ASD_MAX_DRAFT_LEN + 1.
 * With a = clamp(n_acc[b], 0, K1 - 1): rows j <= a are LIVE; live row j scores g = tok[b*ld_tok + j] for j < a and
 * g = drawn[b] for j == a (what the step's commit may commit; K1 == 1, n_acc == 0 is a stage without a draft: tok may be
 * NULL).  Rows j > a are never committed: no pass is made over them and their outputs are NEUTRAL: rank 0, arg-max id -1,
 * entropy 0.0, max log-prob 0.0, table slots (-1, -inf).
 * Per live row (b, j), x the stored row:
 *   stat_id[b,j,0]  = rank of g: 1 + #{v : x[v] > x[g], or x[v] == x[g] and v < g} (asd_prompt_logprobs' definition and count:
 *                     exact, the same in every launch geometry); 0 when g is outside [0, V) (never dereferenced) or x[g] is NaN.
 *   stat_id[b,j,1], stat_val[b,j,1] = the arg-max id (ties: the lowest id) and its log-prob: the bits of asd_top_logprobs'
 *                     slot 0 at the same inv_temperature and split count; a row without a finite logit: (-1, -inf).
 *   stat_val[b,j,0] = the entropy H = -sum_v p_v ln p_v in nats.  A -inf element carries no mass; s == 0 (no finite logit) or
 *                     any NaN element: NaN.  Its partial sums are merged in the fixed lane / wave / slice order of the lse's.
 *   top_id / top_lp [b,j,:N]: what asd_top_logprobs writes for the row at the same inv_temperature, N and split count, bit
 *                     for bit.  N == 0: no table is written; top_id / top_lp may be NULL.
 * inv_t_rows: DEVICE array [B] of per-sequence 1 / T as in asd_top_logprobs_rows (a sequence returns the bits the scalar call
 * returns for it), or NULL: the scalar inv_temperature holds.  With inv_t_rows the scalar is ignored.
 * stat_id / stat_val are [B, K1, 2], so asd_commit_top_logprobs with N = 2 moves row j to the step's j-th committed token.
 * splits and the workspace: asd_prompt_logprobs' (sized for the split count the launch USES; whole rows need 256 bytes).
 * Status, in this order: NULL stat_id / stat_val (NULL top_id / top_lp with N > 0), inv_temperature not > 0 (without
 * inv_t_rows), negative sizes: invalid argument; B == 0 or K1 == 0: ASD_OK, nothing launched; V == 0: invalid argument;
 * unknown dtype: unsupported; N > ASD_MAX_TOP_LOGPROBS, splits outside [0, ASD_MAX_SPLITS], K1 > ASD_MAX_DRAFT_LEN + 1:
 * unsupported; NULL logits / n_acc / drawn / workspace, NULL tok with K1 > 1, ld_row < V, ld_seq < K1*ld_row,
 * ld_tok < K1 - 1 (K1 > 1): invalid argument; a row of 2 GiB or more: unsupported; logits not aligned to the element size:
 * alignment; workspace misaligned (256): workspace; B*K1*splits > INT32_MAX: unsupported; workspace too small: workspace.
 * ---------------------------------------------------------------------------------------- */
size_t asd_token_stats_workspace_bytes(int B, int K1, int V, int dtype, int splits);   /* a multiple of 256; 256 for empty or invalid sizes */
int asd_token_stats(const void* logits, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V,
                    const int32_t* tok /*[B, ld_tok]; NULL iff K1 == 1*/, int64_t ld_tok,
                    const int32_t* n_acc /*[B]*/, const int32_t* drawn /*[B]*/,
                    float inv_temperature, const float* inv_t_rows /*[B] device, or NULL*/,
                    int N /*0..ASD_MAX_TOP_LOGPROBS*/, int splits /*0 = heuristic*/,
                    int32_t* stat_id /*[B,K1,2]: rank, arg-max id*/, float* stat_val /*[B,K1,2]: entropy, max log-prob*/,
                    int32_t* top_id /*[B,K1,N]; may be NULL when N == 0*/, float* top_lp /*likewise*/,
                    void* workspace, size_t workspace_bytes, void* stream);

/* The table of a step follows the step's commit (RESEARCH_PROTOCOL.md:272-277: one [N] row per GENERATED token).  Runs behind
 * asd_commit_step_lp / asd_commit_step_stop of the same step and reads their outputs: seq_len[b] AFTER the commit and
 * n_commit[b].  For j < min(n_commit[b], K1):  out[b, seq_len[b] - n_commit[b] + j, :] = top[b, j, :]  (ids and log-probs;
 * bits are copied; positions outside [0, max_len) are not written).  Row j of a step is the distribution its j-th committed
 * token came from: accepted draft token j comes from score row j, the token drawn behind the prefix from row n_acc (the bonus
 * row when n_acc == K).  A finished sequence (n_commit == 0) appends nothing.  out_id / out_lp: [B][max_len][N], contiguous.
 * Status: negative sizes: invalid argument; B == 0: ASD_OK; K1 > ASD_MAX_DRAFT_LEN + 1, N > ASD_MAX_TOP_LOGPROBS: unsupported;
 * K1 < 1, N < 1, any NULL pointer: invalid argument. */
int asd_commit_top_logprobs(const int32_t* top_id /*[B,K1,N]*/, const float* top_lp /*[B,K1,N]*/,
                            const int32_t* seq_len /*[B]: AFTER the step's commit*/, const int32_t* n_commit /*[B]*/,
                            int B, int K1, int N, int32_t* out_id /*[B,max_len,N]*/, float* out_lp /*[B,max_len,N]*/,
                            int max_len, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-request seeds (SamplingParams(seed=...); the reference's evaluation runs `random_seeds: [42, 123, 456, 789, 999]`):
 * every uniform a decoding step consumes, in ONE launch, from a counter-based generator keyed by the request's seed.
 * Generator: Philox4x32-10 (Random123), multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85.
 *   key     = (seed_lo, seed_hi) of seeds[b], the 64 bits read as unsigned
 *   counter = (step, k, stage, 0): the caller's step index, the draft slot k, the stage's index
 *   word 0 of counter (step, k, stage, 0): the proposal uniform of slot k   -> r_draft[k*B + b]   (k < K_draft)
 *   word 1:                                the accept uniform of slot k     -> u[b*K_accept + k]  (k < K_accept)
 *   word 2, from k == 0 only:              the commit uniform               -> r_commit[b]
 *   word 3: unused
 *   float = (float)(x >> 8) * 2^-24: exact, in [0, 1) (torch.rand's range; 0 is possible, 1 is not)
 * A row's uniforms depend on (seeds[b], step, stage) alone: not on b, B, the other rows, K_draft / K_accept or earlier calls.
 * A NULL output is skipped.  One thread per (b, k), k < max(K_draft, K_accept, 1); no workspace, nothing waits.
 * Status: B < 1, K_draft or K_accept outside [0, ASD_MAX_DRAFT_LEN], NULL seeds, all three outputs NULL, r_draft with
 * K_draft < 1, u with K_accept < 1: invalid argument, nothing launched; seeds not 8-byte or an output not 4-byte aligned:
 * alignment.
 * ---------------------------------------------------------------------------------------- */
int asd_step_uniforms(const int64_t* seeds /*[B], read as uint64*/, uint32_t step, uint32_t stage, int B, int K_draft,
                      int K_accept, float* r_draft /*[K_draft,B] out, may be NULL*/,
                      float* u /*[B,K_accept] out, may be NULL*/, float* r_commit /*[B] out, may be NULL*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * Logit edits: a sparse in-place edit of a few logits per row AHEAD of the samplers -- OpenAI's `logit_bias`, vLLM's
 * `bad_words` / `logit_bias` (a ban, a push) and vLLM's `min_tokens` (the stop ids banned until a row has generated enough).
 * Every sampler above and below admits -inf logits ("no logit > -inf", "a logit of -inf is never listed"), so an edited row is
 * an ordinary input of theirs; applied alike to the draft's proposal rows and the target's K+1 rows, the draft -> verify ->
 * residual chain stays lossless against the EDITED target distribution.
 * logits: B sequences of K1 rows, element (b, j, v) at b*ld_seq + j*ld_row + v (asd_top_logprobs' addressing; K1 == 1 is a
 * [B, V] matrix), bf16 / f16 / f32, edited in place.  ld_row >= V, ld_seq >= K1*ld_row; the padding is never touched.
 * Entries: three parallel DEVICE arrays edit_id / edit_bias / edit_until of n entries.  row_first != NULL: int32 [B+1], row b
 * owns the entries [row_first[b], row_first[b+1]) and n_shared is n, the length of the arrays (indices are clamped into it,
 * so a damaged row_first never leaves them).  row_first == NULL: every row owns the entries [0, n_shared).  At most
 * ASD_MAX_LOGIT_EDITS entries of a row are honoured.
 * One entry (id, bias, until) at position j of row b, with
 *     g = seq_len[b] - start + offset + j
 * the 0-based index, among the row's generated tokens, of the token that logits row decides (start: the prompt length;
 * offset: the draft slot of a proposal row, 0 for the target's rows):
 *     g < until           element id becomes -inf
 *     else, bias != 0     element id becomes round_to_dtype((float)x + bias): one f32 addition, one rounding, to nearest even
 *     else                nothing is stored (the bits stay)
 * until == 0 is a plain bias, until == INT32_MAX a permanent ban, a value between them the min_tokens ban of a stop id (which
 * keeps its bias for afterwards).
 * THE PACKING CONTRACT: inside one row the ids are distinct.  The launcher cannot check device data, so it does not; the
 * kernel relies on it (no two lanes write one element: no atomics) and writes nothing but the named elements, with ordinary
 * per-lane stores.  Likewise the ids themselves cannot be checked by the launcher: an id outside [0, V) is skipped by the
 * kernel, never written.  A bias must be finite; the caller keeps x + bias away from +inf, which the samplers forbid.
 * One launch, one workgroup per (b, j); no workspace, nothing waits.
 * Status, in this order: negative B / K1 / V / n_shared: invalid argument; B == 0, K1 == 0 or n_shared == 0: ASD_OK, nothing
 * launched; unknown dtype, row_first == NULL with n_shared > ASD_MAX_LOGIT_EDITS, B*K1 > INT32_MAX: unsupported; NULL logits /
 * edit_id / edit_bias / edit_until / seq_len, ld_row < V, ld_seq < K1*ld_row: invalid argument; logits not aligned to the
 * element size: alignment.
 * ---------------------------------------------------------------------------------------- */
int asd_logit_edit_rows(void* logits /*in/out*/, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V,
                        const int32_t* edit_id /*[n]*/, const float* edit_bias /*[n]*/, const int32_t* edit_until /*[n]*/,
                        const int32_t* row_first /*[B+1], or NULL: entries [0, n_shared) for every row*/, int n_shared,
                        const int32_t* seq_len /*[B]*/, int start, int offset, void* stream);

/* ------------------------------------------------------------------------------------------
 * Token masks: a DENSE allow-list ahead of the samplers -- vLLM's `allowed_token_ids`, and the [rows, ceil(V/32)] int32
 * bitmask that grammar / structured-output back ends produce.  The complement of a sparse edit: an allow-list of 4 tokens
 * bans V - 4, far beyond ASD_MAX_LOGIT_EDITS.  Like an edited row, a masked row is an ordinary input of every sampler ("no
 * logit > -inf" must hold: a mask that keeps nothing is legal HERE and illegal THERE); applied alike to the draft's proposal
 * rows and the target's K+1 rows, the draft -> verify -> residual chain stays lossless against the masked target distribution.
 * logits: asd_logit_edit_rows' addressing -- element (b, j, v) at b*ld_seq + j*ld_row + v, bf16 / f16 / f32, unit last stride,
 * any ld_row >= V, any ld_seq >= K1*ld_row, the base aligned to the element size only -- edited in place.
 * mask_bits: [R, W] uint32 on the device, W = (V + 31) / 32.  Bit (v & 31) of word (v >> 5) is SET when token v is KEPT.  Bits
 * at v >= V of the last word are ignored, whatever they hold.
 * Which mask: sequence b uses mask r = mask_row[b] (int32 [B] on the device); mask_row == NULL: every sequence uses mask 0.
 * With r < 0 or r >= R the sequence's rows are not touched at all (a mixed batch; a damaged index never leaves the array).
 * Semantics: element v < V of every position j of a masked sequence becomes -inf of the dtype (bits 0xFF80 bf16, 0xFC00 f16,
 * -INFINITY f32, as asd_logit_edit_rows writes a ban) when its bit is clear.  EVERY OTHER element of the allocation keeps its
 * bits: kept elements, the row padding [V, ld_row), the rows of unmasked sequences, whatever lies in front of or behind the
 * tensor.  No logit's VALUE is needed: the launch is a write stream of 16-byte stores of -inf over the chunks whose bits are all
 * clear, with single-element stores in front of a row's first and behind its last 16-byte boundary; a 16-byte chunk whose bits
 * are MIXED is loaded, blended and stored back whole, its kept elements receiving the bits they had (so nothing else may write
 * the tensor while the launch runs, as for any in-place operation); a chunk whose bits are all set is not touched.
 * One launch, grid (B*K1) x S with S chosen by the launcher (a row is cut on mask-word boundaries; the result does not depend
 * on S); no workspace, no atomics, nothing waits on another workgroup.
 * Status, in this order: negative B / K1 / V / R: invalid argument; B, K1, V or R == 0: ASD_OK, nothing launched; unknown
 * dtype, B*K1 > INT32_MAX: unsupported; NULL logits / mask_bits, ld_row < V, ld_seq < K1*ld_row: invalid argument; logits not
 * aligned to the element size or mask_bits not aligned to 4: alignment.
 * ---------------------------------------------------------------------------------------- */
int asd_logit_mask_rows(void* logits /*in/out*/, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V,
                        const uint32_t* mask_bits /*[R, (V+31)/32]*/, int R, const int32_t* mask_row /*[B], or NULL: mask 0*/,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * Bad words: MULTI-token bans ahead of the samplers -- vLLM's `bad_words`, on token ids.  asd_logit_edit_rows bans a token for
 * a whole call; here WHICH logit is banned depends on what the row has just produced, and inside a speculative step on the
 * step's own uncommitted proposals.  A row with banned elements is an ordinary input of every sampler ("no logit > -inf" must
 * hold); applied alike, from the same history, to the draft's proposal rows and the target's K+1 rows, the draft -> verify ->
 * residual chain stays lossless against the target distribution with the bad words removed.
 * logits: asd_logit_edit_rows' addressing -- element (b, j, v) at b*ld_seq + j*ld_row + v, bf16 / f16 / f32, unit last stride,
 * any ld_row >= V, any ld_seq >= K1*ld_row, the base aligned to the element size only; K1 == 1 is a [B, V] matrix -- edited in
 * place.
 * Words: two DEVICE tables in asd_commit_step_finish's layout: word_tok int32 [n, ASD_MAX_BAD_WORD_LEN], word w's ids
 * w_0 .. w_{m-1} at word_tok[w][0 .. m) with m = word_n[w] in 1..ASD_MAX_BAD_WORD_LEN (the padding behind them is never
 * looked at).  row_first != NULL: int32 [B+1], sequence b owns the words [row_first[b], row_first[b+1]) and n_shared is n, the
 * number of words in the tables (indices are clamped into [0, n_shared], so a damaged row_first never leaves them).
 * row_first == NULL: every sequence owns the words [0, n_shared).  At most ASD_MAX_BAD_WORDS words of a sequence are honoured.
 * History: position j of sequence b has
 *     H = tokens[b][start .. seq_len[b])  ++  step_tok[b][0 .. n_prev + j)
 * tokens: int32 rows ld_tokens >= max_len elements apart; seq_len[b], as it stands BEFORE the step's commit, is clamped into
 * [start, max_len].  The prompt and its padding in front of `start` are NOT history (vLLM matches over the output only).
 * step_tok: int32 [B] rows of n_tok proposals, ld_tok >= n_tok elements apart: the tokens the step has proposed and not
 * committed (asd_penalty_rows' argument): a proposal row of draft slot k is K1 = 1 with n_prev = k, the target's K+1 rows are
 * n_prev = 0, and row j of them sees the proposals 0 .. j-1.  step_tok == NULL: no position sees a proposal, and n_prev must be
 * 0.  n_tok <= ASD_MAX_DRAFT_LEN.
 * Semantics: element w_{m-1} of position (b, j) becomes -inf of the dtype (bits 0xFF80 bf16, 0xFC00 f16, -INFINITY f32, the
 * ones asd_logit_edit_rows and asd_logit_mask_rows write) when BOTH
 *     len(H) >= m - 1
 *     the last m - 1 tokens of H equal w_0 .. w_{m-2}
 * hold; a word with m == 1 always bans its token.  Nothing else is written: a matched element that is already -inf may be
 * stored again, every other bit of the allocation stays as it was.  A rejected proposal never reaches `tokens`: nothing is
 * rolled back, and the operation keeps no state.
 * THE DATA CONTRACT: the launcher cannot check device data, so the kernel does: a word with word_n outside
 * 1..ASD_MAX_BAD_WORD_LEN, or with a last id outside [0, V), is skipped, never written; prefix ids, committed tokens and
 * proposals are compared as plain integers and index nothing.  Two words of one sequence MAY end in the same id (and the host
 * need not remove that): both lanes then store the same -inf bits to one element with ordinary per-lane vector-memory stores,
 * which gives the same result in either order -- no atomics.
 * One launch, one workgroup of ASD_MAX_BAD_WORDS threads per (b, j), lane t handling word t of the sequence: at most
 * ASD_MAX_BAD_WORD_LEN - 1 independent history loads and one store per lane.  No loop over the vocabulary, no LDS, no
 * workspace, nothing waits on another workgroup.
 * Status, in this order: negative B / K1 / V / n_shared / n_tok / n_prev / start / max_len: invalid argument; B, K1, V or
 * n_shared == 0: ASD_OK, nothing launched; unknown dtype, row_first == NULL with n_shared > ASD_MAX_BAD_WORDS,
 * n_tok > ASD_MAX_DRAFT_LEN, B*K1 > INT32_MAX: unsupported; NULL logits / word_tok / word_n / tokens / seq_len, ld_row < V,
 * ld_seq < K1*ld_row, ld_tokens < max_len, start > max_len, step_tok == NULL with n_prev != 0, step_tok != NULL with
 * n_prev + K1 - 1 > n_tok or ld_tok < n_tok: invalid argument; logits not aligned to the element size, or word_tok / word_n /
 * row_first / tokens / seq_len / step_tok not aligned to 4: alignment.
 * ---------------------------------------------------------------------------------------- */
int asd_bad_words_rows(void* logits /*in/out*/, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V,
                       const int32_t* word_tok /*[n, ASD_MAX_BAD_WORD_LEN]*/, const int32_t* word_n /*[n]*/,
                       const int32_t* row_first /*[B+1], or NULL: words [0, n_shared) for every row*/, int n_shared,
                       const int32_t* tokens /*[B, ld_tokens]*/, int64_t ld_tokens, const int32_t* seq_len /*[B]*/,
                       int start, int max_len,
                       const int32_t* step_tok /*[B, ld_tok], or NULL*/, int64_t ld_tok, int n_tok, int n_prev, void* stream);

/* ------------------------------------------------------------------------------------------
 * No repeated n-gram AHEAD of the samplers -- HF generate's `no_repeat_ngram_size` (NoRepeatNGramLogitsProcessor).  The
 * "words" of asd_bad_words_rows are given by the caller; here they are every n-gram of the row's own history, so the kernel
 * scans the history instead of a table.  A row with banned elements is an ordinary input of every sampler ("no logit > -inf"
 * must hold: a position bans at most len(H) - n + 1 tokens, which the host can bound before the call); applied alike, from the
 * same history, to the draft's proposal rows and the target's K+1 rows, the draft -> verify -> residual chain stays lossless
 * against the target distribution with the repeating tokens removed.
 * logits: asd_bad_words_rows' addressing -- element (b, j, v) at b*ld_seq + j*ld_row + v, bf16 / f16 / f32, unit last stride,
 * any ld_row >= V, any ld_seq >= K1*ld_row, the base aligned to the element size only; K1 == 1 is a [B, V] matrix -- edited in
 * place.
 * n: ngram_n != NULL: int32 [B], sequence b has n = ngram_n[b]; 0 switches the row off, a value outside
 * 1..ASD_MAX_NGRAM skips the row.  ngram_n == NULL: every sequence has n = n_shared, in 0..ASD_MAX_NGRAM.
 * History: position j of sequence b has
 *     H = tokens[b][row_start[b] .. L)  ++  step_tok[b][0 .. n_prev + j),      L = clamp(seq_len[b], start, max_len)
 * tokens: int32 rows ld_tokens >= max_len elements apart, only read; seq_len[b] is the length as it stands BEFORE the step's
 * commit.  `start` is the (padded) prompt length; row_start != NULL: int32 [B], the index of the row's first REAL prompt id,
 * clamped into [0, start]: the prompt counts as history (as in HF for decoder-only models), the left-padding in front of it
 * does not.  row_start == NULL: `start` for every row (no prompt in the history).  step_tok, ld_tok, n_tok, n_prev: as in
 * asd_bad_words_rows -- a proposal row of draft slot k is K1 = 1 with n_prev = k, the target's K+1 rows are n_prev = 0, and
 * row j of them sees the proposals 0 .. j-1; step_tok == NULL: no position sees a proposal, and n_prev must be 0.
 * Semantics: for every i in [0, len(H) - n] with
 *     H[i .. i+n-1) == H[len(H)-n+1 .. len(H))          (n - 1 tokens on either side)
 * element H[i+n-1] of position (b, j) becomes -inf of the dtype (bits 0xFF80 bf16, 0xFC00 f16, -INFINITY f32, the ones
 * asd_logit_edit_rows, asd_logit_mask_rows and asd_bad_words_rows write).  With n == 1 the compared run is empty: every token
 * of H is banned.  With len(H) < n nothing is banned.  Nothing else is written: a matched element that is already -inf may be
 * stored again, every other bit of the allocation stays as it was.  A rejected proposal never reaches `tokens`: nothing is
 * rolled back, and the operation keeps no state.
 * THE DATA CONTRACT: the launcher cannot check device data, so the kernel does: seq_len[b] is clamped into [start, max_len],
 * row_start[b] into [0, start], a row with ngram_n[b] outside 1..ASD_MAX_NGRAM is skipped, and a history token outside [0, V)
 * is compared as a plain integer but never used as a store index.
 * One launch: a workgroup of 256 threads per (b, j) and per slice of ASD_NGRAM_SLICE n-gram starts (the number of slices
 * follows max_len + n_tok, so a long context is not walked by one workgroup); each lane compares the LAST suffix token first
 * and stores with ordinary per-lane vector-memory stores; several lanes and slices may store the same bits to one element, in
 * either order the same result.  No atomics, no loop over the vocabulary, no LDS, no workspace, nothing waits on another
 * workgroup.
 * Status, in this order: negative B / K1 / V / n_shared / n_tok / n_prev / start / max_len: invalid argument; B, K1 or V == 0,
 * or ngram_n == NULL with n_shared == 0: ASD_OK, nothing launched; unknown dtype, ngram_n == NULL with
 * n_shared > ASD_MAX_NGRAM, n_tok > ASD_MAX_DRAFT_LEN, B*K1 > INT32_MAX, max_len + n_tok > INT32_MAX - 256: unsupported; NULL
 * logits / tokens / seq_len, ld_row < V, ld_seq < K1*ld_row, ld_tokens < max_len, start > max_len, step_tok == NULL with
 * n_prev != 0, step_tok != NULL with n_prev + K1 - 1 > n_tok or ld_tok < n_tok: invalid argument; logits not aligned to the
 * element size, or ngram_n / row_start / tokens / seq_len / step_tok not aligned to 4: alignment.
 * ---------------------------------------------------------------------------------------- */
int asd_no_repeat_ngram_rows(void* logits /*in/out*/, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V,
                             const int32_t* ngram_n /*[B], or NULL: n_shared for every row*/, int n_shared,
                             const int32_t* row_start /*[B], or NULL: start for every row*/,
                             const int32_t* tokens /*[B, ld_tokens]*/, int64_t ld_tokens, const int32_t* seq_len /*[B]*/,
                             int start, int max_len,
                             const int32_t* step_tok /*[B, ld_tok], or NULL*/, int64_t ld_tok, int n_tok, int n_prev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Entropy cuts AHEAD of the samplers -- HF's TypicalLogitsWarper (`typical_p`), EpsilonLogitsWarper (`epsilon_cutoff`) and
 * EtaLogitsWarper (`eta_cutoff`), each with min_tokens_to_keep = 1.  They are no threshold on the sorted probabilities: all
 * three need the row's entropy or its exact probabilities, and typical-p may cut the arg-max.  One in-place pass, the last one
 * ahead of the draw, applied alike to the draft's proposal rows and the target's K+1 rows; top-k, top-p and min-p then act on
 * the survivors.
 * logits: asd_no_repeat_ngram_rows' addressing -- element (b, j, v) at b*ld_seq + j*ld_row + v, bf16 / f16 / f32, unit last
 * stride, any ld_row >= V, any ld_seq >= K1*ld_row, the base aligned to the element size only.
 * table: B records {float inv_t; int32 mode; float value} (asd_entropy_cut_rec, 12 bytes) on the device; all K1 rows of
 * sequence b use record b.  The row's distribution is p = softmax(x * inv_t) of the row as it stands (whatever is -inf carries no
 * mass and stays -inf), H = -sum p ln p its entropy in nats.
 *   ASD_CUT_OFF (0): the row is not read.
 *   ASD_CUT_TYPICAL (1), value = m in (0, 1): d_v = |-ln p_v - H|; d* is the smallest value with sum{p_v : d_v <= d*} >= m;
 *     element v is cut iff d_v > d*.  Every tie at d* is kept; when the mass never reaches m nothing is cut; the arg-max may be.
 *   ASD_CUT_EPSILON (2), value = e in (0, 1): element v is cut iff p_v < e and x_v < x_max (every element that ties the
 *     maximum survives).
 *   ASD_CUT_ETA (3), value = e in (0, 1): the same with min(e, sqrt(e) * exp(-H)) in place of e.
 * A cut element becomes -inf of the dtype (0xFF80 bf16, 0xFC00 f16, -INFINITY f32); nothing else is written, and a 16-byte
 * vector is stored only where a bit of it changes.  A row with a NaN or +inf element, or without a finite element, has no
 * distribution and is left exactly as it is.  THE DATA CONTRACT: a record whose mode lies outside 0..3, whose value lies
 * outside (0, 1) or whose inv_t is not a positive finite number skips its rows.
 * Arithmetic: one workgroup of 1024 threads per (b, j).  The first sweep takes (m2, s, u) as asd_token_stats does (u: the
 * entropy's running sum relative to the running maximum) and the exact maximum, merged lanes -> waves in a fixed order; then
 * log2 p_v = fma(x_v, c2, -L.hi) - L.lo with c2 = float(log2(e) * inv_t) and L = m2 + log2 s in two floats.  Epsilon / eta:
 * one more sweep compares log2 p_v with log2 of the bound.  Typical: the key of v is |fma(x_v, c2, -A.hi) - A.lo| with
 * A = L - H / ln 2, and an ascending radix select (12 + 12 + 8 bits of the key's order-preserving integer) on the masses
 * floor(p_v 2^40), summed in integer counters, finds the key at which the mass reaches floor(m 2^40); a last sweep cuts what lies
 * above it.  The result depends on the row's bytes and its record only.  No workspace, no state.
 * Status, in this order: negative B / K1 / V: invalid argument; B, K1 or V == 0: ASD_OK, nothing launched; unknown dtype,
 * B*K1 > INT32_MAX, V * element size > INT32_MAX: unsupported; NULL logits / table, ld_row < V, ld_seq < K1*ld_row: invalid
 * argument; logits not aligned to the element size, or table not aligned to 4: alignment.
 * ---------------------------------------------------------------------------------------- */
#define ASD_CUT_OFF 0
#define ASD_CUT_TYPICAL 1
#define ASD_CUT_EPSILON 2
#define ASD_CUT_ETA 3
#define ASD_ENTROPY_CUT_REC_BYTES 12
typedef struct asd_entropy_cut_rec {
    float inv_t;   /* 1 / temperature of the sequence */
    int32_t mode;  /* ASD_CUT_* */
    float value;   /* typical_p, epsilon_cutoff or eta_cutoff */
} asd_entropy_cut_rec;
int asd_entropy_cut_rows(void* logits /*in/out*/, int dtype, int B, int K1, int V, int64_t ld_seq, int64_t ld_row,
                         const asd_entropy_cut_rec* table /*[B]*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * Guided decoding: a token-level deterministic automaton (FSM) per sequence, AHEAD of the samplers -- what grammar /
 * structured-output back ends compile a set of answers, a regex or a schema to.  Inside a speculative step the mask of
 * position j depends on the proposals 0 .. j-1, which exist only on the device: so the state lives there, small kernels
 * advance it, and the mask is chosen per (sequence, position).  Applied alike, from the same history, to the draft's proposal
 * rows and the target's K+1 rows, the draft -> verify -> residual chain stays lossless against the grammar-restricted target
 * distribution.
 * TABLES (device, int32 unless stated; one state space of S states and E edges for the whole call):
 *   state_first [S+1]  CSR offsets: state s owns the edges [state_first[s], state_first[s+1])
 *   edge_tok    [E]    the edges' token ids, ASCENDING and DISTINCT within a state
 *   edge_next   [E]    the edges' next states; -1: the token is forbidden in that state
 *   state_other [S]    the next state of every token WITHOUT an edge in s; -1: such tokens are forbidden
 *   state_bits  uint32 [S, W], W = (V+31)/32, asd_logit_mask_rows' bit layout: bit v & 31 of word v >> 5 of row s SET = token v
 *               has a transition in s that is not -1.  Built by the host from the other four; bits at v >= V are never looked at.
 *   pos_state   [B] rows of ld_state columns: column 0 is the state behind the sequence's committed tokens, column i the
 *               state behind the proposals 0 .. i-1 of the running step.  A sequence without an automaton holds -1.
 * THE TRANSITION delta(s, t):
 *     s outside [0, S)                                   -> s (no automaton, or damaged data)
 *     t has an edge in s                                 -> that edge's next state
 *     t has no edge in s                                 -> state_other[s]
 *     that result outside [0, S) (-1: forbidden), or t outside [0, V)   -> s
 * The last line cannot occur in correct operation -- every proposal was drawn from masked logits -- and mapping it to "s
 * unchanged" means a sequence never loses its non-empty mask.
 *
 * asd_fsm_mask_rows: logits in asd_logit_edit_rows' addressing (element (b, j, v) at b*ld_seq + j*ld_row + v, bf16 / f16 / f32,
 * unit last stride, any ld_row >= V, any ld_seq >= K1*ld_row, the base aligned to the element size only), masked in place:
 * position j of sequence b with row s = pos_state[b][first + j] of state_bits -- element v becomes -inf of the dtype (the bits
 * asd_logit_mask_rows writes) where bit v of row s is clear; s outside [0, S) leaves the position alone.  Nothing else in the
 * allocation is written.  This is asd_logit_mask_rows with a mask index per (b, j) instead of per b, and the same write stream
 * (one shared kernel body): 16-byte all-clear stores, mixed chunks loaded, blended and stored whole, single elements in front
 * of the first and behind the last 16-byte boundary, grid (B*K1) x slices of whole mask words.
 * Status, in this order: negative B / K1 / V / S / first / ld_state: invalid argument; B, K1, V or S == 0: ASD_OK, nothing
 * launched; unknown dtype, B*K1 > INT32_MAX: unsupported; NULL logits / state_bits / pos_state, ld_row < V, ld_seq < K1*ld_row,
 * first + K1 > ld_state: invalid argument; logits not aligned to the element size, state_bits / pos_state not to 4: alignment.
 *
 * asd_fsm_advance: pos_state[b][k+1] = delta(pos_state[b][k], step_tok[b][k]) for every sequence -- behind proposal k of a
 * step, for every k including the last, so that column K exists for the target's bonus row.  step_tok: int32 [B] rows of n_tok
 * proposals, ld_tok >= n_tok apart (asd_bad_words_rows' argument).
 * Status, in this order: negative B / S / E / V / k / n_tok / ld_state: invalid argument; B == 0: ASD_OK; n_tok >
 * ASD_MAX_DRAFT_LEN: unsupported; NULL state_first / state_other / pos_state / step_tok, NULL edge_tok / edge_next with E > 0,
 * k + 1 >= ld_state, k >= n_tok, ld_tok < n_tok: invalid argument; a pointer not aligned to 4: alignment.
 *
 * asd_fsm_commit: behind the step's commit, which left seq_len and n_commit.  For a sequence with c = n_commit[b] > 0, c
 * clamped to ld_state and L = seq_len[b] clamped into [1, max_len]:
 *     pos_state[b][0] = delta(pos_state[b][c-1], tokens[b][L-1])
 * One transition is enough: the first c-1 committed tokens of a step are always its accepted proposals 0 .. c-2 (stop rules
 * and length limits cut from the END), so column c-1 already is the state behind them.  c <= 0 (a finished sequence) leaves
 * the state as it is.  tokens: int32 rows ld_tokens >= max_len apart.
 * Status, in this order: negative B / S / E / V / max_len / ld_state: invalid argument; B == 0: ASD_OK; NULL state_first /
 * state_other / pos_state / tokens / seq_len / n_commit, NULL edge_tok / edge_next with E > 0, ld_state < 1, max_len < 1,
 * ld_tokens < max_len: invalid argument; a pointer not aligned to 4: alignment.
 *
 * Both small kernels: one launch, ONE WAVE per sequence, on the serial draft path where latency counts, not bytes.  The wave
 * searches the state's sorted edge range cooperatively -- one probe per lane per round, a wave ballot picks the bracket -- in at
 * most ceil(log64(n_edges)) dependent rounds (3 at a vocabulary-sized state, against 18 for a per-lane binary search).  No LDS,
 * no atomics, no workspace; the result is one ordinary per-lane vector-memory store.  THE DATA CONTRACT: the launchers cannot
 * check device data, so the kernels do: the edge range of a state is clamped into [0, E], tokens and states are compared as
 * plain integers, and a state indexes the tables only inside [0, S).
 * ---------------------------------------------------------------------------------------- */
int asd_fsm_mask_rows(void* logits /*in/out*/, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V,
                      const uint32_t* state_bits /*[S, (V+31)/32]*/, int S, const int32_t* pos_state /*[B, ld_state]*/,
                      int64_t ld_state, int first, void* stream);
int asd_fsm_advance(const int32_t* state_first /*[S+1]*/, const int32_t* edge_tok /*[E]*/, const int32_t* edge_next /*[E]*/,
                    const int32_t* state_other /*[S]*/, int S, int E, int V, int32_t* pos_state /*[B, ld_state] in/out*/,
                    int64_t ld_state, int B, int k, const int32_t* step_tok /*[B, ld_tok]*/, int64_t ld_tok, int n_tok,
                    void* stream);
int asd_fsm_commit(const int32_t* state_first /*[S+1]*/, const int32_t* edge_tok /*[E]*/, const int32_t* edge_next /*[E]*/,
                   const int32_t* state_other /*[S]*/, int S, int E, int V, int32_t* pos_state /*[B, ld_state] in/out*/,
                   int64_t ld_state, int B, const int32_t* tokens /*[B, ld_tokens]*/, int64_t ld_tokens,
                   const int32_t* seq_len /*[B]*/, const int32_t* n_commit /*[B]*/, int max_len, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stateful penalties AHEAD of the samplers and behind the mask and the edit -- vLLM's `apply_penalties`: repetition_penalty,
 * presence_penalty, frequency_penalty.  A penalised row is an ordinary input of every sampler; applied alike, from the same
 * history, to the draft's proposal rows and the target's K+1 rows, the draft -> verify -> residual chain stays lossless against
 * the PENALISED target distribution.
 * State, DEVICE arrays kept by the caller for one generation: seen uint32 [B, W], W = (V + 31) / 32, in asd_logit_mask_rows'
 * bit layout -- bit (v & 31) of word (v >> 5) of row b SET when token v occurs in sequence b's prompt or among its committed
 * generated tokens (bits at v >= V are ignored) -- and counts int32 [B, V], the occurrences of v among sequence b's committed
 * generated tokens (the prompt is not counted).  THE STATE CONTRACT: counts[b][v] > 0 only where the bit is set;
 * asd_penalty_commit keeps it.  counts is read only where the bit is set or the token is one of the step's proposals.
 * params float [B, 3]: (rep, pres, freq) of sequence b.  rep <= 0 or NaN reads as 1.  A sequence with (1, 0, 0) is not touched.
 *
 * asd_penalty_rows: logits in asd_logit_edit_rows' addressing -- element (b, j, v) at b*ld_seq + j*ld_row + v, bf16 / f16 / f32,
 * K1 == 1 is a [B, V] matrix -- edited in place.  step_tok: int32 [B] rows of n_tok proposals, ld_tok >= n_tok elements apart:
 * the tokens the step has proposed and NOT committed.  Position j of sequence b sees step_tok[b][0 .. n_prev + j): a proposal
 * row of draft slot k is K1 = 1 with n_prev = k, the target's K+1 rows are n_prev = 0.  step_tok == NULL: no position sees a
 * proposal, and n_prev must be 0.  A proposal outside [0, V) is skipped.  n_tok <= ASD_MAX_DRAFT_LEN.
 * At (b, j), token v is SEEN when its bit is set or it is among the proposals the position sees, and c is counts[b][v] plus
 * its occurrences among them.  In f32, in exactly this order, without fused multiply-add, the division correctly rounded:
 *     y = x
 *     if seen and rep != 1:   y = (x > 0) ? x / rep : x * rep
 *     if c > 0:               y = y - freq * (float)c;   y = y - pres
 * and the element becomes round_to_dtype(y), one rounding to nearest even -- except that nothing is stored where y == x (an
 * element that is neither seen nor counted, a -inf, a zero keep their bits), and that a result which rounds to +inf (f16 with
 * rep < 1; an f32 overflow) is stored as the dtype's largest finite value: the samplers forbid +inf.  Nothing but such
 * elements is written: the row padding, neutral sequences and everything around the tensor keep their bits.
 * One launch, grid B x S with S chosen by the launcher (a row's mask words are cut into slices of whole words; the result does
 * not depend on S); the cost follows the number of distinct seen tokens, not V.  Every element is written by at most one lane
 * of one workgroup: no atomics, no workspace, nothing waits on another workgroup.
 * Status, in this order: negative B / K1 / V / n_tok / n_prev: invalid argument; B, K1 or V == 0: ASD_OK, nothing launched;
 * unknown dtype, n_tok > ASD_MAX_DRAFT_LEN: unsupported; NULL logits / seen / counts / params, ld_row < V,
 * ld_seq < K1*ld_row, step_tok == NULL with n_prev != 0, step_tok != NULL with n_prev + K1 - 1 > n_tok or ld_tok < n_tok:
 * invalid argument; logits not aligned to the element size, or seen / counts / params / step_tok not aligned to 4: alignment.
 * ---------------------------------------------------------------------------------------- */
int asd_penalty_rows(void* logits /*in/out*/, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V,
                     const uint32_t* seen /*[B, (V+31)/32]*/, const int32_t* counts /*[B, V]*/, const float* params /*[B, 3]*/,
                     const int32_t* step_tok /*[B, ld_tok], or NULL*/, int64_t ld_tok, int n_tok, int n_prev, void* stream);

/* asd_penalty_commit: behind the step's commit kernel (asd_commit_step_lp / _stop / _finish, which left seq_len and n_commit),
 * the n_commit[b] tokens at tokens[b][seq_len[b] - n_commit[b] .. seq_len[b]) enter sequence b's state: counts[b][v] grows by
 * the multiplicity of v among them and the bit of v is set.  tokens: int32 rows ld_tokens >= max_len elements apart.
 * n_commit[b] is clamped into [0, ASD_MAX_DRAFT_LEN + 1], a position into [0, max_len), and a token outside [0, V) is skipped,
 * so damaged inputs never leave the arrays.  The commit kernels leave n_commit == 0 for a finished sequence: its state is
 * frozen.  Rejected proposals were never written to `tokens`: there is nothing to roll back.
 * One launch, one workgroup per sequence; a token committed twice in one step is counted by ONE lane (its first occurrence),
 * the bit is set with a vector atomic OR (two tokens may share a word).
 * Status, in this order: negative B / V / max_len: invalid argument; B, V or max_len == 0: ASD_OK, nothing launched; NULL
 * tokens / seq_len / n_commit / seen / counts, ld_tokens < max_len: invalid argument; a pointer not aligned to 4: alignment. */
int asd_penalty_commit(const int32_t* tokens /*[B, ld_tokens]*/, int64_t ld_tokens, const int32_t* seq_len /*[B]*/,
                       const int32_t* n_commit /*[B]*/, int B, int V, int max_len, uint32_t* seen /*in/out [B, (V+31)/32]*/,
                       int32_t* counts /*in/out [B, V]*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * A7  log-prob statistics: features [5..9] of extract_features,
 * src/training/generate_training_data.py:166-175 -- np.mean, np.std (population), np.min,
 * np.percentile(.,25) (linear interpolation), np.median, all in float64 like numpy.
 * lp: [B rows][<=K valid] f32, rows `ld` elements apart; n_valid[b] in [0,K] (NULL => K).
 * n_valid[b]==0 => five zeros (reference: `features.extend([0.0]*5)`, :174-175).
 * stats: [B,5] f64.
 * ---------------------------------------------------------------------------------------- */
int asd_logprob_stats(const float* lp, int64_t ld, const int32_t* n_valid, int B, int K,
                      double* stats /*[B,5] out*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * A8  MinimalQualityPredictor.forward in eval mode, src/minimal_adaptive_decoder.py:38-49:
 *   score = sigmoid(W2 . relu(W1 x + b1) + b2)          (Dropout(0.1) == identity)
 * packed_w (f32): W1T [in_dim][hidden] (= net.0.weight transposed), b1 [hidden],
 *                 W2 [hidden] (= net.3.weight[0]), b2 [1]   => in_dim*hidden + 2*hidden + 1.
 * asd_mlp_pack_weights (host pointers) builds that buffer from the state_dict tensors.
 * ---------------------------------------------------------------------------------------- */
size_t asd_mlp_packed_floats(int in_dim, int hidden);
int asd_mlp_pack_weights(const float* w1 /*host [hidden,in_dim]*/, const float* b1 /*host*/,
                         const float* w2 /*host [hidden]*/, const float* b2 /*host [1]*/,
                         int in_dim, int hidden, float* packed /*host out*/);
int asd_mlp_predict(const float* x /*[B rows][in_dim], rows ldx apart*/, int64_t ldx,
                    const float* packed_w, int B, int in_dim, int hidden,
                    float* score /*[B] out*/, void* stream);

/* A11  stop test of MinimalAdaptiveDecoder.decode, src/minimal_adaptive_decoder.py:153-164:
 *   stage[b] = first s in [0,L) with (double)score[b] >= theta[s], or s == L-1. */
int asd_threshold_stop(const float* score /*[B]*/, const double* theta /*[L]*/, int B, int L,
                       int32_t* stage /*[B] out*/, void* stream);

/* A2  bayesian_adjustment, src/algorithms/dp_solver.py:106-130 (f64, no FMA contraction):
 *   a = n_obs*p + alpha;  b = n_obs*(1-p) + beta;  out = a / (a + b) */
int asd_bayes_adjust(const double* p /*[n]*/, int64_t n_obs, double alpha, double beta, int n,
                     double* out /*[n] out*/, void* stream);

/* A1  optimal_stopping_rule, src/algorithms/dp_solver.py:12-71, batched over B requests.
 *   p: [B,L] f64; C: [L] f64 shared by the batch; lam f64.
 *   risk_adjustment != 0 applies bayesian_adjustment(p, n_obs=100, alpha, beta) first (:38-39).
 *   k_star: [B] i32; J: [B,L+1] f64 (may be NULL).  Bit-exact with CPython float arithmetic. */
int asd_optimal_stopping(const double* p, const double* C, double lam, int B, int L,
                         int risk_adjustment, double alpha, double beta,
                         int32_t* k_star, double* J, void* stream);

/* A3  compute_expected_cost, dp_solver.py:74-103: sum(C[:k+1]) + lam*(1 - prod(p[:k+1])),
 * for a per-request stopping stage k[b] in [0,L). */
int asd_expected_cost(const double* p /*[B,L]*/, const double* C /*[L]*/, double lam,
                      const int32_t* k /*[B]*/, int B, int L, double* cost /*[B] out*/,
                      void* stream);

/* N4  the DP rule over a GRID of lambda values in one launch: what a lambda controller
 * (src/algorithms/optimizer.py:47-205 LambdaOptimizer, :261-335 GridSearchOptimizer) needs per candidate
 * when requests are described by their predicted stage probabilities.  For every lam[g] and request b:
 *   k_star[g,b]  optimal_stopping_rule(p[b], C, lam[g], risk_adjustment, alpha, beta)      (dp_solver.py:12-71)
 *   cost[g,b]    sum(C[:k*+1]),   p_ok[g,b] = prod(p[b,:k*+1])     (the two terms of compute_expected_cost,
 *                dp_solver.py:74-103: expected cost = cost + lam * (1 - p_ok)).  cost / p_ok may be NULL. */
int asd_lambda_sweep(const double* p /*[B,L]*/, const double* C /*[L]*/, const double* lam /*[G]*/,
                     int B, int L, int G, int risk_adjustment, double alpha, double beta,
                     int32_t* k_star /*[G,B]*/, double* cost /*[G,B]*/, double* p_ok /*[G,B]*/, void* stream);

/* A10  OptimalStoppingTheory.derive_optimal_policy, src/theory/optimal_stopping.py:45-82
 * (+ _compute_improvement_probability :84-91).  HOST pointers: an O(n) f64 recursion run once
 * per set_lambda; theta[n] (theta[n-1] = 0), V[n+1] (may be NULL). */
int asd_derive_thresholds(const double* q, const double* c, int n, double lam,
                          double* theta, double* V);

/* ------------------------------------------------------------------------------------------
 * Fused post-verify epilogue (first form): one launch per tier step does
 *   stats   = logprob_stats(lp[b, :n_valid[b]])                      (A7)
 *   x       = feat[b,:] with x[stats_col .. stats_col+5) = (f32)stats (stats_col < 0: untouched)
 *   score   = mlp(x)                                                  (A8)
 *   p_adj   = risk_adjustment ? bayes(score, n_obs, alpha, beta) : score   (A2, pipeline.py:234-238)
 *   p_hist[b, stage_idx] = p_adj            (p_hist: [B,L] f64, columns < stage_idx are inputs)
 *   k_star  = optimal_stopping_rule(p_hist[b,:n_dp], C[:n_dp], lam)   (A1)  n_dp = prefix ? stage_idx+1 : L
 *             (columns > stage_idx are read as given: the caller pre-fills priors, 1.0 for the last)
 *   theta != NULL additionally:  thr_stop[b] = (double)score >= theta[stage_idx] || stage_idx == L-1   (A11)
 *   stop[b] = (k_star == stage_idx)
 * Outputs that are NULL are skipped.  feat rows are ldf apart and are NOT modified.
 * ---------------------------------------------------------------------------------------- */
int asd_predictor_stop(const float* lp /*[B,K]*/, int64_t ld_lp, const int32_t* n_valid, int K,
                       const float* feat /*[B,in_dim]*/, int64_t ldf, int stats_col,
                       const float* packed_w, int in_dim, int hidden,
                       int risk_adjustment, int64_t n_obs, double alpha, double beta,
                       double* p_hist /*[B,L] in/out*/, const double* C /*[L]*/, double lam,
                       int L, int stage_idx, int prefix_rule,
                       const double* theta /*[L] or NULL*/, int B,
                       float* score /*[B]*/, int32_t* k_star /*[B]*/, uint8_t* stop /*[B]*/,
                       uint8_t* thr_stop /*[B]*/, double* stats /*[B,5]*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * The token a speculative step COMMITS after its accepted prefix (no reference symbol).
 * For sequence b with j = n_acc[b]:
 *   j <  K : w(v) = max(0, softmax(t_logits[b,j]/T)(v) - softmax(d_logits[b,j]/T)(v))   (residual distribution;
 *            if it is empty, i.e. p_t <= p_d everywhere, w = softmax(t_logits[b,j]/T))
 *   j >= K : w(v) = softmax(bonus_logits[b]/T)(v)      (all drafted tokens accepted; bonus_logits NULL => token -1)
 *   token[b] = min { v : sum_{v' <= v} w(v') > r[b] * sum_v w(v) }        (inverse CDF in vocabulary order)
 * t_logits / d_logits: [B*K rows][V], bonus_logits: [B rows][V], all of `dtype`, rows ld_* ELEMENTS apart,
 * 16-byte aligned and a whole number of 16-byte vectors (ASD_ERR_ALIGNMENT otherwise).  r: [B] uniforms in [0,1).
 * workspace: >= asd_residual_sample_workspace_bytes(B, V, dtype), 256-byte aligned, zero-initialised ONCE with asd_workspace_init
 * (since 0.2: up to 64 sequences every sequence's two rows are spread over 2 ... 32 workgroups inside ONE launch, whose single-writer /
 * single-reader mailboxes live in the workspace and are handed back empty by every call; larger batches use the multi-launch /
 * one-workgroup-per-sequence forms, which need no initialisation).  A hand-off that never arrives poisons the sequence (token -1).
 * ---------------------------------------------------------------------------------------- */
size_t asd_residual_sample_workspace_bytes(int B, int V, int dtype);
int asd_residual_sample(const void* t_logits, int64_t ld_t, const void* d_logits, int64_t ld_d,
                        const void* bonus_logits, int64_t ld_b, int dtype,
                        const int32_t* n_acc /*[B]*/, const float* r /*[B]*/, int B, int K, int V,
                        float inv_temperature, int32_t* token /*[B] out*/,
                        void* workspace, size_t workspace_bytes, void* stream);

/* asd_residual_sample for drafts that were drawn with nucleus (top-p) truncation (asd_draft_sample below): the draft
 * distribution at row (b,k) is softmax(d_logits[b,k]/T) restricted to logits >= d_threshold[b,k] and renormalised --
 * the distribution the drafted token was actually drawn from, so the residual max(0, p_t - p_d) stays exact.
 * d_threshold: [B,K] f32 (asd_draft_sample's nucleus_logit per drafted position); NULL == asd_residual_sample. */
int asd_residual_sample_ex(const void* t_logits, int64_t ld_t, const void* d_logits, int64_t ld_d,
                           const void* bonus_logits, int64_t ld_b, int dtype,
                           const int32_t* n_acc, const float* r, int B, int K, int V,
                           float inv_temperature, const float* d_threshold /*[B,K] or NULL*/, int32_t* token,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * X1  the draft tier's per-step token proposal (north star piece (i)).  The reference delegates it to
 * HF `model.generate(do_sample=True, temperature=0.7, top_p=0.9)` (src/training/generate_training_data.py:110-119;
 * third-party arithmetic, parity unpinned); torch needs log_softmax + multinomial + gather over [B,V] per token.
 * One call per drafted position, for row b (one next-token logits row per sequence):
 *   q(v)   = softmax(logits[b]/T)(v) for v in the nucleus N_b, 0 outside, renormalised over N_b
 *   N_b    = { v : logits[b,v] >= x*_b },  x*_b = the LARGEST logit value with  sum_{logits[b,v] >= x*} softmax(.)(v) >= top_p
 *            (HF's TopPLogitsWarper set, with every token tied at the boundary value kept);  top_p outside (0,1): all v
 *   tok[b] = min { v in N_b : sum_{v' in N_b, v' <= v} q(v') > r[b] }          (inverse CDF in vocabulary order, r in [0,1))
 *   lp[b]  = log q(tok[b])                                       (the lp_draft the verify step needs; may be NULL)
 *   nucleus_logit[b] = x*_b (-inf without truncation; may be NULL): with it asd_residual_sample_ex reconstructs q exactly.
 * logits: [B rows][V] of `dtype`, rows ld ELEMENTS apart, 16-byte aligned, a whole number of 16-byte vectors.
 * Rows must not contain NaN / +inf.  ONE launch; V*sizeof(elem) <= 2 MiB.
 * Geometry: up to 128 rows, every row is spread over G = 2 ... 32 workgroups (~one per compute unit) that keep their part
 * of the row in registers and meet through single-writer / single-reader mailbox words in `workspace`; more rows, or a NULL /
 * short workspace: one streaming 1024-lane workgroup per row.  The per-tile partial sums are canonical and folded in a
 * fixed order, so tok / lp / nucleus_logit do NOT depend on the geometry (lp and nucleus_logit bit for bit; the token
 * wherever the draw is more than a float rounding away from a tile boundary of the CDF).
 * workspace: asd_draft_sample_workspace_bytes(B,V,dtype) bytes (~25 MB), 256-byte aligned, zero-initialised ONCE with
 * asd_workspace_init; every call hands it back all-zero, so one workspace serves any number of stream-ordered calls of any
 * B' <= B (two calls that may run concurrently need two).  A hand-off that never arrives (bounded wait) POISONS the row --
 * tok = -1, lp = nucleus_logit = NaN -- it is never guessed.
 * ---------------------------------------------------------------------------------------- */
size_t asd_draft_sample_workspace_bytes(int B, int V, int dtype);
int asd_draft_sample(const void* logits, int64_t ld, int dtype, const float* r /*[B]*/, int B, int V,
                     float inv_temperature, float top_p, int32_t* tok /*[B] out*/, float* lp /*[B] out, may be NULL*/,
                     float* nucleus_logit /*[B] out, may be NULL*/, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Target-side top-p: verify and commit against the TARGET's nucleus.  The reference samples every model -- the target
 * included -- with HF generate(do_sample=True, temperature=0.7, top_p=0.9) (src/training/generate_training_data.py:110-119,
 * src/serving/real_model_pipeline.py:60,326,378, the per-request top_p of src/serving/server.py:45), and HF's assisted
 * generation applies the same warpers to the target's scores before its speculative test.  For a target row x = logits[b,k]:
 *   N      = { v : x_v >= x* },  x* = asd_draft_sample's nucleus_logit of that row for the same T and top_p (the same select
 *            code: bit-identical), HF's TopPLogitsWarper set with every tie at the boundary kept
 *   p^N    = softmax(x / T) restricted to N, renormalised
 *   lp_t[b,k]            = log p^N(tok[b,k])  (-inf when x_tok < x* or tok outside [0,V); bit-identical to asd_draft_sample's
 *                          lp for the token it drew)
 *   accept / n_acc / accept_bits: the rules of asd_verify_accept (log u <= lp_t - lp_d, the leading run)
 *   t_nucleus_logit[b,k] = x* (f32, raw score units; -inf without truncation; may be NULL)
 *   n_finite[b]          = number of leading positions whose lp_t is finite: the n_valid of asd_predictor_stop, so that a
 *                          token outside the nucleus never reaches the statistics as -inf (may be NULL)
 * The features the reference's predictor reads are log-probs of the WARPED scores (generate_training_data.py:128-136).
 * top_p outside (0,1): asd_verify_accept_ex with inv_temperature (the same bits; workspace as for it), x* = -inf.
 * Otherwise: logits 16-byte aligned, a whole number of 16-byte vectors per row, V*sizeof(elem) <= 2 MiB; no workspace (may be
 * NULL); two stream-ordered launches (one 1024-lane workgroup per row, then one wave per sequence), nothing crosses workgroups.
 * ---------------------------------------------------------------------------------------- */
int asd_verify_accept_top_p(const void* logits, int dtype, int64_t ld_row,
                            const int32_t* tok /*[B,K]*/, const float* lp_draft /*[B,K]*/, const float* u /*[B,K]*/,
                            int B, int K, int V, float inv_temperature, float top_p,
                            float* lp_target /*[B,K] out*/, uint8_t* accept /*[B,K] out*/, int32_t* n_acc /*[B] out*/,
                            uint64_t* accept_bits /*[B] out, may be NULL*/, float* t_nucleus_logit /*[B,K] out, may be NULL*/,
                            int32_t* n_finite /*[B] out, may be NULL*/, void* workspace, size_t workspace_bytes, void* stream);

/* The committed token against the target's nucleus (asd_residual_sample_ex with p_t replaced by p^N):
 *   j <  K : w = max(0, p_t^N - p_d^N), N of row (b,j) given by t_threshold[b,j] (asd_verify_accept_top_p's t_nucleus_logit),
 *            p_d^N by d_threshold as in asd_residual_sample_ex; an empty residual falls back to p_t^N
 *   j >= K : w = p^N of bonus_logits[b]; its x* is computed here by asd_draft_sample's select (the same bits as its
 *            nucleus_logit on that row)
 * The draw is the inverse CDF in vocabulary order of asd_residual_sample.  top_p outside (0,1): asd_residual_sample_ex (the
 * same bits; t_threshold is ignored).  workspace: asd_residual_sample_top_p_workspace_bytes(B,V,dtype) bytes (the residual
 * workspace + the bonus rows' thresholds), initialised as for asd_residual_sample. */
size_t asd_residual_sample_top_p_workspace_bytes(int B, int V, int dtype);
int asd_residual_sample_top_p(const void* t_logits, int64_t ld_t, const void* d_logits, int64_t ld_d,
                              const void* bonus_logits, int64_t ld_b, int dtype,
                              const int32_t* n_acc /*[B]*/, const float* r /*[B]*/, int B, int K, int V,
                              float inv_temperature, float top_p, const float* t_threshold /*[B,K]*/,
                              const float* d_threshold /*[B,K] or NULL*/, int32_t* token /*[B] out*/,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Top-k before top-p, on all three sampling steps.  The reference calls HF generate(do_sample=True, temperature=0.7,
 * top_p=0.9) (src/training/generate_training_data.py:110-119) and passes no top_k, so transformers applies its default
 * top_k = 50 (GenerationConfig; a checkpoint's generation_config.json may set another value): the warper chain is
 * TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper, on the draft's scores and, in assisted generation, on the
 * target's.  For a row x (raw logits, T > 0) and 1 <= top_k < V:
 *   x_k   = the top_k-th largest value of the row counting multiplicity; K = { v : x_v >= x_k } (every tie at x_k kept:
 *           TopKLogitsWarper removes scores < topk(scores, k).values[-1]).  Fewer than top_k values > -inf: x_k = -inf.
 *   x*_K  = the nucleus threshold of softmax(x / T) restricted to K and renormalised over K, by the definition of
 *           asd_draft_sample (the largest value whose upper mass reaches top_p, every tie kept); -inf for top_p outside (0,1)
 *   thr   = max(x_k, x*_K);  q = softmax(x / T) restricted to { x >= thr } and renormalised
 * The draw, lp, the accept rule and the residual rule are those of the top-p entry points with this thr, so every
 * threshold output below is thr and asd_residual_sample_ex / _top_p consume it unchanged.  x_k is found by a radix select by
 * COUNT (integer counts: no dependence on the geometry); thr, lp and lp_t come from ONE select body shared by the three
 * entry points (the same bits for the same row).  The sets are defined on raw logits: for bf16 / f16 rows x / T in f32
 * cannot merge two distinct values, so K and thr's set equal HF's; for f32 rows two logits one ulp apart can round to the
 * same x / T in HF's scores while the select still tells them apart (a difference at the boundary only).
 * Off switch: top_k <= 0 or top_k >= V is the corresponding top-p entry point (asd_draft_sample, asd_verify_accept_top_p,
 * asd_residual_sample_top_p) with the same arguments: the same bits, the same status codes.  Otherwise the argument checks
 * and status codes are those of that entry point.  Rows: 16-byte aligned, a whole number of 16-byte vectors,
 * V*sizeof(elem) <= 2 MiB.
 *
 * asd_draft_sample_top_k: tok / lp / threshold as asd_draft_sample's tok / lp / nucleus_logit, with thr.  Geometry: ONE
 *   launch of one 1024-lane workgroup per row at every B (the spread-over-workgroups form of asd_draft_sample does not take
 *   top-k yet); `workspace` is accepted as for asd_draft_sample (asd_draft_sample_workspace_bytes) and left untouched.
 * ---------------------------------------------------------------------------------------- */
int asd_draft_sample_top_k(const void* logits, int64_t ld, int dtype, const float* r /*[B]*/, int B, int V,
                           float inv_temperature, int top_k, float top_p, int32_t* tok /*[B] out*/,
                           float* lp /*[B] out, may be NULL*/, float* threshold /*[B] out, may be NULL*/,
                           void* workspace, size_t workspace_bytes, void* stream);
/* asd_verify_accept_top_k: asd_verify_accept_top_p against thr: lp_t = log q(tok) (-inf when x_tok < thr; bit-identical to
 *   asd_draft_sample_top_k's lp for the token it drew), accept / n_acc / accept_bits / n_finite as there,
 *   t_nucleus_logit = thr.  No workspace (may be NULL); two launches (one workgroup per row, one wave per sequence). */
int asd_verify_accept_top_k(const void* logits, int dtype, int64_t ld_row,
                            const int32_t* tok /*[B,K]*/, const float* lp_draft /*[B,K]*/, const float* u /*[B,K]*/,
                            int B, int K, int V, float inv_temperature, int top_k, float top_p,
                            float* lp_target /*[B,K] out*/, uint8_t* accept /*[B,K] out*/, int32_t* n_acc /*[B] out*/,
                            uint64_t* accept_bits /*[B] out, may be NULL*/, float* t_nucleus_logit /*[B,K] out, may be NULL*/,
                            int32_t* n_finite /*[B] out, may be NULL*/, void* workspace, size_t workspace_bytes, void* stream);
/* asd_residual_sample_top_k: asd_residual_sample_top_p with thr: rows j < K take t_threshold[b,j] (asd_verify_accept_top_k's
 *   t_nucleus_logit), the bonus row's thr is found here by the same select (bit-identical to asd_draft_sample_top_k's threshold
 *   on that row), d_threshold = asd_draft_sample_top_k's threshold.  workspace: asd_residual_sample_top_p_workspace_bytes, the
 *   geometry of asd_residual_sample_top_p. */
int asd_residual_sample_top_k(const void* t_logits, int64_t ld_t, const void* d_logits, int64_t ld_d,
                              const void* bonus_logits, int64_t ld_b, int dtype,
                              const int32_t* n_acc /*[B]*/, const float* r /*[B]*/, int B, int K, int V,
                              float inv_temperature, int top_k, float top_p, const float* t_threshold /*[B,K]*/,
                              const float* d_threshold /*[B,K] or NULL*/, int32_t* token /*[B] out*/,
                              void* workspace, size_t workspace_bytes, void* stream);
/* asd_residual_sample_lp: asd_residual_sample_top_k that also reports the committed token's TARGET log-prob -- the per-token
 *   log-prob the reference's stages hand to the quality predictor (stage.generate(..., return_logprobs=True),
 *   src/serving/pipeline.py:204-231); the verify gives lp_target for the accepted tokens, this call for the one drawn after them.
 *   lp[b] = log p_t^N(token[b]): p_t^N = softmax(x / T) over the target row the draw used (t_logits[b, n_acc[b]], or the bonus
 *   row) restricted to that row's threshold and renormalised -- the distribution the step is lossless against, NOT the residual
 *   weight.  Formed like lp_target: ln 2 * (x_tok * c2 - log2 normaliser).  token[b] == -1 => lp[b] = NaN.  lp must not be NULL.
 *   Arguments that truncate nothing make it asd_residual_sample_ex (t_threshold ignored); the tokens are those of the
 *   corresponding existing entry point, bit for bit.  workspace: asd_residual_sample_top_p_workspace_bytes when truncating. */
int asd_residual_sample_lp(const void* t_logits, int64_t ld_t, const void* d_logits, int64_t ld_d,
                           const void* bonus_logits, int64_t ld_b, int dtype,
                           const int32_t* n_acc /*[B]*/, const float* r /*[B]*/, int B, int K, int V,
                           float inv_temperature, int top_k, float top_p, const float* t_threshold /*[B,K] or NULL*/,
                           const float* d_threshold /*[B,K] or NULL*/, int32_t* token /*[B] out*/, float* lp /*[B] out*/,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Min-p behind top-k and top-p, on all three sampling steps: HF's MinPLogitsWarper (generate(min_p=...)), vLLM's
 * SamplingParams.min_p -- what is set in place of top-p at temperatures of 0.7 and above.  The warper keeps the tokens with
 * p_v >= min_p * p_max, and at least one.  For a row x (raw logits, T > 0, c = inv_temperature) and 0 < min_p <= 1:
 *   thr_kp = the threshold of Temperature -> TopK -> TopP: max(x_k, x*_K), computed exactly as asd_draft_sample_top_k computes
 *            it for the same (top_k, top_p); -inf when both are off
 *   x_max  = the largest value of the row, exactly (a float max over the raw logits, not the streaming pair's scaled
 *            maximum).  x_max lies inside every top-k and every top-p set.
 *   delta  = (float)(log((double)min_p) / (double)inv_temperature) <= 0, formed once on the host by the launcher
 *   x_mp   = x_max + delta, ONE f32 addition on the device.  This is the warper's rule on raw logits, with min-p LAST in
 *            the chain: p_v / p_max = exp((x_v - x_max) c) does not change under the renormalisation of top-k or top-p, so the
 *            kept set is { x_v >= thr_kp } n { x_v >= x_mp }
 *   thr    = max(thr_kp, x_mp);  q = softmax(x / T) restricted to { x >= thr } and renormalised.  Every tie at thr is kept and
 *            the maximum is always kept (HF's min_tokens_to_keep = 1).
 * The draw, lp, the accept rule, n_finite, the residual rule and the -1 / NaN poisoning are those of the top-k entry points
 * with this thr; every threshold output below is thr.  One addition: min-p often keeps a single token, q = 1, and the f32
 * normaliser can leave its log-prob a rounding above 0 -- the min-p entry points report such an lp / lp_target as 0 (the draft
 * and the verify alike: still the same bits).  Where x_mp > thr_kp the normaliser is taken over { x >= x_mp } by one
 * more sweep of the (L2-resident) row: canonical tile pairs folded in the fixed order, inside the ONE select body the three
 * entry points share (the same bits for the same row).  With top-k and top-p both off no select runs at all.  The set is
 * defined on raw logits in f32: against HF, which compares softmax probabilities, it can differ only for tokens whose logit
 * lies within one f32 rounding of x_mp (for 16-bit and f32 rows alike: the boundary is a sum, not a value of the row).
 * Off switch: min_p <= 0 is the corresponding top-k entry point (asd_draft_sample_top_k, asd_verify_accept_top_k,
 * asd_residual_sample_lp) with the same arguments: the same bits, the same status codes.  min_p > 1 or NaN:
 * ASD_ERR_INVALID_ARG, reported before anything else (the empty-batch return included).  Otherwise the argument checks and
 * status codes are those of the top-k entry point with a live bound.  Rows: 16-byte aligned, a whole number of 16-byte
 * vectors, V*sizeof(elem) <= 2 MiB, no NaN / +inf.
 *
 * asd_draft_sample_min_p: tok / lp / threshold as asd_draft_sample_top_k's, with thr.  ONE launch of one 1024-lane workgroup
 *   per row at every B (the spread-over-workgroups form does not take min-p); `workspace` is accepted and left untouched.
 * ---------------------------------------------------------------------------------------- */
int asd_draft_sample_min_p(const void* logits, int64_t ld, int dtype, const float* r /*[B]*/, int B, int V,
                           float inv_temperature, int top_k, float top_p, float min_p, int32_t* tok /*[B] out*/,
                           float* lp /*[B] out, may be NULL*/, float* threshold /*[B] out, may be NULL*/,
                           void* workspace, size_t workspace_bytes, void* stream);
/* asd_verify_accept_min_p: asd_verify_accept_top_k against thr: lp_t = log q(tok) (-inf when x_tok < thr; bit-identical to
 *   asd_draft_sample_min_p's lp for the token it drew), accept / n_acc / accept_bits / n_finite as there,
 *   t_nucleus_logit = thr.  No workspace (may be NULL); two launches (one workgroup per row, one wave per sequence). */
int asd_verify_accept_min_p(const void* logits, int dtype, int64_t ld_row,
                            const int32_t* tok /*[B,K]*/, const float* lp_draft /*[B,K]*/, const float* u /*[B,K]*/,
                            int B, int K, int V, float inv_temperature, int top_k, float top_p, float min_p,
                            float* lp_target /*[B,K] out*/, uint8_t* accept /*[B,K] out*/, int32_t* n_acc /*[B] out*/,
                            uint64_t* accept_bits /*[B] out, may be NULL*/, float* t_nucleus_logit /*[B,K] out, may be NULL*/,
                            int32_t* n_finite /*[B] out, may be NULL*/, void* workspace, size_t workspace_bytes, void* stream);
/* asd_residual_sample_lp_min_p: asd_residual_sample_lp with thr: rows j < K take t_threshold[b,j] (asd_verify_accept_min_p's
 *   t_nucleus_logit), the bonus row's thr is found here by the same select (bit-identical to asd_draft_sample_min_p's
 *   threshold on that row), d_threshold = the draft draw's threshold.  workspace:
 *   asd_residual_sample_top_p_workspace_bytes, the geometry of asd_residual_sample_top_p. */
int asd_residual_sample_lp_min_p(const void* t_logits, int64_t ld_t, const void* d_logits, int64_t ld_d,
                                 const void* bonus_logits, int64_t ld_b, int dtype,
                                 const int32_t* n_acc /*[B]*/, const float* r /*[B]*/, int B, int K, int V,
                                 float inv_temperature, int top_k, float top_p, float min_p,
                                 const float* t_threshold /*[B,K]*/, const float* d_threshold /*[B,K] or NULL*/,
                                 int32_t* token /*[B] out*/, float* lp /*[B] out*/,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-sequence sampling parameters: a batch is a set of independent requests, each with its own temperature, top-k, top-p
 * and min-p (the reference's GenerationRequest carries temperature and top_p per request, src/serving/server.py:44-45,67;
 * vLLM's SamplingParams and HF generate add top_k and min_p).  The scalar entry points above bake c2, levels, top_k and
 * delta into one parameter block per launch; the *_rows entry points below read them per SEQUENCE from a packed table.
 *
 * asd_sampling_rows_pack (host pointers, like asd_mlp_pack_weights) writes B rows of ASD_SAMPLING_ROW_BYTES:
 *   +0  f32 c2        (float)(log2(e) * (double)inv_temperature[b])
 *   +4  f32 top_p     top_p[b] (1 without the array); used by the mass select where levels > 0
 *   +8  i32 levels    0 when top_p[b] is outside (0, 1), else 2 (16-bit logits) or 3 (f32): why the table is per dtype
 *   +12 i32 top_k     top_k[b] where 0 < top_k[b] < V, else 0: why it is per V
 *   +16 f32 delta     (float)(log((double)min_p[b]) / (double)inv_temperature[b]) where min_p[b] > 0, else -inf
 *   +20 u32 clamp     1 where min_p[b] > 0 (the row takes the min-p select and its "lp a rounding above 0 reads as 0" rule)
 *   +24 8 bytes reserved (zero)
 * formed by the very host functions the scalar launchers call: a row holds the bits a scalar launch with its four values
 * would use.  NULL top_k / top_p / min_p = off for every sequence.  Status: B < 0, V < 1, NULL inv_temperature or packed (with
 * B > 0), an inv_temperature that is not finite and > 0, a NaN top_p, a min_p that is NaN or > 1: invalid argument; an unknown
 * dtype: unsupported.  The caller copies the table to the device once (per generate call) and hands that copy to the kernels,
 * which index it by sequence b (the verify by b = row / K); it must stay alive and unchanged until they have run.
 *
 * Semantics: sequence b of a *_rows call is the scalar min-p entry point called with b's four values -- through the off
 * switches (top_k <= 0 or >= V; top_p outside (0, 1); min_p <= 0) the top-k, top-p or plain entry point -- and returns its
 * bits: thresholds, lp / lp_target, n_finite, the commit draw's lp and the tokens (the draft's token: that of the
 * one-workgroup form, which the scalar call takes by itself whenever top-k or min-p is on).  Every kernel takes a
 * workgroup-uniform branch on the sequence's mode into the instantiation of the ONE select body the scalar kernel of that mode
 * runs.  One exception: a sequence that truncates nothing is verified by the same select kernel with levels = 0 -- not by
 * asd_verify_accept_ex's streaming kernel -- so its lp_target is the select's sweep-1 normaliser (the bits asd_draft_sample
 * reports as lp for that token), its t_nucleus_logit is -inf, and it agrees with asd_verify_accept_ex to 1e-5 against f64,
 * not bit for bit.  Mixing is per sequence, never per row of a sequence.
 * Status: a NULL table (with rows to process) is an invalid argument; everything else is checked as by the min-p entry point
 * with a live bound (whole 16-byte vectors, 16-byte aligned rows, V*sizeof(elem) <= 2 MiB at every B).  The table's contents
 * are not checked by the device entry points.
 * ---------------------------------------------------------------------------------------- */
#define ASD_SAMPLING_ROW_BYTES 32
size_t asd_sampling_rows_bytes(int B);     /* B * ASD_SAMPLING_ROW_BYTES; 0 when B <= 0 */
int asd_sampling_rows_pack(const float* inv_temperature /*host [B]*/, const int32_t* top_k /*host [B] or NULL = off*/,
                           const float* top_p /*host [B] or NULL = off*/, const float* min_p /*host [B] or NULL = off*/,
                           int B, int V, int dtype, void* packed /*host out*/);
/* asd_draft_sample_rows: asd_draft_sample_min_p with sequence b's parameters from rows[b].  ONE launch of one 1024-lane
 *   workgroup per row at every B; `workspace` is accepted and left untouched. */
int asd_draft_sample_rows(const void* logits, int64_t ld, int dtype, const float* r /*[B]*/, int B, int V,
                          const void* rows /*device, asd_sampling_rows_pack*/, int32_t* tok /*[B] out*/,
                          float* lp /*[B] out, may be NULL*/, float* threshold /*[B] out, may be NULL*/,
                          void* workspace, size_t workspace_bytes, void* stream);
/* asd_verify_accept_rows: asd_verify_accept_min_p with the parameters of rows[b] for the K rows of sequence b.  The two
 *   launches of the truncated verify at every B, for every row (the untruncated-sequence exception above); no workspace. */
int asd_verify_accept_rows(const void* logits, int dtype, int64_t ld_row,
                           const int32_t* tok /*[B,K]*/, const float* lp_draft /*[B,K]*/, const float* u /*[B,K]*/,
                           int B, int K, int V, const void* rows /*device*/,
                           float* lp_target /*[B,K] out*/, uint8_t* accept /*[B,K] out*/, int32_t* n_acc /*[B] out*/,
                           uint64_t* accept_bits /*[B] out, may be NULL*/, float* t_nucleus_logit /*[B,K] out, may be NULL*/,
                           int32_t* n_finite /*[B] out, may be NULL*/, void* workspace, size_t workspace_bytes, void* stream);
/* asd_residual_sample_lp_rows: asd_residual_sample_lp_min_p with the parameters of rows[b]: t_threshold =
 *   asd_verify_accept_rows' t_nucleus_logit (-inf on an untruncated sequence: the whole row), d_threshold = the draft draws',
 *   the bonus row's threshold found here by the select of rows[b].  workspace: asd_residual_sample_top_p_workspace_bytes,
 *   always; the geometry choice of asd_residual_sample_lp_min_p. */
int asd_residual_sample_lp_rows(const void* t_logits, int64_t ld_t, const void* d_logits, int64_t ld_d,
                                const void* bonus_logits, int64_t ld_b, int dtype,
                                const int32_t* n_acc /*[B]*/, const float* r /*[B]*/, int B, int K, int V,
                                const void* rows /*device*/, const float* t_threshold /*[B,K]*/,
                                const float* d_threshold /*[B,K] or NULL*/, int32_t* token /*[B] out*/, float* lp /*[B] out*/,
                                void* workspace, size_t workspace_bytes, void* stream);

/* N1, second form: asd_verify_accept with the epilogue of asd_predictor_stop run INSIDE the same
 * launch by the wave that completes each sequence (lp = the kernel's own lp_target, all K
 * positions valid).  ONE launch per tier step instead of two, at every batch size: with one workgroup
 * per row (B*K >= CUs) every row hands its lp_t to the sequence's finisher through a self-tagging
 * workspace slot; with split rows (B*K < CUs, e.g. B = 8) the finisher wave already holds all K lp_t.
 * The in-kernel form covers the reference's 64->32->1 predictor (src/minimal_adaptive_decoder.py:38-49) and -- with one
 * workgroup per row -- the 256->128->1 predictor its server instantiates (QualityPredictor(feature_dim=256),
 * src/serving/server.py:168; docs/guides/RESEARCH_PROTOCOL.md:315-364), for hierarchies of <= 4 tiers and draft lengths
 * <= 16; any other predictor shape, depth, draft length or forced geometry is served by the same call as two launches with
 * identical results (bit-identical: tests/test_gpu_predictor.py).  Parameters: those of asd_verify_accept followed by those
 * of asd_predictor_stop (without lp / n_valid / K / B); _ex adds asd_verify_options (inv_temperature:
 * the tiers verify at T = 0.7, pipeline.py:94).  Replaces the per-stage sequence
 * predictor.predict -> bayesian_adjustment -> optimal_stopping_rule of src/serving/pipeline.py:225-261. */
int asd_verify_accept_fused(const void* logits, int dtype, int64_t ld_row,
                            const int32_t* tok, const float* lp_draft, const float* u, int B, int K, int V,
                            float* lp_target, uint8_t* accept, int32_t* n_acc, uint64_t* accept_bits,
                            void* workspace, size_t workspace_bytes,
                            const float* feat, int64_t ldf, int stats_col,
                            const float* packed_w, int in_dim, int hidden,
                            int risk_adjustment, int64_t n_obs, double alpha, double beta,
                            double* p_hist, const double* C, double lam, int L, int stage_idx, int prefix_rule,
                            const double* theta,
                            float* score, int32_t* k_star, uint8_t* stop, uint8_t* thr_stop, double* stats,
                            void* stream);
int asd_verify_accept_fused_ex(const void* logits, int dtype, int64_t ld_row,
                               const int32_t* tok, const float* lp_draft, const float* u, int B, int K, int V,
                               float* lp_target, uint8_t* accept, int32_t* n_acc, uint64_t* accept_bits,
                               void* workspace, size_t workspace_bytes,
                               const float* feat, int64_t ldf, int stats_col,
                               const float* packed_w, int in_dim, int hidden,
                               int risk_adjustment, int64_t n_obs, double alpha, double beta,
                               double* p_hist, const double* C, double lam, int L, int stage_idx, int prefix_rule,
                               const double* theta,
                               float* score, int32_t* k_star, uint8_t* stop, uint8_t* thr_stop, double* stats,
                               const asd_verify_options* opt /*host, may be NULL*/, void* stream);

#ifdef ASD_TEST_HOOKS
/* ------------------------------------------------------------------------------------------
 * TEST HOOKS -- not part of the product library.  They are process-global switches (not thread-safe next to the
 * reference's 100-thread caller, src/serving/pipeline.py:83), so libasd_hip.so does not contain them at all: they exist in
 * the separate TEST build of the same sources (-DASD_TEST_HOOKS -> lib/libasd_hip_test.so, build.py), which the test-suite
 * loads next to the product library for the few tests that need them (kernels.test_hooks()).
 * ---------------------------------------------------------------------------------------- */
/* force the reduction slices of asd_linear* (0 = the launcher's own choice); returns the previous value */
int asd_debug_force_linear_slices(int k_slices);
/* 256 < M <= 288 as one 288-row block (1, default) or as 256 + 32 rows (0); returns the previous value */
int asd_debug_linear_tall(int on);
/* force the workgroups per sequence of the following asd_residual_sample[_ex] calls (1 ... 32; -1 = never the group form;
 * 0 = heuristic) */
int asd_debug_residual_groups(int groups);
/* force the workgroups per row of the following asd_draft_sample calls (1, 2, 4 ... 32; -1 = the one-workgroup streaming
 * form; 0 = heuristic).  Results must not depend on it. */
int asd_debug_draft_groups(int groups);
/* fault injection: in the asd_draft_sample calls that follow, partner workgroup g >= 1 of row b (index = b * G + g, G = the
 * launch's workgroups per row) does not publish its tile pairs.  The leader's bounded wait (~0.5 s) must end in tok = -1 /
 * lp = nucleus_logit = NaN for that row and ASD_WS_LOST_HANDOFF in the workspace's status word.  index < 0 = off. */
int asd_debug_draft_withhold(int index);
/* fault injection: in the verify launches that follow, the workgroup with linear index row * S + split (S = the launch's
 * splits per row) does not publish its hand-off slot.  The kernel's bounded wait must then POISON the affected outputs --
 * lp_target = NaN and accept = 0 for the row (split rows), score = NaN / k_star = L - 1 / stop = 0 for the sequence
 * (in-kernel epilogue) -- and raise ASD_WS_LOST_HANDOFF in the workspace's status word; never return a plausible wrong
 * value.  index < 0 switches the hook off. */
int asd_debug_verify_withhold(int index);
#endif /* ASD_TEST_HOOKS */

#ifdef __cplusplus
}
#endif
#endif /* ASD_HIP_H */
