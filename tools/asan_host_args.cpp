// Stand-alone host harness for `make asan-host-args`: calls the argument checks of the launchers behind asd_residual_sample_lp,
// asd_commit_step_lp, asd_commit_step_stop, asd_commit_step_finish, asd_verify_greedy, asd_top_logprobs, asd_commit_top_logprobs, asd_step_uniforms, asd_logit_edit_rows, asd_logit_mask_rows, asd_penalty_rows, asd_penalty_commit, asd_bad_words_rows, asd_fsm_mask_rows, asd_fsm_advance, asd_fsm_commit, asd_no_repeat_ngram_rows, asd_prompt_logprobs and asd_token_stats in a library whose HOST code is built with AddressSanitizer + UBSan (build.py --asan).  Every call below is
// rejected (or is the B == 0 no-op) before anything is launched, so no GPU is needed and no pointer is dereferenced.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "asd_hip.h"

static int failures = 0;
#define EXPECT(call, want)                                                                 \
    do {                                                                                   \
        const int rc_ = (call);                                                            \
        if (rc_ != (want)) { std::printf("FAIL %s:%d  %s -> %d, want %d\n", __FILE__, __LINE__, #call, rc_, (want)); ++failures; } \
    } while (0)

int main() {
    const int B = 4, K = 8, V = 1024, BF16 = 1;
    alignas(256) static unsigned char rows[16];          // stands for every device buffer: aligned, never read
    void* p = rows;
    int32_t* i32 = reinterpret_cast<int32_t*>(rows);
    float* f32 = reinterpret_cast<float*>(rows);
    const size_t plain = asd_residual_sample_workspace_bytes(B, V, BF16);
    const size_t cut = asd_residual_sample_top_p_workspace_bytes(B, V, BF16);
    if (cut < plain || plain % 256 != 0) { std::printf("FAIL workspace sizes %zu %zu\n", plain, cut); ++failures; }

    // ---- asd_residual_sample_lp
    EXPECT(asd_residual_sample_lp(p, V, p, V, p, V, BF16, i32, f32, B, K, V, 1.0f, 0, 1.0f, nullptr, nullptr, i32, nullptr, p, cut, nullptr), ASD_ERR_INVALID_ARG);   // lp
    EXPECT(asd_residual_sample_lp(p, V, p, V, p, V, BF16, i32, f32, 0, K, V, 1.0f, 0, 1.0f, nullptr, nullptr, i32, nullptr, p, cut, nullptr), ASD_OK);                // B == 0
    EXPECT(asd_residual_sample_lp(p, V, p, V, p, V, BF16, i32, f32, B, K, V, 1.0f, 0, NAN, nullptr, nullptr, i32, f32, p, cut, nullptr), ASD_ERR_INVALID_ARG);        // top_p NaN
    EXPECT(asd_residual_sample_lp(p, V, p, V, p, V, BF16, i32, f32, B, K, V, 1.0f, 0, 0.9f, nullptr, nullptr, i32, f32, p, cut, nullptr), ASD_ERR_INVALID_ARG);       // t_threshold
    EXPECT(asd_residual_sample_lp(p, V, p, V, p, V, BF16, i32, f32, B, K, V, 1.0f, 50, 0.9f, f32, nullptr, i32, f32, p, plain, nullptr), ASD_ERR_WORKSPACE);                      // truncating call, plain workspace
    EXPECT(asd_residual_sample_lp(p, V, p, V, p, V, BF16, i32, f32, -1, K, V, 1.0f, 0, 1.0f, nullptr, nullptr, i32, f32, p, cut, nullptr), ASD_ERR_INVALID_ARG);
    EXPECT(asd_residual_sample_lp(p, V, p, V, p, V, BF16, i32, f32, B, -1, V, 1.0f, 0, 1.0f, nullptr, nullptr, i32, f32, p, cut, nullptr), ASD_ERR_INVALID_ARG);
    EXPECT(asd_residual_sample_lp(p, V, p, V, p, V, BF16, i32, f32, B, K, 0, 1.0f, 0, 1.0f, nullptr, nullptr, i32, f32, p, cut, nullptr), ASD_ERR_INVALID_ARG);
    EXPECT(asd_residual_sample_lp(p, V, p, V, p, V, 99, i32, f32, B, K, V, 1.0f, 0, 1.0f, nullptr, nullptr, i32, f32, p, cut, nullptr), ASD_ERR_UNSUPPORTED);         // dtype
    EXPECT(asd_residual_sample_lp(p, V, p, V, p, V, BF16, nullptr, f32, B, K, V, 1.0f, 0, 1.0f, nullptr, nullptr, i32, f32, p, cut, nullptr), ASD_ERR_INVALID_ARG);   // n_acc
    EXPECT(asd_residual_sample_lp(p, V, p, V, p, V, BF16, i32, nullptr, B, K, V, 1.0f, 0, 1.0f, nullptr, nullptr, i32, f32, p, cut, nullptr), ASD_ERR_INVALID_ARG);   // r
    EXPECT(asd_residual_sample_lp(p, V, p, V, p, V, BF16, i32, f32, B, K, V, 1.0f, 0, 1.0f, nullptr, nullptr, nullptr, f32, p, cut, nullptr), ASD_ERR_INVALID_ARG);   // token
    EXPECT(asd_residual_sample_lp(p, V, p, V, p, V, BF16, i32, f32, B, K, V, 1.0f, 0, 1.0f, nullptr, nullptr, i32, f32, nullptr, cut, nullptr), ASD_ERR_INVALID_ARG); // workspace
    EXPECT(asd_residual_sample_lp(nullptr, V, p, V, p, V, BF16, i32, f32, B, K, V, 1.0f, 0, 1.0f, nullptr, nullptr, i32, f32, p, cut, nullptr), ASD_ERR_INVALID_ARG);
    EXPECT(asd_residual_sample_lp(p, V - 1, p, V, p, V, BF16, i32, f32, B, K, V, 1.0f, 0, 1.0f, nullptr, nullptr, i32, f32, p, cut, nullptr), ASD_ERR_INVALID_ARG);  // ld_t < V
    EXPECT(asd_residual_sample_lp(p, V, p, V, p, V - 1, BF16, i32, f32, B, K, V, 1.0f, 0, 1.0f, nullptr, nullptr, i32, f32, p, cut, nullptr), ASD_ERR_INVALID_ARG);  // ld_b < V
    EXPECT(asd_residual_sample_lp(p, V, p, V, p, V, BF16, i32, f32, B, K, V, -1.0f, 0, 1.0f, nullptr, nullptr, i32, f32, p, cut, nullptr), ASD_ERR_INVALID_ARG);     // temperature
    EXPECT(asd_residual_sample_lp(p, 1001, p, 1001, p, 1001, BF16, i32, f32, B, K, 1001, 1.0f, 0, 1.0f, nullptr, nullptr, i32, f32, p, cut, nullptr), ASD_ERR_ALIGNMENT);   // not whole vectors
    EXPECT(asd_residual_sample_lp(rows + 2, V, p, V, p, V, BF16, i32, f32, B, K, V, 1.0f, 0, 1.0f, nullptr, nullptr, i32, f32, p, cut, nullptr), ASD_ERR_ALIGNMENT);  // misaligned rows
    EXPECT(asd_residual_sample_lp(p, V, p, V, p, V, BF16, i32, f32, B, K, V, 1.0f, 0, 1.0f, nullptr, nullptr, i32, f32, rows + 16, cut, nullptr), ASD_ERR_WORKSPACE); // misaligned workspace
    EXPECT(asd_residual_sample_lp(p, V, p, V, p, V, BF16, i32, f32, B, K, V, 1.0f, 0, 1.0f, nullptr, nullptr, i32, f32, p, plain - 1, nullptr), ASD_ERR_WORKSPACE);   // too small

    // ---- asd_commit_step_lp (the checks of asd_commit_step, plus the three new pointers)
    const int64_t ld = 64;
    EXPECT(asd_commit_step_lp(i32, f32, i32, i32, f32, -1, K, i32, i32, f32, ld, i32, 32, nullptr), ASD_ERR_INVALID_ARG);
    EXPECT(asd_commit_step_lp(i32, f32, i32, i32, f32, B, -1, i32, i32, f32, ld, i32, 32, nullptr), ASD_ERR_INVALID_ARG);
    EXPECT(asd_commit_step_lp(i32, f32, i32, i32, f32, B, K, i32, i32, f32, ld, i32, -1, nullptr), ASD_ERR_INVALID_ARG);
    EXPECT(asd_commit_step_lp(nullptr, nullptr, nullptr, nullptr, nullptr, 0, K, nullptr, nullptr, nullptr, ld, nullptr, 32, nullptr), ASD_OK);
    EXPECT(asd_commit_step_lp(i32, f32, i32, i32, f32, B, ASD_MAX_DRAFT_LEN + 1, i32, i32, f32, ld, i32, 32, nullptr), ASD_ERR_UNSUPPORTED);
    EXPECT(asd_commit_step_lp(nullptr, f32, i32, i32, f32, B, K, i32, i32, f32, ld, i32, 32, nullptr), ASD_ERR_INVALID_ARG);
    EXPECT(asd_commit_step_lp(i32, nullptr, i32, i32, f32, B, K, i32, i32, f32, ld, i32, 32, nullptr), ASD_ERR_INVALID_ARG);
    EXPECT(asd_commit_step_lp(i32, f32, nullptr, i32, f32, B, K, i32, i32, f32, ld, i32, 32, nullptr), ASD_ERR_INVALID_ARG);
    EXPECT(asd_commit_step_lp(i32, f32, i32, nullptr, f32, B, K, i32, i32, f32, ld, i32, 32, nullptr), ASD_ERR_INVALID_ARG);
    EXPECT(asd_commit_step_lp(i32, f32, i32, i32, nullptr, B, K, i32, i32, f32, ld, i32, 32, nullptr), ASD_ERR_INVALID_ARG);
    EXPECT(asd_commit_step_lp(i32, f32, i32, i32, f32, B, K, nullptr, i32, f32, ld, i32, 32, nullptr), ASD_ERR_INVALID_ARG);
    EXPECT(asd_commit_step_lp(i32, f32, i32, i32, f32, B, K, i32, nullptr, f32, ld, i32, 32, nullptr), ASD_ERR_INVALID_ARG);
    EXPECT(asd_commit_step_lp(i32, f32, i32, i32, f32, B, K, i32, i32, nullptr, ld, i32, 32, nullptr), ASD_ERR_INVALID_ARG);
    EXPECT(asd_commit_step_lp(i32, f32, i32, i32, f32, B, K, i32, i32, f32, 31, i32, 32, nullptr), ASD_ERR_INVALID_ARG);       // ld_out < max_len
    // ---- asd_commit_step_stop (the checks of asd_commit_step_lp, plus the stop set and the finished flag)
#define STOP(tok_, lp_tok_, n_acc_, drawn_, lp_drawn_, B_, K_, stops_, n_stop_, seq_, out_, out_lp_, ld_, fin_, max_len_) \
    asd_commit_step_stop(tok_, lp_tok_, n_acc_, drawn_, lp_drawn_, B_, K_, stops_, n_stop_, seq_, out_, out_lp_, ld_, i32, fin_, i32, max_len_, nullptr)
    EXPECT(STOP(i32, f32, i32, i32, f32, -1, K, i32, 2, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(STOP(i32, f32, i32, i32, f32, B, -1, i32, 2, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(STOP(i32, f32, i32, i32, f32, B, K, i32, 2, i32, i32, f32, ld, i32, -1), ASD_ERR_INVALID_ARG);
    EXPECT(STOP(nullptr, nullptr, nullptr, nullptr, nullptr, 0, K, nullptr, 0, nullptr, nullptr, nullptr, ld, nullptr, 32), ASD_OK);
    EXPECT(STOP(i32, f32, i32, i32, f32, B, ASD_MAX_DRAFT_LEN + 1, i32, 2, i32, i32, f32, ld, i32, 32), ASD_ERR_UNSUPPORTED);
    EXPECT(STOP(nullptr, f32, i32, i32, f32, B, K, i32, 2, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(STOP(i32, nullptr, i32, i32, f32, B, K, i32, 2, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(STOP(i32, f32, nullptr, i32, f32, B, K, i32, 2, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(STOP(i32, f32, i32, nullptr, f32, B, K, i32, 2, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(STOP(i32, f32, i32, i32, nullptr, B, K, i32, 2, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(STOP(i32, f32, i32, i32, f32, B, K, i32, 2, nullptr, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(STOP(i32, f32, i32, i32, f32, B, K, i32, 2, i32, nullptr, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(STOP(i32, f32, i32, i32, f32, B, K, i32, 2, i32, i32, nullptr, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(STOP(i32, f32, i32, i32, f32, B, K, i32, 2, i32, i32, f32, 31, i32, 32), ASD_ERR_INVALID_ARG);                  // ld_out < max_len
    EXPECT(STOP(i32, f32, i32, i32, f32, B, K, i32, 2, i32, i32, f32, ld, nullptr, 32), ASD_ERR_INVALID_ARG);              // finished
    EXPECT(STOP(i32, f32, i32, i32, f32, B, K, i32, -1, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);                 // n_stop < 0
    EXPECT(STOP(i32, f32, i32, i32, f32, B, K, nullptr, 1, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);              // ids missing
    EXPECT(STOP(i32, f32, i32, i32, f32, B, K, i32, ASD_MAX_STOP_IDS + 1, i32, i32, f32, ld, i32, 32), ASD_ERR_UNSUPPORTED);
    EXPECT(STOP(i32, f32, i32, i32, f32, -1, K, nullptr, 0, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);             // no stop set: B is still checked
#undef STOP
    // ---- asd_commit_step_finish (the checks of asd_commit_step_stop, plus the sequence tables, the row lists and `start`)
#define FINISH(tok_, lp_tok_, n_acc_, drawn_, lp_drawn_, B_, K_, seq_tok_, seq_n_, n_seq_, first_, start_, seq_, out_, out_lp_, ld_, fin_, max_len_) \
    asd_commit_step_finish(tok_, lp_tok_, n_acc_, drawn_, lp_drawn_, B_, K_, seq_tok_, seq_n_, n_seq_, first_, i32, start_, seq_, out_, out_lp_, ld_, i32, fin_, i32, i32, max_len_, nullptr)
    EXPECT(FINISH(i32, f32, i32, i32, f32, -1, K, i32, i32, 2, i32, 4, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(FINISH(i32, f32, i32, i32, f32, B, -1, i32, i32, 2, i32, 4, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(FINISH(i32, f32, i32, i32, f32, B, K, i32, i32, 2, i32, 4, i32, i32, f32, ld, i32, -1), ASD_ERR_INVALID_ARG);
    EXPECT(FINISH(i32, f32, i32, i32, f32, B, K, i32, i32, -1, i32, 4, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);               // n_seq < 0
    EXPECT(FINISH(i32, f32, i32, i32, f32, B, K, i32, i32, 2, i32, -1, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);               // start < 0
    EXPECT(FINISH(i32, f32, i32, i32, f32, 0, K, i32, i32, 2, i32, -1, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);               // ... before the empty batch
    EXPECT(FINISH(nullptr, nullptr, nullptr, nullptr, nullptr, 0, K, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, ld, nullptr, 32), ASD_OK);
    EXPECT(FINISH(i32, f32, i32, i32, f32, B, ASD_MAX_DRAFT_LEN + 1, i32, i32, 2, i32, 4, i32, i32, f32, ld, i32, 32), ASD_ERR_UNSUPPORTED);
    EXPECT(FINISH(i32, f32, i32, i32, f32, B, K, i32, i32, ASD_MAX_STOP_SEQS + 1, nullptr, 4, i32, i32, f32, ld, i32, 32), ASD_ERR_UNSUPPORTED);   // no row lists: all of them are every row's
    EXPECT(FINISH(i32, f32, i32, i32, f32, B, K, i32, i32, ASD_MAX_STOP_SEQS + 1, i32, 4, i32, i32, f32, ld, nullptr, 32), ASD_ERR_INVALID_ARG);   // with row lists the total is free: on to the pointers
    EXPECT(FINISH(nullptr, f32, i32, i32, f32, B, K, i32, i32, 2, i32, 4, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(FINISH(i32, nullptr, i32, i32, f32, B, K, i32, i32, 2, i32, 4, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(FINISH(i32, f32, nullptr, i32, f32, B, K, i32, i32, 2, i32, 4, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(FINISH(i32, f32, i32, nullptr, f32, B, K, i32, i32, 2, i32, 4, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(FINISH(i32, f32, i32, i32, nullptr, B, K, i32, i32, 2, i32, 4, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(FINISH(i32, f32, i32, i32, f32, B, K, nullptr, i32, 2, i32, 4, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);            // seq_tok missing
    EXPECT(FINISH(i32, f32, i32, i32, f32, B, K, i32, nullptr, 2, i32, 4, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);            // seq_n missing
    EXPECT(FINISH(i32, f32, i32, i32, f32, B, K, i32, i32, 2, i32, 4, nullptr, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(FINISH(i32, f32, i32, i32, f32, B, K, i32, i32, 2, i32, 4, i32, nullptr, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(FINISH(i32, f32, i32, i32, f32, B, K, i32, i32, 2, i32, 4, i32, i32, nullptr, ld, i32, 32), ASD_ERR_INVALID_ARG);
    EXPECT(FINISH(i32, f32, i32, i32, f32, B, K, i32, i32, 2, i32, 4, i32, i32, f32, 31, i32, 32), ASD_ERR_INVALID_ARG);                // ld_out < max_len
    EXPECT(FINISH(i32, f32, i32, i32, f32, B, K, i32, i32, 2, i32, 4, i32, i32, f32, ld, nullptr, 32), ASD_ERR_INVALID_ARG);            // finished
    EXPECT(FINISH(i32, f32, i32, i32, f32, -1, K, nullptr, nullptr, 0, nullptr, 0, i32, i32, f32, ld, i32, 32), ASD_ERR_INVALID_ARG);   // no sequences: B is still checked
#undef FINISH
    // the same rejections from the entry point it extends
    EXPECT(asd_commit_step(i32, i32, i32, B, ASD_MAX_DRAFT_LEN + 1, i32, i32, ld, i32, 32, nullptr), ASD_ERR_UNSUPPORTED);
    EXPECT(asd_commit_step(i32, i32, i32, B, K, i32, i32, 31, i32, 32, nullptr), ASD_ERR_INVALID_ARG);

    // ---- asd_verify_greedy: NULL outputs and the temperature first (both ahead of the empty-batch return), then sizes, the empty batch,
    // K / dtype / splits, pointers, strides, alignment, the workspace
    {
        const int KG = 4, VG = 1000;
        const int64_t ldr = VG, lds = static_cast<int64_t>(KG + 1) * VG;
        uint8_t* u8 = rows;
        const size_t ws = asd_verify_greedy_workspace_bytes(B, KG, VG, BF16);
        if (ws % 256 != 0 || ws < asd_verify_greedy_workspace_bytes(B, 0, VG, BF16) || asd_verify_greedy_workspace_bytes(0, KG, VG, BF16) != 256) {
            std::printf("FAIL greedy workspace size %zu\n", ws);
            ++failures;
        }
#define GREEDY(logits_, dtype_, lds_, ldr_, tok_, B_, K_, V_, inv_t_, splits_, n_acc_, drawn_, lp_drawn_, ws_, ws_bytes_) \
    asd_verify_greedy(logits_, dtype_, lds_, ldr_, tok_, B_, K_, V_, inv_t_, splits_, i32, f32, f32, u8, n_acc_, drawn_, lp_drawn_, ws_, ws_bytes_, nullptr)
        EXPECT(GREEDY(p, BF16, lds, ldr, i32, B, KG, VG, 1.0f, 0, nullptr, i32, f32, p, ws), ASD_ERR_INVALID_ARG);           // n_acc
        EXPECT(GREEDY(p, BF16, lds, ldr, i32, B, KG, VG, 1.0f, 0, i32, nullptr, f32, p, ws), ASD_ERR_INVALID_ARG);           // drawn
        EXPECT(GREEDY(p, BF16, lds, ldr, i32, B, KG, VG, 1.0f, 0, i32, i32, nullptr, p, ws), ASD_ERR_INVALID_ARG);           // lp_drawn
        EXPECT(GREEDY(nullptr, BF16, lds, ldr, i32, B, KG, VG, 1.0f, 0, i32, i32, f32, p, ws), ASD_ERR_INVALID_ARG);         // logits
        EXPECT(GREEDY(p, BF16, lds, ldr, i32, B, KG, VG, 1.0f, 0, i32, i32, f32, nullptr, ws), ASD_ERR_INVALID_ARG);         // workspace
        EXPECT(GREEDY(p, BF16, lds, ldr, i32, B, KG, VG, 0.0f, 0, i32, i32, f32, p, ws), ASD_ERR_INVALID_ARG);               // temperature
        EXPECT(GREEDY(p, BF16, lds, ldr, i32, B, KG, VG, -1.0f, 0, i32, i32, f32, p, ws), ASD_ERR_INVALID_ARG);
        EXPECT(GREEDY(p, BF16, lds, ldr, i32, B, KG, VG, NAN, 0, i32, i32, f32, p, ws), ASD_ERR_INVALID_ARG);
        EXPECT(GREEDY(p, BF16, lds, ldr, i32, B, KG, VG, INFINITY, 0, i32, i32, f32, p, ws), ASD_ERR_INVALID_ARG);
        EXPECT(GREEDY(p, BF16, lds, ldr, i32, 0, KG, VG, 0.0f, 0, i32, i32, f32, p, ws), ASD_ERR_INVALID_ARG);               // ... before the empty batch
        EXPECT(GREEDY(p, BF16, lds, ldr, i32, -1, KG, VG, 1.0f, 0, i32, i32, f32, p, ws), ASD_ERR_INVALID_ARG);
        EXPECT(GREEDY(p, BF16, lds, ldr, i32, B, -1, VG, 1.0f, 0, i32, i32, f32, p, ws), ASD_ERR_INVALID_ARG);
        EXPECT(GREEDY(p, BF16, 0, 0, i32, B, KG, 0, 1.0f, 0, i32, i32, f32, p, ws), ASD_ERR_INVALID_ARG);                    // V == 0
        EXPECT(GREEDY(p, BF16, lds, ldr, nullptr, B, KG, VG, 1.0f, 0, i32, i32, f32, p, ws), ASD_ERR_INVALID_ARG);           // tok == NULL, K > 0
        EXPECT(GREEDY(p, BF16, ldr, ldr, nullptr, B, 0, VG, 1.0f, 0, i32, i32, f32, p, 0), ASD_ERR_WORKSPACE);               // K == 0 needs no tok
        EXPECT(GREEDY(p, BF16, lds, ldr - 1, i32, B, KG, VG, 1.0f, 0, i32, i32, f32, p, ws), ASD_ERR_INVALID_ARG);           // ld_row < V
        EXPECT(GREEDY(p, BF16, lds - 1, ldr, i32, B, KG, VG, 1.0f, 0, i32, i32, f32, p, ws), ASD_ERR_INVALID_ARG);           // ld_seq < (K+1) ld_row
        EXPECT(GREEDY(p, BF16, 66 * ldr, ldr, i32, B, ASD_MAX_DRAFT_LEN + 1, VG, 1.0f, 0, i32, i32, f32, p, ws), ASD_ERR_UNSUPPORTED);
        EXPECT(GREEDY(p, 99, lds, ldr, i32, B, KG, VG, 1.0f, 0, i32, i32, f32, p, ws), ASD_ERR_UNSUPPORTED);                 // dtype
        EXPECT(GREEDY(p, BF16, lds, ldr, i32, B, KG, VG, 1.0f, -1, i32, i32, f32, p, ws), ASD_ERR_UNSUPPORTED);              // splits
        EXPECT(GREEDY(p, BF16, lds, ldr, i32, B, KG, VG, 1.0f, ASD_MAX_SPLITS + 1, i32, i32, f32, p, ws), ASD_ERR_UNSUPPORTED);
        EXPECT(GREEDY(rows + 1, BF16, lds, ldr, i32, B, KG, VG, 1.0f, 0, i32, i32, f32, p, ws), ASD_ERR_ALIGNMENT);          // below the element size
        EXPECT(GREEDY(p, BF16, lds, ldr, i32, B, KG, VG, 1.0f, 0, i32, i32, f32, rows + 16, ws), ASD_ERR_WORKSPACE);         // misaligned workspace
        EXPECT(GREEDY(p, BF16, lds, ldr, i32, B, KG, VG, 1.0f, ASD_MAX_SPLITS, i32, i32, f32, p, ws - 1), ASD_ERR_WORKSPACE); // too small
        EXPECT(GREEDY(rows + 2, BF16, lds, ldr, i32, B, KG, VG, 1.0f, 1, i32, i32, f32, p, 0), ASD_ERR_WORKSPACE);           // (an element-aligned base is valid)
        EXPECT(GREEDY(nullptr, 99, 0, 0, nullptr, 0, KG, VG, 1.0f, 0, nullptr, nullptr, nullptr, nullptr, 0), ASD_OK);       // B == 0: nothing launched
#undef GREEDY
    }

    // ---- asd_top_logprobs: asd_verify_greedy's order (NULL outputs and the temperature ahead of the empty-batch return, sizes, the
    // empty batch, N / K1 / dtype / splits, pointers, strides, alignment, the workspace), then asd_commit_top_logprobs
    {
        const int K1 = 5, VT = 1000, NT = 5;
        const int64_t ldr = VT, lds = static_cast<int64_t>(K1) * VT;
        const size_t ws = asd_top_logprobs_workspace_bytes(B, K1, NT);
        if (ws % 256 != 0 || ws <= asd_top_logprobs_workspace_bytes(B, 1, NT) || asd_top_logprobs_workspace_bytes(0, K1, NT) != 256 ||
            asd_top_logprobs_workspace_bytes(B, 0, NT) != 256) {
            std::printf("FAIL top_logprobs workspace size %zu\n", ws);
            ++failures;
        }
#define TOP(logits_, dtype_, lds_, ldr_, B_, K1_, V_, inv_t_, N_, splits_, id_, lp_, ws_, ws_bytes_) \
    asd_top_logprobs(logits_, dtype_, lds_, ldr_, B_, K1_, V_, inv_t_, N_, splits_, id_, lp_, ws_, ws_bytes_, nullptr)
        EXPECT(TOP(p, BF16, lds, ldr, B, K1, VT, 1.0f, NT, 0, nullptr, f32, p, ws), ASD_ERR_INVALID_ARG);                   // top_id
        EXPECT(TOP(p, BF16, lds, ldr, B, K1, VT, 1.0f, NT, 0, i32, nullptr, p, ws), ASD_ERR_INVALID_ARG);                   // top_lp
        EXPECT(TOP(p, BF16, lds, ldr, B, K1, VT, 0.0f, NT, 0, i32, f32, p, ws), ASD_ERR_INVALID_ARG);                       // temperature
        EXPECT(TOP(p, BF16, lds, ldr, B, K1, VT, NAN, NT, 0, i32, f32, p, ws), ASD_ERR_INVALID_ARG);
        EXPECT(TOP(p, BF16, lds, ldr, B, K1, VT, INFINITY, NT, 0, i32, f32, p, ws), ASD_ERR_INVALID_ARG);
        EXPECT(TOP(p, BF16, lds, ldr, 0, K1, VT, -1.0f, NT, 0, i32, f32, p, ws), ASD_ERR_INVALID_ARG);                      // ... before the empty batch
        EXPECT(TOP(p, BF16, lds, ldr, -1, K1, VT, 1.0f, NT, 0, i32, f32, p, ws), ASD_ERR_INVALID_ARG);
        EXPECT(TOP(p, BF16, lds, ldr, B, -1, VT, 1.0f, NT, 0, i32, f32, p, ws), ASD_ERR_INVALID_ARG);
        EXPECT(TOP(p, BF16, lds, ldr, B, K1, -1, 1.0f, NT, 0, i32, f32, p, ws), ASD_ERR_INVALID_ARG);
        EXPECT(TOP(p, BF16, lds, ldr, B, K1, VT, 1.0f, -1, 0, i32, f32, p, ws), ASD_ERR_INVALID_ARG);
        EXPECT(TOP(nullptr, 99, 0, 0, 0, 99, VT, 1.0f, 99, 99, nullptr, nullptr, nullptr, 0), ASD_OK);                      // B == 0: nothing launched
        EXPECT(TOP(p, BF16, 0, 0, B, K1, 0, 1.0f, NT, 0, i32, f32, p, ws), ASD_ERR_INVALID_ARG);                            // V == 0
        EXPECT(TOP(p, BF16, 0, ldr, B, 0, VT, 1.0f, NT, 0, i32, f32, p, ws), ASD_ERR_INVALID_ARG);                          // K1 < 1
        EXPECT(TOP(p, BF16, lds, ldr, B, K1, VT, 1.0f, 0, 0, i32, f32, p, ws), ASD_ERR_INVALID_ARG);                        // N < 1
        EXPECT(TOP(p, BF16, lds, ldr, B, K1, VT, 1.0f, ASD_MAX_TOP_LOGPROBS + 1, 0, i32, f32, p, ws), ASD_ERR_UNSUPPORTED);
        EXPECT(TOP(p, BF16, 66 * ldr, ldr, B, ASD_MAX_DRAFT_LEN + 2, VT, 1.0f, NT, 0, i32, f32, p, ws), ASD_ERR_UNSUPPORTED);
        EXPECT(TOP(p, 99, lds, ldr, B, K1, VT, 1.0f, NT, 0, i32, f32, p, ws), ASD_ERR_UNSUPPORTED);                         // dtype
        EXPECT(TOP(p, BF16, lds, ldr, B, K1, VT, 1.0f, NT, -1, i32, f32, p, ws), ASD_ERR_UNSUPPORTED);                      // splits
        EXPECT(TOP(p, BF16, lds, ldr, B, K1, VT, 1.0f, NT, ASD_MAX_SPLITS + 1, i32, f32, p, ws), ASD_ERR_UNSUPPORTED);
        EXPECT(TOP(nullptr, BF16, lds, ldr, B, K1, VT, 1.0f, NT, 0, i32, f32, p, ws), ASD_ERR_INVALID_ARG);                 // logits
        EXPECT(TOP(p, BF16, lds, ldr, B, K1, VT, 1.0f, NT, 0, i32, f32, nullptr, ws), ASD_ERR_INVALID_ARG);                 // workspace
        EXPECT(TOP(p, BF16, lds, ldr - 1, B, K1, VT, 1.0f, NT, 0, i32, f32, p, ws), ASD_ERR_INVALID_ARG);                   // ld_row < V
        EXPECT(TOP(p, BF16, lds - 1, ldr, B, K1, VT, 1.0f, NT, 0, i32, f32, p, ws), ASD_ERR_INVALID_ARG);                   // ld_seq < K1 ld_row
        EXPECT(TOP(p, BF16, int64_t{5} << 30, int64_t{1} << 30, B, K1, 1 << 30, 1.0f, NT, 0, i32, f32, p, ws), ASD_ERR_UNSUPPORTED);   // a 2 GiB row
        EXPECT(TOP(rows + 1, BF16, lds, ldr, B, K1, VT, 1.0f, NT, 0, i32, f32, p, ws), ASD_ERR_ALIGNMENT);                  // below the element size
        EXPECT(TOP(p, BF16, lds, ldr, B, K1, VT, 1.0f, NT, 0, i32, f32, rows + 16, ws), ASD_ERR_WORKSPACE);                 // misaligned workspace
        EXPECT(TOP(p, BF16, lds, ldr, B, K1, VT, 1.0f, NT, ASD_MAX_SPLITS, i32, f32, p, ws - 1), ASD_ERR_WORKSPACE);        // too small
        EXPECT(TOP(rows + 2, BF16, lds, ldr, B, K1, VT, 1.0f, NT, 1, i32, f32, p, 0), ASD_ERR_WORKSPACE);                   // (an element-aligned base is valid)
#undef TOP
#define CTOP(id_, lp_, seq_, nc_, B_, K1_, N_, oid_, olp_, max_len_) asd_commit_top_logprobs(id_, lp_, seq_, nc_, B_, K1_, N_, oid_, olp_, max_len_, nullptr)
        EXPECT(CTOP(i32, f32, i32, i32, -1, K1, NT, i32, f32, 32), ASD_ERR_INVALID_ARG);
        EXPECT(CTOP(i32, f32, i32, i32, B, -1, NT, i32, f32, 32), ASD_ERR_INVALID_ARG);
        EXPECT(CTOP(i32, f32, i32, i32, B, K1, -1, i32, f32, 32), ASD_ERR_INVALID_ARG);
        EXPECT(CTOP(i32, f32, i32, i32, B, K1, NT, i32, f32, -1), ASD_ERR_INVALID_ARG);
        EXPECT(CTOP(nullptr, nullptr, nullptr, nullptr, 0, 99, 99, nullptr, nullptr, 32), ASD_OK);                          // B == 0
        EXPECT(CTOP(i32, f32, i32, i32, B, ASD_MAX_DRAFT_LEN + 2, NT, i32, f32, 32), ASD_ERR_UNSUPPORTED);
        EXPECT(CTOP(i32, f32, i32, i32, B, K1, ASD_MAX_TOP_LOGPROBS + 1, i32, f32, 32), ASD_ERR_UNSUPPORTED);
        EXPECT(CTOP(i32, f32, i32, i32, B, 0, NT, i32, f32, 32), ASD_ERR_INVALID_ARG);
        EXPECT(CTOP(i32, f32, i32, i32, B, K1, 0, i32, f32, 32), ASD_ERR_INVALID_ARG);
        EXPECT(CTOP(nullptr, f32, i32, i32, B, K1, NT, i32, f32, 32), ASD_ERR_INVALID_ARG);
        EXPECT(CTOP(i32, nullptr, i32, i32, B, K1, NT, i32, f32, 32), ASD_ERR_INVALID_ARG);
        EXPECT(CTOP(i32, f32, nullptr, i32, B, K1, NT, i32, f32, 32), ASD_ERR_INVALID_ARG);
        EXPECT(CTOP(i32, f32, i32, nullptr, B, K1, NT, i32, f32, 32), ASD_ERR_INVALID_ARG);
        EXPECT(CTOP(i32, f32, i32, i32, B, K1, NT, nullptr, f32, 32), ASD_ERR_INVALID_ARG);
        EXPECT(CTOP(i32, f32, i32, i32, B, K1, NT, i32, nullptr, 32), ASD_ERR_INVALID_ARG);
#undef CTOP
    }

    // ---- asd_step_uniforms: every rejection is ASD_ERR_INVALID_ARG and comes before the launch
    {
        const int64_t* seeds = reinterpret_cast<const int64_t*>(rows);
#define UNI(seeds_, B_, Kd_, Ka_, rd_, u_, rc_) asd_step_uniforms(seeds_, 0u, 0u, B_, Kd_, Ka_, rd_, u_, rc_, nullptr)
        EXPECT(UNI(seeds, 0, 2, 2, f32, f32, f32), ASD_ERR_INVALID_ARG);                                    // B < 1
        EXPECT(UNI(seeds, -1, 2, 2, f32, f32, f32), ASD_ERR_INVALID_ARG);
        EXPECT(UNI(seeds, B, -1, 2, f32, f32, f32), ASD_ERR_INVALID_ARG);
        EXPECT(UNI(seeds, B, 2, -1, f32, f32, f32), ASD_ERR_INVALID_ARG);
        EXPECT(UNI(seeds, B, ASD_MAX_DRAFT_LEN + 1, 2, f32, f32, f32), ASD_ERR_INVALID_ARG);
        EXPECT(UNI(seeds, B, 2, ASD_MAX_DRAFT_LEN + 1, f32, f32, f32), ASD_ERR_INVALID_ARG);
        EXPECT(UNI(nullptr, B, 2, 2, f32, f32, f32), ASD_ERR_INVALID_ARG);                                  // seeds
        EXPECT(UNI(seeds, B, 2, 2, nullptr, nullptr, nullptr), ASD_ERR_INVALID_ARG);                        // no output at all
        EXPECT(UNI(seeds, B, 0, 0, nullptr, nullptr, nullptr), ASD_ERR_INVALID_ARG);
        EXPECT(UNI(seeds, B, 0, 2, f32, f32, f32), ASD_ERR_INVALID_ARG);                                    // r_draft without a slot
        EXPECT(UNI(seeds, B, 2, 0, f32, f32, f32), ASD_ERR_INVALID_ARG);                                    // u without a slot
        EXPECT(UNI(seeds, INT32_MAX, ASD_MAX_DRAFT_LEN, ASD_MAX_DRAFT_LEN, nullptr, nullptr, nullptr), ASD_ERR_INVALID_ARG);   // (the largest grid the launcher would size)
        EXPECT(UNI(reinterpret_cast<const int64_t*>(rows + 4), B, 2, 2, f32, f32, f32), ASD_ERR_ALIGNMENT);
        EXPECT(UNI(seeds, B, 2, 2, reinterpret_cast<float*>(rows + 2), f32, f32), ASD_ERR_ALIGNMENT);
#undef UNI
    }

    // ---- asd_logit_edit_rows: every rejection, and every "nothing to do", comes before the launch
    {
#define EDIT(x_, dt_, lds_, ldr_, B_, K1_, V_, id_, bias_, until_, first_, n_, seq_) \
    asd_logit_edit_rows(x_, dt_, lds_, ldr_, B_, K1_, V_, id_, bias_, until_, first_, n_, seq_, 5, 0, nullptr)
        const int K1 = 5;
        EXPECT(EDIT(p, BF16, K1 * V, V, -1, K1, V, i32, f32, i32, nullptr, 4, i32), ASD_ERR_INVALID_ARG);
        EXPECT(EDIT(p, BF16, K1 * V, V, B, -1, V, i32, f32, i32, nullptr, 4, i32), ASD_ERR_INVALID_ARG);
        EXPECT(EDIT(p, BF16, K1 * V, V, B, K1, -1, i32, f32, i32, nullptr, 4, i32), ASD_ERR_INVALID_ARG);
        EXPECT(EDIT(p, BF16, K1 * V, V, B, K1, V, i32, f32, i32, nullptr, -1, i32), ASD_ERR_INVALID_ARG);
        EXPECT(EDIT(nullptr, 99, 0, 0, 0, K1, V, nullptr, nullptr, nullptr, nullptr, 4, nullptr), ASD_OK);          // B == 0
        EXPECT(EDIT(nullptr, 99, 0, 0, B, 0, V, nullptr, nullptr, nullptr, nullptr, 4, nullptr), ASD_OK);           // K1 == 0
        EXPECT(EDIT(nullptr, 99, 0, 0, B, K1, V, nullptr, nullptr, nullptr, nullptr, 0, nullptr), ASD_OK);          // no entries
        EXPECT(EDIT(p, 99, K1 * V, V, B, K1, V, i32, f32, i32, nullptr, 4, i32), ASD_ERR_UNSUPPORTED);              // dtype
        EXPECT(EDIT(p, BF16, K1 * V, V, B, K1, V, i32, f32, i32, nullptr, ASD_MAX_LOGIT_EDITS + 1, i32), ASD_ERR_UNSUPPORTED);
        EXPECT(EDIT(p, BF16, int64_t{1} << 40, V, INT32_MAX, K1, V, i32, f32, i32, nullptr, 4, i32), ASD_ERR_UNSUPPORTED);   // grid
        EXPECT(EDIT(nullptr, BF16, K1 * V, V, B, K1, V, i32, f32, i32, nullptr, 4, i32), ASD_ERR_INVALID_ARG);
        EXPECT(EDIT(p, BF16, K1 * V, V, B, K1, V, nullptr, f32, i32, nullptr, 4, i32), ASD_ERR_INVALID_ARG);
        EXPECT(EDIT(p, BF16, K1 * V, V, B, K1, V, i32, nullptr, i32, nullptr, 4, i32), ASD_ERR_INVALID_ARG);
        EXPECT(EDIT(p, BF16, K1 * V, V, B, K1, V, i32, f32, nullptr, nullptr, 4, i32), ASD_ERR_INVALID_ARG);
        EXPECT(EDIT(p, BF16, K1 * V, V, B, K1, V, i32, f32, i32, nullptr, 4, nullptr), ASD_ERR_INVALID_ARG);        // seq_len
        EXPECT(EDIT(p, BF16, K1 * V, V - 1, B, K1, V, i32, f32, i32, nullptr, 4, i32), ASD_ERR_INVALID_ARG);        // ld_row < V
        EXPECT(EDIT(p, BF16, K1 * V - 1, V, B, K1, V, i32, f32, i32, nullptr, 4, i32), ASD_ERR_INVALID_ARG);        // ld_seq < K1 ld_row
        EXPECT(EDIT(rows + 1, BF16, K1 * V, V, B, K1, V, i32, f32, i32, nullptr, 4, i32), ASD_ERR_ALIGNMENT);
        EXPECT(EDIT(rows + 2, 0 /*f32*/, K1 * V, V, B, K1, V, i32, f32, i32, i32, 4, i32), ASD_ERR_ALIGNMENT);
#undef EDIT
    }

    // ---- asd_logit_mask_rows: every rejection, and every "nothing to do", comes before the launch
    {
#define MASK(x_, dt_, lds_, ldr_, B_, K1_, V_, bits_, R_, row_) asd_logit_mask_rows(x_, dt_, lds_, ldr_, B_, K1_, V_, bits_, R_, row_, nullptr)
        const int K1 = 5;
        const uint32_t* u32 = reinterpret_cast<const uint32_t*>(rows);
        EXPECT(MASK(p, BF16, K1 * V, V, -1, K1, V, u32, 1, i32), ASD_ERR_INVALID_ARG);
        EXPECT(MASK(p, BF16, K1 * V, V, B, -1, V, u32, 1, i32), ASD_ERR_INVALID_ARG);
        EXPECT(MASK(p, BF16, K1 * V, V, B, K1, -1, u32, 1, i32), ASD_ERR_INVALID_ARG);
        EXPECT(MASK(p, BF16, K1 * V, V, B, K1, V, u32, -1, i32), ASD_ERR_INVALID_ARG);
        EXPECT(MASK(p, BF16, K1 * V, V, 0, K1, V, u32, -1, i32), ASD_ERR_INVALID_ARG);                 // ... before the empty batch
        EXPECT(MASK(nullptr, 99, 0, 0, 0, K1, V, nullptr, 1, nullptr), ASD_OK);                        // B == 0
        EXPECT(MASK(nullptr, 99, 0, 0, B, 0, V, nullptr, 1, nullptr), ASD_OK);                         // K1 == 0
        EXPECT(MASK(nullptr, 99, 0, 0, B, K1, 0, nullptr, 1, nullptr), ASD_OK);                        // V == 0
        EXPECT(MASK(nullptr, 99, 0, 0, B, K1, V, nullptr, 0, nullptr), ASD_OK);                        // no masks
        EXPECT(MASK(p, 99, K1 * V, V, B, K1, V, u32, 1, i32), ASD_ERR_UNSUPPORTED);                    // dtype
        EXPECT(MASK(p, -1, K1 * V, V, B, K1, V, u32, 1, i32), ASD_ERR_UNSUPPORTED);
        EXPECT(MASK(p, BF16, int64_t{1} << 40, V, INT32_MAX, K1, V, u32, 1, i32), ASD_ERR_UNSUPPORTED);   // grid
        EXPECT(MASK(nullptr, BF16, K1 * V, V, B, K1, V, u32, 1, i32), ASD_ERR_INVALID_ARG);
        EXPECT(MASK(p, BF16, K1 * V, V, B, K1, V, nullptr, 1, i32), ASD_ERR_INVALID_ARG);              // mask_bits
        EXPECT(MASK(p, BF16, K1 * V, V, B, K1, V, nullptr, 1, nullptr), ASD_ERR_INVALID_ARG);          // (mask_row may be NULL, mask_bits not)
        EXPECT(MASK(p, BF16, K1 * V, V - 1, B, K1, V, u32, 1, i32), ASD_ERR_INVALID_ARG);              // ld_row < V
        EXPECT(MASK(p, BF16, K1 * V - 1, V, B, K1, V, u32, 1, i32), ASD_ERR_INVALID_ARG);              // ld_seq < K1 ld_row
        EXPECT(MASK(rows + 1, BF16, K1 * V, V, B, K1, V, u32, 1, i32), ASD_ERR_ALIGNMENT);             // below the element size
        EXPECT(MASK(rows + 2, 0 /*f32*/, K1 * V, V, B, K1, V, u32, 1, nullptr), ASD_ERR_ALIGNMENT);
        EXPECT(MASK(p, BF16, K1 * V, V, B, K1, V, reinterpret_cast<const uint32_t*>(rows + 2), 1, nullptr), ASD_ERR_ALIGNMENT);   // mask_bits
#undef MASK
    }

    // ---- asd_penalty_rows / asd_penalty_commit: every rejection, and every "nothing to do", comes before the launch
    {
#define PEN(x_, dt_, lds_, ldr_, B_, K1_, V_, seen_, cnt_, par_, tok_, ldt_, nt_, np_) \
    asd_penalty_rows(x_, dt_, lds_, ldr_, B_, K1_, V_, seen_, cnt_, par_, tok_, ldt_, nt_, np_, nullptr)
        const int K1 = 5;
        const uint32_t* u32 = reinterpret_cast<const uint32_t*>(rows);
        const uint32_t* u32_off = reinterpret_cast<const uint32_t*>(rows + 2);
        EXPECT(PEN(p, BF16, K1 * V, V, -1, K1, V, u32, i32, f32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);
        EXPECT(PEN(p, BF16, K1 * V, V, B, -1, V, u32, i32, f32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);
        EXPECT(PEN(p, BF16, K1 * V, V, B, K1, -1, u32, i32, f32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);
        EXPECT(PEN(p, BF16, K1 * V, V, B, K1, V, u32, i32, f32, i32, 4, -1, 0), ASD_ERR_INVALID_ARG);
        EXPECT(PEN(p, BF16, K1 * V, V, B, K1, V, u32, i32, f32, i32, 4, 4, -1), ASD_ERR_INVALID_ARG);
        EXPECT(PEN(p, BF16, K1 * V, V, 0, K1, V, u32, i32, f32, i32, 4, 4, -1), ASD_ERR_INVALID_ARG);      // ... before the empty batch
        EXPECT(PEN(nullptr, 99, 0, 0, 0, K1, V, nullptr, nullptr, nullptr, nullptr, 0, 0, 0), ASD_OK);       // B == 0
        EXPECT(PEN(nullptr, 99, 0, 0, B, 0, V, nullptr, nullptr, nullptr, nullptr, 0, 0, 0), ASD_OK);        // K1 == 0
        EXPECT(PEN(nullptr, 99, 0, 0, B, K1, 0, nullptr, nullptr, nullptr, nullptr, 0, 0, 0), ASD_OK);       // V == 0
        EXPECT(PEN(p, 99, K1 * V, V, B, K1, V, u32, i32, f32, i32, 4, 4, 0), ASD_ERR_UNSUPPORTED);          // dtype
        EXPECT(PEN(p, -1, K1 * V, V, B, K1, V, u32, i32, f32, i32, 4, 4, 0), ASD_ERR_UNSUPPORTED);
        EXPECT(PEN(p, BF16, K1 * V, V, B, K1, V, u32, i32, f32, i32, 65, ASD_MAX_DRAFT_LEN + 1, 0), ASD_ERR_UNSUPPORTED);   // n_tok
        EXPECT(PEN(nullptr, BF16, K1 * V, V, B, K1, V, u32, i32, f32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);
        EXPECT(PEN(p, BF16, K1 * V, V, B, K1, V, nullptr, i32, f32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);    // seen
        EXPECT(PEN(p, BF16, K1 * V, V, B, K1, V, u32, nullptr, f32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);    // counts
        EXPECT(PEN(p, BF16, K1 * V, V, B, K1, V, u32, i32, nullptr, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);    // params
        EXPECT(PEN(p, BF16, K1 * V, V - 1, B, K1, V, u32, i32, f32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);    // ld_row < V
        EXPECT(PEN(p, BF16, K1 * V - 1, V, B, K1, V, u32, i32, f32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);    // ld_seq < K1 ld_row
        EXPECT(PEN(p, BF16, K1 * V, V, B, K1, V, u32, i32, f32, nullptr, 0, 0, 1), ASD_ERR_INVALID_ARG);    // n_prev without step_tok
        EXPECT(PEN(p, BF16, K1 * V, V, B, K1, V, u32, i32, f32, i32, 4, 4, 1), ASD_ERR_INVALID_ARG);        // position 4 would see 5 of 4
        EXPECT(PEN(p, BF16, K1 * V, V, B, K1, V, u32, i32, f32, i32, 3, 4, 0), ASD_ERR_INVALID_ARG);        // ld_tok < n_tok
        EXPECT(PEN(rows + 1, BF16, K1 * V, V, B, K1, V, u32, i32, f32, i32, 4, 4, 0), ASD_ERR_ALIGNMENT);   // below the element size
        EXPECT(PEN(rows + 2, 0 /*f32*/, K1 * V, V, B, K1, V, u32, i32, f32, nullptr, 0, 0, 0), ASD_ERR_ALIGNMENT);
        EXPECT(PEN(p, BF16, K1 * V, V, B, K1, V, u32_off, i32, f32, i32, 4, 4, 0), ASD_ERR_ALIGNMENT);      // seen
        EXPECT(PEN(p, BF16, K1 * V, V, B, K1, V, u32, reinterpret_cast<int32_t*>(rows + 2), f32, i32, 4, 4, 0), ASD_ERR_ALIGNMENT);
        EXPECT(PEN(p, BF16, K1 * V, V, B, K1, V, u32, i32, reinterpret_cast<float*>(rows + 2), i32, 4, 4, 0), ASD_ERR_ALIGNMENT);
        EXPECT(PEN(p, BF16, K1 * V, V, B, K1, V, u32, i32, f32, reinterpret_cast<int32_t*>(rows + 2), 4, 4, 0), ASD_ERR_ALIGNMENT);
#undef PEN
#define PCOMMIT(tok_, ld_, seq_, n_, B_, V_, cap_, seen_, cnt_) asd_penalty_commit(tok_, ld_, seq_, n_, B_, V_, cap_, seen_, cnt_, nullptr)
        uint32_t* seen = reinterpret_cast<uint32_t*>(rows);
        EXPECT(PCOMMIT(i32, 32, i32, i32, -1, V, 32, seen, i32), ASD_ERR_INVALID_ARG);
        EXPECT(PCOMMIT(i32, 32, i32, i32, B, -1, 32, seen, i32), ASD_ERR_INVALID_ARG);
        EXPECT(PCOMMIT(i32, 32, i32, i32, B, V, -1, seen, i32), ASD_ERR_INVALID_ARG);
        EXPECT(PCOMMIT(nullptr, 0, nullptr, nullptr, 0, V, 32, nullptr, nullptr), ASD_OK);                  // B == 0
        EXPECT(PCOMMIT(nullptr, 0, nullptr, nullptr, B, 0, 32, nullptr, nullptr), ASD_OK);                  // V == 0
        EXPECT(PCOMMIT(nullptr, 0, nullptr, nullptr, B, V, 0, nullptr, nullptr), ASD_OK);                   // max_len == 0
        EXPECT(PCOMMIT(nullptr, 32, i32, i32, B, V, 32, seen, i32), ASD_ERR_INVALID_ARG);
        EXPECT(PCOMMIT(i32, 32, nullptr, i32, B, V, 32, seen, i32), ASD_ERR_INVALID_ARG);
        EXPECT(PCOMMIT(i32, 32, i32, nullptr, B, V, 32, seen, i32), ASD_ERR_INVALID_ARG);
        EXPECT(PCOMMIT(i32, 32, i32, i32, B, V, 32, nullptr, i32), ASD_ERR_INVALID_ARG);
        EXPECT(PCOMMIT(i32, 32, i32, i32, B, V, 32, seen, nullptr), ASD_ERR_INVALID_ARG);
        EXPECT(PCOMMIT(i32, 31, i32, i32, B, V, 32, seen, i32), ASD_ERR_INVALID_ARG);                       // ld_tokens < max_len
        EXPECT(PCOMMIT(reinterpret_cast<int32_t*>(rows + 2), 32, i32, i32, B, V, 32, seen, i32), ASD_ERR_ALIGNMENT);
        EXPECT(PCOMMIT(i32, 32, i32, i32, B, V, 32, reinterpret_cast<uint32_t*>(rows + 2), i32), ASD_ERR_ALIGNMENT);
        EXPECT(PCOMMIT(i32, 32, i32, i32, B, V, 32, seen, reinterpret_cast<int32_t*>(rows + 2)), ASD_ERR_ALIGNMENT);
#undef PCOMMIT
    }

    // ---- asd_bad_words_rows: every rejection, and every "nothing to do", comes before the launch
    {
#define BADW(x_, dt_, lds_, ldr_, B_, K1_, V_, wt_, wn_, rf_, n_, tk_, ldk_, sl_, st_, ml_, tok_, ldt_, nt_, np_) \
    asd_bad_words_rows(x_, dt_, lds_, ldr_, B_, K1_, V_, wt_, wn_, rf_, n_, tk_, ldk_, sl_, st_, ml_, tok_, ldt_, nt_, np_, nullptr)
        const int K1 = 5;
        int32_t* off = reinterpret_cast<int32_t*>(rows + 2);
        EXPECT(BADW(p, BF16, K1 * V, V, -1, K1, V, i32, i32, i32, 8, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);
        EXPECT(BADW(p, BF16, K1 * V, V, B, -1, V, i32, i32, i32, 8, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, -1, i32, i32, i32, 8, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, i32, i32, -1, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, i32, i32, 8, i32, 32, i32, -1, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);   // start
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, i32, i32, 8, i32, 32, i32, 4, -1, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);    // max_len
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, i32, i32, 8, i32, 32, i32, 4, 32, i32, 4, -1, 0), ASD_ERR_INVALID_ARG);   // n_tok
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, i32, i32, 8, i32, 32, i32, 4, 32, i32, 4, 4, -1), ASD_ERR_INVALID_ARG);   // n_prev
        EXPECT(BADW(p, BF16, K1 * V, V, 0, K1, V, i32, i32, i32, 8, i32, 32, i32, 4, 32, i32, 4, 4, -1), ASD_ERR_INVALID_ARG);   // ... before the empty batch
        EXPECT(BADW(nullptr, 99, 0, 0, 0, K1, V, nullptr, nullptr, nullptr, 8, nullptr, 0, nullptr, 0, 0, nullptr, 0, 0, 0), ASD_OK);   // B == 0
        EXPECT(BADW(nullptr, 99, 0, 0, B, 0, V, nullptr, nullptr, nullptr, 8, nullptr, 0, nullptr, 0, 0, nullptr, 0, 0, 0), ASD_OK);    // K1 == 0
        EXPECT(BADW(nullptr, 99, 0, 0, B, K1, 0, nullptr, nullptr, nullptr, 8, nullptr, 0, nullptr, 0, 0, nullptr, 0, 0, 0), ASD_OK);   // V == 0
        EXPECT(BADW(nullptr, 99, 0, 0, B, K1, V, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, 0, nullptr, 0, 0, 0), ASD_OK);   // no word
        EXPECT(BADW(p, 99, K1 * V, V, B, K1, V, i32, i32, i32, 8, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_UNSUPPORTED);     // dtype
        EXPECT(BADW(p, -1, K1 * V, V, B, K1, V, i32, i32, i32, 8, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_UNSUPPORTED);
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, i32, nullptr, ASD_MAX_BAD_WORDS + 1, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_UNSUPPORTED);
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, i32, i32, 8, i32, 32, i32, 4, 32, i32, 65, ASD_MAX_DRAFT_LEN + 1, 0), ASD_ERR_UNSUPPORTED);
        EXPECT(BADW(nullptr, 99, K1 * V, V, B, K1, V, i32, i32, i32, 8, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_UNSUPPORTED);  // ... before the NULL checks
        EXPECT(BADW(nullptr, BF16, K1 * V, V, B, K1, V, i32, i32, i32, 8, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, nullptr, i32, i32, 8, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);  // word_tok
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, nullptr, i32, 8, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);  // word_n
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, i32, i32, 8, nullptr, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);  // tokens
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, i32, i32, 8, i32, 32, nullptr, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);  // seq_len
        EXPECT(BADW(p, BF16, K1 * V, V - 1, B, K1, V, i32, i32, i32, 8, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);  // ld_row < V
        EXPECT(BADW(p, BF16, K1 * V - 1, V, B, K1, V, i32, i32, i32, 8, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);  // ld_seq < K1 ld_row
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, i32, i32, 8, i32, 31, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);      // ld_tokens < max_len
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, i32, i32, 8, i32, 32, i32, 33, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);     // start > max_len
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, i32, i32, 8, i32, 32, i32, 4, 32, nullptr, 0, 0, 1), ASD_ERR_INVALID_ARG);  // n_prev without step_tok
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, i32, i32, 8, i32, 32, i32, 4, 32, i32, 4, 4, 1), ASD_ERR_INVALID_ARG);      // position 4 would see 5 of 4
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, i32, i32, 8, i32, 32, i32, 4, 32, i32, 3, 4, 0), ASD_ERR_INVALID_ARG);      // ld_tok < n_tok
        EXPECT(BADW(rows + 1, BF16, K1 * V, V - 1, B, K1, V, i32, i32, i32, 8, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);   // ... before alignment
        EXPECT(BADW(rows + 1, BF16, K1 * V, V, B, K1, V, i32, i32, i32, 8, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_ALIGNMENT);   // below the element size
        EXPECT(BADW(rows + 2, 0 /*f32*/, K1 * V, V, B, K1, V, i32, i32, i32, 8, i32, 32, i32, 4, 32, nullptr, 0, 0, 0), ASD_ERR_ALIGNMENT);
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, off, i32, i32, 8, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_ALIGNMENT);        // word_tok
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, off, i32, 8, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_ALIGNMENT);        // word_n
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, i32, off, 8, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_ALIGNMENT);        // row_first
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, i32, i32, 8, off, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_ALIGNMENT);        // tokens
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, i32, i32, 8, i32, 32, off, 4, 32, i32, 4, 4, 0), ASD_ERR_ALIGNMENT);        // seq_len
        EXPECT(BADW(p, BF16, K1 * V, V, B, K1, V, i32, i32, i32, 8, i32, 32, i32, 4, 32, off, 4, 4, 0), ASD_ERR_ALIGNMENT);        // step_tok
#undef BADW
    }

    // ---- asd_fsm_mask_rows / asd_fsm_advance / asd_fsm_commit: every rejection, and every "nothing to do", comes before the launch
    {
#define FMASK(x_, dt_, lds_, ldr_, B_, K1_, V_, bits_, S_, pos_, ldst_, first_) \
    asd_fsm_mask_rows(x_, dt_, lds_, ldr_, B_, K1_, V_, bits_, S_, pos_, ldst_, first_, nullptr)
#define FADV(sf_, et_, en_, so_, S_, E_, V_, pos_, ldst_, B_, k_, tok_, ldt_, nt_) \
    asd_fsm_advance(sf_, et_, en_, so_, S_, E_, V_, pos_, ldst_, B_, k_, tok_, ldt_, nt_, nullptr)
#define FCOM(sf_, et_, en_, so_, S_, E_, V_, pos_, ldst_, B_, tk_, ldk_, sl_, nc_, ml_) \
    asd_fsm_commit(sf_, et_, en_, so_, S_, E_, V_, pos_, ldst_, B_, tk_, ldk_, sl_, nc_, ml_, nullptr)
        const int K1 = 5, S = 7, E = 9;
        const uint32_t* bits = reinterpret_cast<const uint32_t*>(rows);
        int32_t* off = reinterpret_cast<int32_t*>(rows + 2);
        EXPECT(FMASK(p, BF16, K1 * V, V, -1, K1, V, bits, S, i32, 5, 0), ASD_ERR_INVALID_ARG);
        EXPECT(FMASK(p, BF16, K1 * V, V, B, -1, V, bits, S, i32, 5, 0), ASD_ERR_INVALID_ARG);
        EXPECT(FMASK(p, BF16, K1 * V, V, B, K1, -1, bits, S, i32, 5, 0), ASD_ERR_INVALID_ARG);
        EXPECT(FMASK(p, BF16, K1 * V, V, B, K1, V, bits, -1, i32, 5, 0), ASD_ERR_INVALID_ARG);
        EXPECT(FMASK(p, BF16, K1 * V, V, B, K1, V, bits, S, i32, 5, -1), ASD_ERR_INVALID_ARG);      // first
        EXPECT(FMASK(p, BF16, K1 * V, V, B, K1, V, bits, S, i32, -1, 0), ASD_ERR_INVALID_ARG);      // ld_state
        EXPECT(FMASK(p, BF16, K1 * V, V, 0, K1, V, bits, S, i32, 5, -1), ASD_ERR_INVALID_ARG);      // ... before the empty batch
        EXPECT(FMASK(nullptr, 99, 0, 0, 0, K1, V, nullptr, S, nullptr, 0, 0), ASD_OK);              // B == 0
        EXPECT(FMASK(nullptr, 99, 0, 0, B, 0, V, nullptr, S, nullptr, 0, 0), ASD_OK);               // K1 == 0
        EXPECT(FMASK(nullptr, 99, 0, 0, B, K1, 0, nullptr, S, nullptr, 0, 0), ASD_OK);              // V == 0
        EXPECT(FMASK(nullptr, 99, 0, 0, B, K1, V, nullptr, 0, nullptr, 0, 0), ASD_OK);              // no state
        EXPECT(FMASK(p, 99, K1 * V, V, B, K1, V, bits, S, i32, 5, 0), ASD_ERR_UNSUPPORTED);         // dtype
        EXPECT(FMASK(nullptr, 99, K1 * V, V, B, K1, V, bits, S, i32, 5, 0), ASD_ERR_UNSUPPORTED);   // ... before the NULL checks
        EXPECT(FMASK(nullptr, BF16, K1 * V, V, B, K1, V, bits, S, i32, 5, 0), ASD_ERR_INVALID_ARG);
        EXPECT(FMASK(p, BF16, K1 * V, V, B, K1, V, nullptr, S, i32, 5, 0), ASD_ERR_INVALID_ARG);    // state_bits
        EXPECT(FMASK(p, BF16, K1 * V, V, B, K1, V, bits, S, nullptr, 5, 0), ASD_ERR_INVALID_ARG);   // pos_state
        EXPECT(FMASK(p, BF16, K1 * V, V - 1, B, K1, V, bits, S, i32, 5, 0), ASD_ERR_INVALID_ARG);   // ld_row < V
        EXPECT(FMASK(p, BF16, K1 * V - 1, V, B, K1, V, bits, S, i32, 5, 0), ASD_ERR_INVALID_ARG);   // ld_seq < K1 ld_row
        EXPECT(FMASK(p, BF16, K1 * V, V, B, K1, V, bits, S, i32, 5, 1), ASD_ERR_INVALID_ARG);       // positions 1 .. 5 of 5 columns
        EXPECT(FMASK(p, BF16, K1 * V, V, B, K1, V, bits, S, i32, 4, 0), ASD_ERR_INVALID_ARG);
        EXPECT(FMASK(rows + 1, BF16, K1 * V, V - 1, B, K1, V, bits, S, i32, 5, 0), ASD_ERR_INVALID_ARG);   // ... before alignment
        EXPECT(FMASK(rows + 1, BF16, K1 * V, V, B, K1, V, bits, S, i32, 5, 0), ASD_ERR_ALIGNMENT);  // below the element size
        EXPECT(FMASK(rows + 2, 0 /*f32*/, K1 * V, V, B, K1, V, bits, S, i32, 5, 0), ASD_ERR_ALIGNMENT);
        EXPECT(FMASK(p, BF16, K1 * V, V, B, K1, V, reinterpret_cast<const uint32_t*>(rows + 2), S, i32, 5, 0), ASD_ERR_ALIGNMENT);
        EXPECT(FMASK(p, BF16, K1 * V, V, B, K1, V, bits, S, off, 5, 0), ASD_ERR_ALIGNMENT);

        EXPECT(FADV(i32, i32, i32, i32, S, E, V, i32, 5, -1, 1, i32, 4, 4), ASD_ERR_INVALID_ARG);
        EXPECT(FADV(i32, i32, i32, i32, -1, E, V, i32, 5, B, 1, i32, 4, 4), ASD_ERR_INVALID_ARG);
        EXPECT(FADV(i32, i32, i32, i32, S, -1, V, i32, 5, B, 1, i32, 4, 4), ASD_ERR_INVALID_ARG);
        EXPECT(FADV(i32, i32, i32, i32, S, E, -1, i32, 5, B, 1, i32, 4, 4), ASD_ERR_INVALID_ARG);
        EXPECT(FADV(i32, i32, i32, i32, S, E, V, i32, 5, B, -1, i32, 4, 4), ASD_ERR_INVALID_ARG);   // k
        EXPECT(FADV(i32, i32, i32, i32, S, E, V, i32, 5, B, 1, i32, 4, -1), ASD_ERR_INVALID_ARG);   // n_tok
        EXPECT(FADV(i32, i32, i32, i32, S, E, V, i32, -1, B, 1, i32, 4, 4), ASD_ERR_INVALID_ARG);   // ld_state
        EXPECT(FADV(i32, i32, i32, i32, S, E, V, i32, 5, 0, -1, i32, 4, 4), ASD_ERR_INVALID_ARG);   // ... before the empty batch
        EXPECT(FADV(nullptr, nullptr, nullptr, nullptr, S, E, V, nullptr, 0, 0, 0, nullptr, 0, 0), ASD_OK);   // B == 0
        EXPECT(FADV(i32, i32, i32, i32, S, E, V, i32, 5, B, 1, i32, 65, ASD_MAX_DRAFT_LEN + 1), ASD_ERR_UNSUPPORTED);
        EXPECT(FADV(nullptr, i32, i32, i32, S, E, V, i32, 5, B, 1, i32, 65, ASD_MAX_DRAFT_LEN + 1), ASD_ERR_UNSUPPORTED);   // ... before the NULL checks
        EXPECT(FADV(nullptr, i32, i32, i32, S, E, V, i32, 5, B, 1, i32, 4, 4), ASD_ERR_INVALID_ARG);   // state_first
        EXPECT(FADV(i32, nullptr, i32, i32, S, E, V, i32, 5, B, 1, i32, 4, 4), ASD_ERR_INVALID_ARG);   // edge_tok with E > 0
        EXPECT(FADV(i32, i32, nullptr, i32, S, E, V, i32, 5, B, 1, i32, 4, 4), ASD_ERR_INVALID_ARG);   // edge_next with E > 0
        EXPECT(FADV(i32, i32, i32, nullptr, S, E, V, i32, 5, B, 1, i32, 4, 4), ASD_ERR_INVALID_ARG);   // state_other
        EXPECT(FADV(i32, i32, i32, i32, S, E, V, nullptr, 5, B, 1, i32, 4, 4), ASD_ERR_INVALID_ARG);   // pos_state
        EXPECT(FADV(i32, i32, i32, i32, S, E, V, i32, 5, B, 1, nullptr, 4, 4), ASD_ERR_INVALID_ARG);   // step_tok
        EXPECT(FADV(i32, i32, i32, i32, S, E, V, i32, 5, B, 4, i32, 8, 8), ASD_ERR_INVALID_ARG);       // k + 1 == ld_state
        EXPECT(FADV(i32, i32, i32, i32, S, E, V, i32, 9, B, 4, i32, 4, 4), ASD_ERR_INVALID_ARG);       // k == n_tok
        EXPECT(FADV(i32, i32, i32, i32, S, E, V, i32, 5, B, 1, i32, 3, 4), ASD_ERR_INVALID_ARG);       // ld_tok < n_tok
        EXPECT(FADV(off, i32, i32, i32, S, E, V, i32, 5, B, 4, i32, 8, 8), ASD_ERR_INVALID_ARG);       // ... before alignment
        EXPECT(FADV(off, i32, i32, i32, S, E, V, i32, 5, B, 1, i32, 4, 4), ASD_ERR_ALIGNMENT);
        EXPECT(FADV(i32, off, i32, i32, S, E, V, i32, 5, B, 1, i32, 4, 4), ASD_ERR_ALIGNMENT);
        EXPECT(FADV(i32, i32, off, i32, S, E, V, i32, 5, B, 1, i32, 4, 4), ASD_ERR_ALIGNMENT);
        EXPECT(FADV(i32, i32, i32, off, S, E, V, i32, 5, B, 1, i32, 4, 4), ASD_ERR_ALIGNMENT);
        EXPECT(FADV(i32, i32, i32, i32, S, E, V, off, 5, B, 1, i32, 4, 4), ASD_ERR_ALIGNMENT);
        EXPECT(FADV(i32, i32, i32, i32, S, E, V, i32, 5, B, 1, off, 4, 4), ASD_ERR_ALIGNMENT);

        EXPECT(FCOM(i32, i32, i32, i32, S, E, V, i32, 5, -1, i32, 32, i32, i32, 32), ASD_ERR_INVALID_ARG);
        EXPECT(FCOM(i32, i32, i32, i32, -1, E, V, i32, 5, B, i32, 32, i32, i32, 32), ASD_ERR_INVALID_ARG);
        EXPECT(FCOM(i32, i32, i32, i32, S, -1, V, i32, 5, B, i32, 32, i32, i32, 32), ASD_ERR_INVALID_ARG);
        EXPECT(FCOM(i32, i32, i32, i32, S, E, -1, i32, 5, B, i32, 32, i32, i32, 32), ASD_ERR_INVALID_ARG);
        EXPECT(FCOM(i32, i32, i32, i32, S, E, V, i32, 5, B, i32, 32, i32, i32, -1), ASD_ERR_INVALID_ARG);   // max_len
        EXPECT(FCOM(i32, i32, i32, i32, S, E, V, i32, -1, B, i32, 32, i32, i32, 32), ASD_ERR_INVALID_ARG);  // ld_state
        EXPECT(FCOM(i32, i32, i32, i32, S, E, V, i32, 5, 0, i32, 32, i32, i32, -1), ASD_ERR_INVALID_ARG);   // ... before the empty batch
        EXPECT(FCOM(nullptr, nullptr, nullptr, nullptr, S, E, V, nullptr, 0, 0, nullptr, 0, nullptr, nullptr, 0), ASD_OK);   // B == 0
        EXPECT(FCOM(nullptr, i32, i32, i32, S, E, V, i32, 5, B, i32, 32, i32, i32, 32), ASD_ERR_INVALID_ARG);   // state_first
        EXPECT(FCOM(i32, nullptr, i32, i32, S, E, V, i32, 5, B, i32, 32, i32, i32, 32), ASD_ERR_INVALID_ARG);   // edge_tok with E > 0
        EXPECT(FCOM(i32, i32, nullptr, i32, S, E, V, i32, 5, B, i32, 32, i32, i32, 32), ASD_ERR_INVALID_ARG);   // edge_next with E > 0
        EXPECT(FCOM(i32, i32, i32, nullptr, S, E, V, i32, 5, B, i32, 32, i32, i32, 32), ASD_ERR_INVALID_ARG);   // state_other
        EXPECT(FCOM(i32, i32, i32, i32, S, E, V, nullptr, 5, B, i32, 32, i32, i32, 32), ASD_ERR_INVALID_ARG);   // pos_state
        EXPECT(FCOM(i32, i32, i32, i32, S, E, V, i32, 5, B, nullptr, 32, i32, i32, 32), ASD_ERR_INVALID_ARG);   // tokens
        EXPECT(FCOM(i32, i32, i32, i32, S, E, V, i32, 5, B, i32, 32, nullptr, i32, 32), ASD_ERR_INVALID_ARG);   // seq_len
        EXPECT(FCOM(i32, i32, i32, i32, S, E, V, i32, 5, B, i32, 32, i32, nullptr, 32), ASD_ERR_INVALID_ARG);   // n_commit
        EXPECT(FCOM(i32, i32, i32, i32, S, E, V, i32, 0, B, i32, 32, i32, i32, 32), ASD_ERR_INVALID_ARG);       // ld_state < 1
        EXPECT(FCOM(i32, i32, i32, i32, S, E, V, i32, 5, B, i32, 32, i32, i32, 0), ASD_ERR_INVALID_ARG);        // max_len < 1
        EXPECT(FCOM(i32, i32, i32, i32, S, E, V, i32, 5, B, i32, 31, i32, i32, 32), ASD_ERR_INVALID_ARG);       // ld_tokens < max_len
        EXPECT(FCOM(off, i32, i32, i32, S, E, V, i32, 5, B, i32, 31, i32, i32, 32), ASD_ERR_INVALID_ARG);       // ... before alignment
        EXPECT(FCOM(off, i32, i32, i32, S, E, V, i32, 5, B, i32, 32, i32, i32, 32), ASD_ERR_ALIGNMENT);
        EXPECT(FCOM(i32, off, i32, i32, S, E, V, i32, 5, B, i32, 32, i32, i32, 32), ASD_ERR_ALIGNMENT);
        EXPECT(FCOM(i32, i32, off, i32, S, E, V, i32, 5, B, i32, 32, i32, i32, 32), ASD_ERR_ALIGNMENT);
        EXPECT(FCOM(i32, i32, i32, off, S, E, V, i32, 5, B, i32, 32, i32, i32, 32), ASD_ERR_ALIGNMENT);
        EXPECT(FCOM(i32, i32, i32, i32, S, E, V, off, 5, B, i32, 32, i32, i32, 32), ASD_ERR_ALIGNMENT);
        EXPECT(FCOM(i32, i32, i32, i32, S, E, V, i32, 5, B, off, 32, i32, i32, 32), ASD_ERR_ALIGNMENT);
        EXPECT(FCOM(i32, i32, i32, i32, S, E, V, i32, 5, B, i32, 32, off, i32, 32), ASD_ERR_ALIGNMENT);
        EXPECT(FCOM(i32, i32, i32, i32, S, E, V, i32, 5, B, i32, 32, i32, off, 32), ASD_ERR_ALIGNMENT);
#undef FMASK
#undef FADV
#undef FCOM
    }

    // ---- asd_no_repeat_ngram_rows: every rejection, and every "nothing to do", comes before the launch
    {
#define NGRAM(x_, dt_, lds_, ldr_, B_, K1_, V_, nn_, n_, rs_, tk_, ldk_, sl_, st_, ml_, tok_, ldt_, nt_, np_) \
    asd_no_repeat_ngram_rows(x_, dt_, lds_, ldr_, B_, K1_, V_, nn_, n_, rs_, tk_, ldk_, sl_, st_, ml_, tok_, ldt_, nt_, np_, nullptr)
        const int K1 = 5;
        int32_t* off = reinterpret_cast<int32_t*>(rows + 2);
        EXPECT(NGRAM(p, BF16, K1 * V, V, -1, K1, V, i32, 0, i32, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, -1, V, i32, 0, i32, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, -1, i32, 0, i32, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, i32, -1, i32, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);   // n_shared
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, i32, 0, i32, i32, 32, i32, -1, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);   // start
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, i32, 0, i32, i32, 32, i32, 4, -1, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);    // max_len
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, i32, 0, i32, i32, 32, i32, 4, 32, i32, 4, -1, 0), ASD_ERR_INVALID_ARG);   // n_tok
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, i32, 0, i32, i32, 32, i32, 4, 32, i32, 4, 4, -1), ASD_ERR_INVALID_ARG);   // n_prev
        EXPECT(NGRAM(p, BF16, K1 * V, V, 0, K1, V, i32, 0, i32, i32, 32, i32, 4, 32, i32, 4, 4, -1), ASD_ERR_INVALID_ARG);   // ... before the empty batch
        EXPECT(NGRAM(nullptr, 99, 0, 0, 0, K1, V, nullptr, 3, nullptr, nullptr, 0, nullptr, 0, 0, nullptr, 0, 0, 0), ASD_OK);   // B == 0
        EXPECT(NGRAM(nullptr, 99, 0, 0, B, 0, V, nullptr, 3, nullptr, nullptr, 0, nullptr, 0, 0, nullptr, 0, 0, 0), ASD_OK);    // K1 == 0
        EXPECT(NGRAM(nullptr, 99, 0, 0, B, K1, 0, nullptr, 3, nullptr, nullptr, 0, nullptr, 0, 0, nullptr, 0, 0, 0), ASD_OK);   // V == 0
        EXPECT(NGRAM(nullptr, 99, 0, 0, B, K1, V, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, 0, nullptr, 0, 0, 0), ASD_OK);   // every row off
        EXPECT(NGRAM(p, 99, K1 * V, V, B, K1, V, i32, 0, i32, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_UNSUPPORTED);     // dtype
        EXPECT(NGRAM(p, -1, K1 * V, V, B, K1, V, i32, 0, i32, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_UNSUPPORTED);
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, nullptr, ASD_MAX_NGRAM + 1, i32, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_UNSUPPORTED);
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, i32, 0, i32, i32, 32, i32, 4, 32, i32, 65, ASD_MAX_DRAFT_LEN + 1, 0), ASD_ERR_UNSUPPORTED);
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, i32, 0, i32, i32, INT64_C(1) << 31, i32, 4, INT32_MAX - 200, i32, 4, 4, 0), ASD_ERR_UNSUPPORTED);   // the scan counts in int32
        EXPECT(NGRAM(nullptr, 99, K1 * V, V, B, K1, V, i32, 0, i32, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_UNSUPPORTED);  // ... before the NULL checks
        EXPECT(NGRAM(nullptr, BF16, K1 * V, V, B, K1, V, i32, 0, i32, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, i32, 0, i32, nullptr, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);  // tokens
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, i32, 0, i32, i32, 32, nullptr, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);  // seq_len
        EXPECT(NGRAM(p, BF16, K1 * V, V - 1, B, K1, V, i32, 0, i32, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);  // ld_row < V
        EXPECT(NGRAM(p, BF16, K1 * V - 1, V, B, K1, V, i32, 0, i32, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);  // ld_seq < K1 ld_row
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, i32, 0, i32, i32, 31, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);      // ld_tokens < max_len
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, i32, 0, i32, i32, 32, i32, 33, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);     // start > max_len
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, i32, 0, i32, i32, 32, i32, 4, 32, nullptr, 0, 0, 1), ASD_ERR_INVALID_ARG);  // n_prev without step_tok
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, i32, 0, i32, i32, 32, i32, 4, 32, i32, 4, 4, 1), ASD_ERR_INVALID_ARG);      // position 4 would see 5 of 4
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, i32, 0, i32, i32, 32, i32, 4, 32, i32, 3, 4, 0), ASD_ERR_INVALID_ARG);      // ld_tok < n_tok
        EXPECT(NGRAM(rows + 1, BF16, K1 * V, V - 1, B, K1, V, i32, 0, i32, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_INVALID_ARG);   // ... before alignment
        EXPECT(NGRAM(rows + 1, BF16, K1 * V, V, B, K1, V, i32, 0, i32, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_ALIGNMENT);   // below the element size
        EXPECT(NGRAM(rows + 2, 0 /*f32*/, K1 * V, V, B, K1, V, i32, 0, i32, i32, 32, i32, 4, 32, nullptr, 0, 0, 0), ASD_ERR_ALIGNMENT);
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, off, 0, i32, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_ALIGNMENT);        // ngram_n
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, i32, 0, off, i32, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_ALIGNMENT);        // row_start
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, i32, 0, i32, off, 32, i32, 4, 32, i32, 4, 4, 0), ASD_ERR_ALIGNMENT);        // tokens
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, i32, 0, i32, i32, 32, off, 4, 32, i32, 4, 4, 0), ASD_ERR_ALIGNMENT);        // seq_len
        EXPECT(NGRAM(p, BF16, K1 * V, V, B, K1, V, i32, 0, i32, i32, 32, i32, 4, 32, off, 4, 4, 0), ASD_ERR_ALIGNMENT);        // step_tok
#undef NGRAM
    }

    // ---- asd_prompt_logprobs: the header's order (NULL outputs and the temperature, sizes, the empty batch, dtype, N / splits,
    // pointers and strides, a 2 GiB row, alignment, the workspace) and the size query, which is sized for the splits in use
    {
        const int T = 70, VP = 1000, NP = 5;
        const int64_t ldr = VP, lds = static_cast<int64_t>(T) * VP, ldt = T;
        const size_t ws64 = asd_prompt_logprobs_workspace_bytes(B, T, VP, BF16, ASD_MAX_SPLITS);
        const size_t ws2 = asd_prompt_logprobs_workspace_bytes(B, T, VP, BF16, 2);
        if (ws64 % 256 != 0 || ws2 % 256 != 0 || ws2 >= ws64 || asd_prompt_logprobs_workspace_bytes(B, T, VP, BF16, 1) != 256 ||
            asd_prompt_logprobs_workspace_bytes(0, T, VP, BF16, 0) != 256 || asd_prompt_logprobs_workspace_bytes(B, T, VP, 99, 0) != 256 ||
            asd_prompt_logprobs_workspace_bytes(32, 2047, 152064, BF16, 0) >= (size_t{1} << 20)) {
            std::printf("FAIL prompt_logprobs workspace sizes %zu %zu\n", ws2, ws64);
            ++failures;
        }
#define PROMPT(x_, dt_, lds_, ldr_, B_, T_, V_, tg_, ldt_, first_, inv_t_, N_, splits_, lp_, rank_, id_, tlp_, ws_, wsb_) \
    asd_prompt_logprobs(x_, dt_, lds_, ldr_, B_, T_, V_, tg_, ldt_, first_, inv_t_, N_, splits_, lp_, rank_, id_, tlp_, ws_, wsb_, nullptr)
        EXPECT(PROMPT(p, BF16, lds, ldr, B, T, VP, i32, ldt, i32, 1.0f, NP, 0, nullptr, i32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);     // lp
        EXPECT(PROMPT(p, BF16, lds, ldr, B, T, VP, i32, ldt, i32, 1.0f, NP, 0, f32, nullptr, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);     // rank
        EXPECT(PROMPT(p, BF16, lds, ldr, B, T, VP, i32, ldt, i32, 1.0f, NP, 0, f32, i32, nullptr, f32, p, ws64), ASD_ERR_INVALID_ARG);     // top_id with N > 0
        EXPECT(PROMPT(p, BF16, lds, ldr, B, T, VP, i32, ldt, i32, 1.0f, NP, 0, f32, i32, i32, nullptr, p, ws64), ASD_ERR_INVALID_ARG);     // top_lp with N > 0
        EXPECT(PROMPT(p, BF16, lds, ldr, B, T, VP, i32, ldt, i32, 1.0f, 0, 2, f32, i32, nullptr, nullptr, p, 0), ASD_ERR_WORKSPACE);       // N == 0 needs no table
        EXPECT(PROMPT(p, BF16, lds, ldr, B, T, VP, i32, ldt, i32, 0.0f, NP, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);         // temperature
        EXPECT(PROMPT(p, BF16, lds, ldr, B, T, VP, i32, ldt, i32, NAN, NP, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);
        EXPECT(PROMPT(p, BF16, lds, ldr, -1, T, VP, i32, ldt, i32, 1.0f, NP, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);        // negative sizes
        EXPECT(PROMPT(p, BF16, lds, ldr, B, -1, VP, i32, ldt, i32, 1.0f, NP, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);
        EXPECT(PROMPT(p, BF16, lds, ldr, B, T, -1, i32, ldt, i32, 1.0f, NP, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);
        EXPECT(PROMPT(p, BF16, lds, ldr, B, T, VP, i32, ldt, i32, 1.0f, -1, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);
        EXPECT(PROMPT(nullptr, 99, 0, 0, 0, T, VP, nullptr, 0, nullptr, 1.0f, 99, 99, nullptr, nullptr, nullptr, nullptr, nullptr, 0), ASD_OK);   // B == 0: nothing launched
        EXPECT(PROMPT(p, BF16, 0, ldr, B, 0, VP, i32, 0, i32, 1.0f, NP, 0, nullptr, nullptr, nullptr, nullptr, p, 0), ASD_OK);             // T == 0 likewise
        EXPECT(PROMPT(p, BF16, 0, 0, B, T, 0, i32, ldt, i32, 1.0f, NP, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);              // V == 0
        EXPECT(PROMPT(p, 99, lds, ldr, B, T, VP, i32, ldt, i32, 1.0f, NP, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_UNSUPPORTED);           // dtype
        EXPECT(PROMPT(p, 99, lds, ldr, B, T, VP, i32, ldt, i32, 1.0f, ASD_MAX_TOP_LOGPROBS + 1, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_UNSUPPORTED);
        EXPECT(PROMPT(p, BF16, lds, ldr, B, T, VP, i32, ldt, i32, 1.0f, ASD_MAX_TOP_LOGPROBS + 1, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_UNSUPPORTED);   // N
        EXPECT(PROMPT(p, BF16, lds, ldr - 1, B, T, VP, i32, ldt, i32, 1.0f, ASD_MAX_TOP_LOGPROBS + 1, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_UNSUPPORTED);   // ... before the strides
        EXPECT(PROMPT(p, BF16, lds, ldr, B, T, VP, i32, ldt, i32, 1.0f, NP, -1, f32, i32, i32, f32, p, ws64), ASD_ERR_UNSUPPORTED);        // splits
        EXPECT(PROMPT(p, BF16, lds, ldr, B, T, VP, i32, ldt, i32, 1.0f, NP, ASD_MAX_SPLITS + 1, f32, i32, i32, f32, p, ws64), ASD_ERR_UNSUPPORTED);
        EXPECT(PROMPT(nullptr, BF16, lds, ldr, B, T, VP, i32, ldt, i32, 1.0f, NP, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);   // logits
        EXPECT(PROMPT(p, BF16, lds, ldr, B, T, VP, nullptr, ldt, i32, 1.0f, NP, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);     // target
        EXPECT(PROMPT(p, BF16, lds, ldr, B, T, VP, i32, ldt, i32, 1.0f, NP, 0, f32, i32, i32, f32, nullptr, ws64), ASD_ERR_INVALID_ARG);   // workspace
        EXPECT(PROMPT(p, BF16, lds, ldr - 1, B, T, VP, i32, ldt, i32, 1.0f, NP, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);     // ld_row < V
        EXPECT(PROMPT(p, BF16, lds - 1, ldr, B, T, VP, i32, ldt, i32, 1.0f, NP, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);     // ld_seq < T ld_row
        EXPECT(PROMPT(p, BF16, lds, ldr, B, T, VP, i32, ldt - 1, i32, 1.0f, NP, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);     // ld_target < T
        EXPECT(PROMPT(rows + 1, BF16, lds, ldr, B, T, VP, i32, ldt - 1, i32, 1.0f, NP, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);   // ... before alignment
        EXPECT(PROMPT(rows + 1, BF16, static_cast<int64_t>(T) << 30, int64_t{1} << 30, B, T, 1 << 30, i32, ldt, i32, 1.0f, NP, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_UNSUPPORTED);   // a 2 GiB row, before alignment
        EXPECT(PROMPT(rows + 1, BF16, lds, ldr, B, T, VP, i32, ldt, i32, 1.0f, NP, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_ALIGNMENT);    // below the element size
        EXPECT(PROMPT(rows + 2, 0 /*f32*/, lds, ldr, B, T, VP, i32, ldt, i32, 1.0f, NP, 0, f32, i32, i32, f32, p, ws64), ASD_ERR_ALIGNMENT);
        EXPECT(PROMPT(p, BF16, lds, ldr, B, T, VP, i32, ldt, i32, 1.0f, NP, 0, f32, i32, i32, f32, rows + 16, ws64), ASD_ERR_WORKSPACE);   // misaligned workspace
        EXPECT(PROMPT(p, BF16, lds, ldr, B, T, VP, i32, ldt, i32, 1.0f, NP, ASD_MAX_SPLITS, f32, i32, i32, f32, p, ws64 - 1), ASD_ERR_WORKSPACE);   // too small
        EXPECT(PROMPT(p, BF16, lds, ldr, B, T, VP, i32, ldt, i32, 1.0f, NP, 2, f32, i32, i32, f32, p, ws2 - 1), ASD_ERR_WORKSPACE);
        EXPECT(PROMPT(rows + 2, BF16, lds, ldr, B, T, VP, i32, ldt, nullptr, 1.0f, NP, 1, f32, i32, i32, f32, p, 255), ASD_ERR_WORKSPACE); // (an element-aligned base and a NULL `first` are valid)
        EXPECT(PROMPT(p, BF16, int64_t{VP} << 10, ldr, 1 << 20, 1 << 10, VP, i32, 1 << 10, i32, 1.0f, NP, 4, f32, i32, i32, f32, p, ws64), ASD_ERR_UNSUPPORTED);   // B*T*splits > INT32_MAX
#undef PROMPT
    }

    // ---- asd_token_stats: asd_prompt_logprobs' order with its own checks (NULL tok with K1 > 1, ld_tok, n_acc / drawn, the draft
    // length's bound on K1, inv_t_rows in place of the scalar) and the size query: asd_prompt_logprobs' byte counts
    {
        const int K1 = 9, VS = 1000, NS = 5;
        const int64_t ldr = VS, lds = static_cast<int64_t>(K1) * VS, ldk = K1 - 1;
        const size_t ws64 = asd_token_stats_workspace_bytes(B, K1, VS, BF16, ASD_MAX_SPLITS);
        const size_t ws2 = asd_token_stats_workspace_bytes(B, K1, VS, BF16, 2);
        if (ws64 % 256 != 0 || ws2 % 256 != 0 || ws2 >= ws64 || asd_token_stats_workspace_bytes(B, K1, VS, BF16, 1) != 256 ||
            asd_token_stats_workspace_bytes(0, K1, VS, BF16, 0) != 256 || asd_token_stats_workspace_bytes(B, K1, VS, 99, 0) != 256 ||
            ws64 != asd_prompt_logprobs_workspace_bytes(B, K1, VS, BF16, ASD_MAX_SPLITS) ||
            ws2 != asd_prompt_logprobs_workspace_bytes(B, K1, VS, BF16, 2)) {
            std::printf("FAIL token_stats workspace sizes %zu %zu\n", ws2, ws64);
            ++failures;
        }
#define STATS(x_, dt_, lds_, ldr_, B_, K1_, V_, tok_, ldk_, acc_, drawn_, inv_t_, rows_, N_, splits_, sid_, sval_, id_, tlp_, ws_, wsb_) \
    asd_token_stats(x_, dt_, lds_, ldr_, B_, K1_, V_, tok_, ldk_, acc_, drawn_, inv_t_, rows_, N_, splits_, sid_, sval_, id_, tlp_, ws_, wsb_, nullptr)
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, NS, 0, nullptr, f32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);   // stat_id
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, NS, 0, i32, nullptr, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);   // stat_val
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, NS, 0, i32, f32, nullptr, f32, p, ws64), ASD_ERR_INVALID_ARG);   // top_id with N > 0
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, NS, 0, i32, f32, i32, nullptr, p, ws64), ASD_ERR_INVALID_ARG);   // top_lp with N > 0
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, 0, 2, i32, f32, nullptr, nullptr, p, 0), ASD_ERR_WORKSPACE);     // N == 0 needs no table
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, i32, ldk, i32, i32, 0.0f, nullptr, NS, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);       // temperature
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, i32, ldk, i32, i32, NAN, nullptr, NS, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, i32, ldk, i32, i32, NAN, f32, NS, 2, i32, f32, i32, f32, p, 0), ASD_ERR_WORKSPACE);                 // ... which inv_t_rows replaces
        EXPECT(STATS(p, BF16, lds, ldr, -1, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, NS, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);      // negative sizes
        EXPECT(STATS(p, BF16, lds, ldr, B, -1, VS, i32, ldk, i32, i32, 1.0f, nullptr, NS, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, -1, i32, ldk, i32, i32, 1.0f, nullptr, NS, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, -1, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);
        EXPECT(STATS(nullptr, 99, 0, 0, 0, K1, VS, nullptr, 0, nullptr, nullptr, 1.0f, nullptr, 99, 99, nullptr, nullptr, nullptr, nullptr, nullptr, 0), ASD_OK);   // B == 0: nothing launched
        EXPECT(STATS(p, BF16, 0, ldr, B, 0, VS, nullptr, 0, i32, i32, 1.0f, nullptr, NS, 0, nullptr, nullptr, nullptr, nullptr, p, 0), ASD_OK);        // K1 == 0 likewise
        EXPECT(STATS(p, BF16, 0, 0, B, K1, 0, i32, ldk, i32, i32, 1.0f, nullptr, NS, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);            // V == 0
        EXPECT(STATS(p, 99, lds, ldr, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, NS, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_UNSUPPORTED);         // dtype
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, ASD_MAX_TOP_LOGPROBS + 1, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_UNSUPPORTED);   // N
        EXPECT(STATS(p, BF16, lds, ldr - 1, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, ASD_MAX_TOP_LOGPROBS + 1, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_UNSUPPORTED);   // ... before the strides
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, NS, -1, i32, f32, i32, f32, p, ws64), ASD_ERR_UNSUPPORTED);      // splits
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, NS, ASD_MAX_SPLITS + 1, i32, f32, i32, f32, p, ws64), ASD_ERR_UNSUPPORTED);
        EXPECT(STATS(p, BF16, static_cast<int64_t>(ASD_MAX_DRAFT_LEN + 2) * VS, ldr, B, ASD_MAX_DRAFT_LEN + 2, VS, i32, ASD_MAX_DRAFT_LEN + 1, i32, i32, 1.0f, nullptr, NS, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_UNSUPPORTED);   // K1 above the draft length's bound
        EXPECT(STATS(nullptr, BF16, lds, ldr, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, NS, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG); // logits
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, nullptr, ldk, i32, i32, 1.0f, nullptr, NS, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);   // tok with K1 > 1
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, i32, ldk, nullptr, i32, 1.0f, nullptr, NS, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);   // n_acc
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, i32, ldk, i32, nullptr, 1.0f, nullptr, NS, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);   // drawn
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, NS, 0, i32, f32, i32, f32, nullptr, ws64), ASD_ERR_INVALID_ARG); // workspace
        EXPECT(STATS(p, BF16, lds, ldr - 1, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, NS, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);   // ld_row < V
        EXPECT(STATS(p, BF16, lds - 1, ldr, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, NS, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);   // ld_seq < K1 ld_row
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, i32, ldk - 1, i32, i32, 1.0f, nullptr, NS, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);   // ld_tok < K1 - 1
        EXPECT(STATS(rows + 1, BF16, lds, ldr, B, K1, VS, i32, ldk - 1, i32, i32, 1.0f, nullptr, NS, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_INVALID_ARG);   // ... before alignment
        EXPECT(STATS(rows + 1, BF16, static_cast<int64_t>(K1) << 30, int64_t{1} << 30, B, K1, 1 << 30, i32, ldk, i32, i32, 1.0f, nullptr, NS, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_UNSUPPORTED);   // a 2 GiB row, before alignment
        EXPECT(STATS(rows + 1, BF16, lds, ldr, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, NS, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_ALIGNMENT);  // below the element size
        EXPECT(STATS(rows + 2, 0 /*f32*/, lds, ldr, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, NS, 0, i32, f32, i32, f32, p, ws64), ASD_ERR_ALIGNMENT);
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, NS, 0, i32, f32, i32, f32, rows + 16, ws64), ASD_ERR_WORKSPACE); // misaligned workspace
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, NS, ASD_MAX_SPLITS, i32, f32, i32, f32, p, ws64 - 1), ASD_ERR_WORKSPACE);   // too small
        EXPECT(STATS(p, BF16, lds, ldr, B, K1, VS, i32, ldk, i32, i32, 1.0f, nullptr, NS, 2, i32, f32, i32, f32, p, ws2 - 1), ASD_ERR_WORKSPACE);
        EXPECT(STATS(rows + 2, BF16, VS, ldr, B, 1, VS, nullptr, 0, i32, i32, 1.0f, nullptr, NS, 1, i32, f32, i32, f32, p, 255), ASD_ERR_WORKSPACE);   // (K1 == 1: a NULL tok and any ld_tok are valid)
        EXPECT(STATS(p, BF16, static_cast<int64_t>(ASD_MAX_DRAFT_LEN + 1) * VS, ldr, 1 << 20, ASD_MAX_DRAFT_LEN + 1, VS, i32, ASD_MAX_DRAFT_LEN, i32, i32, 1.0f, nullptr, NS, ASD_MAX_SPLITS, i32, f32, i32, f32, p, ws64), ASD_ERR_UNSUPPORTED);   // B*K1*splits > INT32_MAX
#undef STATS
    }

    std::printf(failures ? "asan_host_args: %d failure(s)\n" : "asan_host_args: ok\n", failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
