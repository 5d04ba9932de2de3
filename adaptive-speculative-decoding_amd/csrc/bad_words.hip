// bad_words.hip -- multi-token banned words ahead of the samplers (vLLM's `bad_words`, on token ids), gfx950: a word
// w_0 .. w_{m-1} bans its LAST token at a position whose history ends in w_0 .. w_{m-2}.
//
// logits[b][j][v] lies at b*ld_seq + j*ld_row + v (asd_logit_edit_rows' addressing; bf16 / f16 / f32).  Row b owns the words
// [row_first[b], row_first[b+1]) of the tables word_tok [n, ASD_MAX_BAD_WORD_LEN] / word_n [n] (pack_stop_sequences' layout) --
// or, with row_first == NULL, the words [0, n) like every other row.  The history of position j of sequence b is
//   H = tokens[b][start .. seq_len[b])  ++  step_tok[b][0 .. n_prev + j)
// -- the row's committed GENERATED tokens (the prompt in front of `start` is not history) and behind them the step's proposals
// the position sees, which are not committed yet.  Element w_{m-1} of the row becomes -inf when len(H) >= m - 1 and the last
// m - 1 tokens of H equal w_0 .. w_{m-2}; a word of one token always bans it.  Nothing else is written.
//
// One workgroup per (b, j), lane t handles word t of the row: at most seven history loads, independent of each other, and one
// store.  Two words of a row may end in one id: both lanes then store the same -inf bits to one element with ordinary per-lane
// vector-memory stores, in either order the same result -- no atomics, no LDS, nothing waits.  Damaged device data never
// leaves the arrays: seq_len[b] is clamped into [start, max_len], word indices into [0, n), a word whose length lies outside
// 1..8 or whose last id lies outside [0, V) is skipped, and prefix ids and proposals are only compared.

#include <hip/hip_runtime.h>

#include "common.hpp"

namespace asd {
namespace {

constexpr int kThreads = ASD_MAX_BAD_WORDS;      // one word per lane
constexpr int kMaxLen = ASD_MAX_BAD_WORD_LEN;

// the -inf bits asd_logit_edit_rows and asd_logit_mask_rows write
template <int DT>
__device__ __forceinline__ void ban_one(void* logits, int64_t at) {
    if constexpr (DT == ASD_DTYPE_BF16) static_cast<uint16_t*>(logits)[at] = 0xFF80u;
    else if constexpr (DT == ASD_DTYPE_F16) static_cast<uint16_t*>(logits)[at] = 0xFC00u;
    else static_cast<float*>(logits)[at] = -INFINITY;
}

template <int DT>
__global__ __launch_bounds__(kThreads) void k_bad_words_rows(void* logits, int64_t ld_seq, int64_t ld_row, int K1, int V,
                                                             const int32_t* __restrict__ word_tok,
                                                             const int32_t* __restrict__ word_n,
                                                             const int32_t* __restrict__ row_first, int n,
                                                             const int32_t* __restrict__ tokens, int64_t ld_tokens,
                                                             const int32_t* __restrict__ seq_len, int start, int max_len,
                                                             const int32_t* __restrict__ step_tok, int64_t ld_tok, int n_prev) {
    const int row = static_cast<int>(blockIdx.x);
    const int b = static_cast<int>(static_cast<uint32_t>(row) / static_cast<uint32_t>(K1));
    const int j = row - b * K1;
    // the row's words: [first, first + n_own) of the n uploaded ones, at most ASD_MAX_BAD_WORDS, never outside the tables
    int first = 0, n_own = n;
    if (row_first) {
        first = row_first[b];
        n_own = row_first[b + 1] - first;
    }
    if (first < 0 || first > n) n_own = 0;
    n_own = n_own > n - first ? n - first : n_own;
    n_own = n_own < 0 ? 0 : (n_own > ASD_MAX_BAD_WORDS ? ASD_MAX_BAD_WORDS : n_own);
    const int t = static_cast<int>(threadIdx.x);
    if (t >= n_own) return;
    const int32_t* const w = word_tok + static_cast<int64_t>(first + t) * kMaxLen;
    const int m = word_n[first + t];
    if (m < 1 || m > kMaxLen) return;                    // the launcher cannot check device data: skipped
    const int last = w[m - 1];
    if (last < 0 || last >= V) return;                   // never written
    int L = seq_len[b];
    L = L < start ? start : (L > max_len ? max_len : L); // start <= max_len <= ld_tokens: the launcher's checks
    const int n_gen = L - start;                         // committed generated tokens
    const int n_see = step_tok ? n_prev + j : 0;         // proposals this position sees; n_prev + K1 - 1 <= n_tok: the launcher's
    const int at0 = n_gen + n_see - (m - 1);             // where in H the prefix would begin
    if (at0 < 0) return;                                 // a history shorter than the prefix
    const int32_t* const committed = tokens + static_cast<int64_t>(b) * ld_tokens + start;
    const int64_t proposed = static_cast<int64_t>(b) * ld_tok - n_gen;     // step_tok's index of H[p], for p >= n_gen
    bool match = true;
#pragma unroll
    for (int i = 0; i < kMaxLen - 1; ++i) {
        if (i < m - 1) {
            const int p = at0 + i;                       // 0 <= p < n_gen + n_see
            const int h = p < n_gen ? committed[p] : step_tok[proposed + p];
            match &= h == w[i];
        }
    }
    if (match) ban_one<DT>(logits, static_cast<int64_t>(b) * ld_seq + static_cast<int64_t>(j) * ld_row + last);
}

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT int asd_bad_words_rows(void* logits, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V,
                                  const int32_t* word_tok, const int32_t* word_n, const int32_t* row_first, int n_shared,
                                  const int32_t* tokens, int64_t ld_tokens, const int32_t* seq_len, int start, int max_len,
                                  const int32_t* step_tok, int64_t ld_tok, int n_tok, int n_prev, void* stream) {
    if (B < 0 || K1 < 0 || V < 0 || n_shared < 0 || n_tok < 0 || n_prev < 0 || start < 0 || max_len < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0 || K1 == 0 || V == 0 || n_shared == 0) return ASD_OK;
    const int esz = dtype_size(dtype);
    if (esz == 0) return ASD_ERR_UNSUPPORTED;
    if (!row_first && n_shared > ASD_MAX_BAD_WORDS) return ASD_ERR_UNSUPPORTED;
    if (n_tok > ASD_MAX_DRAFT_LEN) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(B) * K1 > INT32_MAX) return ASD_ERR_UNSUPPORTED;
    if (!logits || !word_tok || !word_n || !tokens || !seq_len) return ASD_ERR_INVALID_ARG;
    if (ld_row < V || ld_seq < static_cast<int64_t>(K1) * ld_row || ld_tokens < max_len || start > max_len) return ASD_ERR_INVALID_ARG;
    if (!step_tok && n_prev != 0) return ASD_ERR_INVALID_ARG;
    if (step_tok && (static_cast<int64_t>(n_prev) + K1 - 1 > n_tok || ld_tok < n_tok)) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(logits, static_cast<size_t>(esz)) || !aligned_to(word_tok, 4) || !aligned_to(word_n, 4) || !aligned_to(row_first, 4) ||
        !aligned_to(tokens, 4) || !aligned_to(seq_len, 4) || !aligned_to(step_tok, 4))
        return ASD_ERR_ALIGNMENT;
    const dim3 grid(static_cast<uint32_t>(static_cast<int64_t>(B) * K1));
    dispatch_dtype(dtype, [&](auto dt) {
        hipLaunchKernelGGL((k_bad_words_rows<decltype(dt)::value>), grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), logits,
                           ld_seq, ld_row, K1, V, word_tok, word_n, row_first, n_shared, tokens, ld_tokens, seq_len, start, max_len,
                           step_tok, ld_tok, n_prev);
    });
    return launch_status();
}
