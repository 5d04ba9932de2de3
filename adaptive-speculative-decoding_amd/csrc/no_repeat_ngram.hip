// no_repeat_ngram.hip -- `no_repeat_ngram_size` ahead of the samplers (HF generate's NoRepeatNGramLogitsProcessor), gfx950: no
// n-gram of a row's history may occur twice, so every token that would complete a second copy of one is banned.
//
// logits[b][j][v] lies at b*ld_seq + j*ld_row + v (asd_bad_words_rows' addressing; bf16 / f16 / f32).  Row b has the size
// n = ngram_n[b] (or n_shared with ngram_n == NULL); the history of position j of sequence b is
//   H = tokens[b][row_start[b] .. L)  ++  step_tok[b][0 .. n_prev + j),     L = clamp(seq_len[b], start, max_len)
// -- the row's real prompt ids (row_start[b] is where they begin behind the left-padding; NULL: `start`, no prompt), its
// committed generated tokens, and behind them the step's proposals the position sees.  For every i in [0, len(H) - n] with
// H[i .. i+n-1) == H[len(H)-n+1 .. len(H)) element H[i+n-1] of the row becomes -inf.  Nothing else is written.
//
// The "words" are not a table: they are every n-gram of H, so the kernel scans H.  A workgroup of 256 lanes serves one (b, j)
// and the n-gram starts of one slice of ASD_NGRAM_SLICE (grid = (B*K1, slices); slices need no hand-off).  Every lane holds the
// n - 1 suffix tokens in registers (uniform loads), strides over the starts i of its slice, compares H[i+n-2] with the LAST
// suffix token first -- which rejects almost every candidate after one load -- then the rest, and on a match issues one
// ordinary per-lane vector-memory store of the -inf bits.  Several lanes and slices may store the same bits to one element, in
// either order the same result -- no atomics, no LDS, no workspace, nothing waits.  Damaged device data never leaves the
// arrays: seq_len[b] is clamped into [start, max_len], row_start[b] into [0, start], a row whose n lies outside 1..8 is
// skipped, a history token outside [0, V) is compared but never used as a store index.  `tokens` is only read.

#include <hip/hip_runtime.h>

#include "common.hpp"

namespace asd {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxN = ASD_MAX_NGRAM;
constexpr int kSlice = ASD_NGRAM_SLICE;          // n-gram starts per workgroup: 8 per lane
constexpr int kMaxSlices = 65535;                // gridDim.y; a longer history goes round the grid again

// the -inf bits asd_logit_edit_rows, asd_logit_mask_rows and asd_bad_words_rows write
template <int DT>
__device__ __forceinline__ void ban_one(void* logits, int64_t at) {
    if constexpr (DT == ASD_DTYPE_BF16) static_cast<uint16_t*>(logits)[at] = 0xFF80u;
    else if constexpr (DT == ASD_DTYPE_F16) static_cast<uint16_t*>(logits)[at] = 0xFC00u;
    else static_cast<float*>(logits)[at] = -INFINITY;
}

template <int DT>
__global__ __launch_bounds__(kThreads) void k_no_repeat_ngram_rows(void* logits, int64_t ld_seq, int64_t ld_row, int K1, int V,
                                                                   const int32_t* __restrict__ ngram_n, int n_shared,
                                                                   const int32_t* __restrict__ row_start,
                                                                   const int32_t* __restrict__ tokens, int64_t ld_tokens,
                                                                   const int32_t* __restrict__ seq_len, int start, int max_len,
                                                                   const int32_t* __restrict__ step_tok, int64_t ld_tok,
                                                                   int n_prev) {
    const int row = static_cast<int>(blockIdx.x);
    const int b = static_cast<int>(static_cast<uint32_t>(row) / static_cast<uint32_t>(K1));
    const int j = row - b * K1;
    const int n = ngram_n ? ngram_n[b] : n_shared;
    if (n < 1 || n > kMaxN) return;                      // 0: the row is off; anything else outside 1..8: damaged, skipped
    int L = seq_len[b];
    L = L < start ? start : (L > max_len ? max_len : L); // start <= max_len <= ld_tokens: the launcher's checks
    int first = start;
    if (row_start) {
        first = row_start[b];
        first = first < 0 ? 0 : (first > start ? start : first);
    }
    const int n_com = L - first;                         // real prompt ids and committed generated tokens: one run of `tokens`
    const int n_see = step_tok ? n_prev + j : 0;         // proposals this position sees; n_prev + K1 - 1 <= n_tok: the launcher's
    const int len = n_com + n_see;                       // <= max_len + n_tok < 2^31 - kThreads: the launcher's
    const int n_starts = len - n + 1;                    // n-grams of H; <= 0: a history shorter than n bans nothing
    const int32_t* const committed = tokens + static_cast<int64_t>(b) * ld_tokens + first;
    const int64_t proposed = static_cast<int64_t>(b) * ld_tok - n_com;     // step_tok's index of H[p], for p >= n_com
    // H[p] for 0 <= p < len, piecewise: an n-gram may lie in `tokens`, in `step_tok`, or across both
    auto hist = [&](int p) -> int { return p < n_com ? committed[p] : step_tok[proposed + p]; };
    int suf[kMaxN - 1];                                  // suf[k] = H[len - (n-1) + k], k < n - 1 (the same in every lane)
    if (n_starts > 0) {
#pragma unroll
        for (int k = 0; k < kMaxN - 1; ++k) suf[k] = k < n - 1 ? hist(len - (n - 1) + k) : 0;
    }
    const int last = (n >= 2 && n_starts > 0) ? hist(len - 1) : 0;         // suf[n-2], without a dynamic register index
    const int64_t out = static_cast<int64_t>(b) * ld_seq + static_cast<int64_t>(j) * ld_row;
    for (int64_t s0 = static_cast<int64_t>(blockIdx.y) * kSlice; s0 < n_starts; s0 += static_cast<int64_t>(gridDim.y) * kSlice) {
        const int i0 = static_cast<int>(s0);
        const int i1 = n_starts - i0 > kSlice ? i0 + kSlice : n_starts;
        for (int i = i0 + static_cast<int>(threadIdx.x); i < i1; i += kThreads) {
            bool match = n < 2 || hist(i + n - 2) == last;
            if (!match) continue;
#pragma unroll
            for (int k = 0; k < kMaxN - 2; ++k) {
                if (k < n - 2) match &= hist(i + k) == suf[k];
            }
            if (!match) continue;
            const int t = hist(i + n - 1);               // i + n - 1 <= len - 1
            if (t >= 0 && t < V) ban_one<DT>(logits, out + t);             // a history token outside [0, V) is never an index
        }
    }
}

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT int asd_no_repeat_ngram_rows(void* logits, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V,
                                        const int32_t* ngram_n, int n_shared, const int32_t* row_start, const int32_t* tokens,
                                        int64_t ld_tokens, const int32_t* seq_len, int start, int max_len, const int32_t* step_tok,
                                        int64_t ld_tok, int n_tok, int n_prev, void* stream) {
    if (B < 0 || K1 < 0 || V < 0 || n_shared < 0 || n_tok < 0 || n_prev < 0 || start < 0 || max_len < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0 || K1 == 0 || V == 0 || (!ngram_n && n_shared == 0)) return ASD_OK;
    const int esz = dtype_size(dtype);
    if (esz == 0) return ASD_ERR_UNSUPPORTED;
    if (!ngram_n && n_shared > ASD_MAX_NGRAM) return ASD_ERR_UNSUPPORTED;
    if (n_tok > ASD_MAX_DRAFT_LEN) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(B) * K1 > INT32_MAX) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(max_len) + n_tok > INT32_MAX - kThreads) return ASD_ERR_UNSUPPORTED;   // the scan counts in int32
    if (!logits || !tokens || !seq_len) return ASD_ERR_INVALID_ARG;
    if (ld_row < V || ld_seq < static_cast<int64_t>(K1) * ld_row || ld_tokens < max_len || start > max_len) return ASD_ERR_INVALID_ARG;
    if (!step_tok && n_prev != 0) return ASD_ERR_INVALID_ARG;
    if (step_tok && (static_cast<int64_t>(n_prev) + K1 - 1 > n_tok || ld_tok < n_tok)) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(logits, static_cast<size_t>(esz)) || !aligned_to(ngram_n, 4) || !aligned_to(row_start, 4) || !aligned_to(tokens, 4) ||
        !aligned_to(seq_len, 4) || !aligned_to(step_tok, 4))
        return ASD_ERR_ALIGNMENT;
    // no position's history is longer than max_len + n_tok: a long context is spread over slices, not walked by one workgroup
    const int64_t slices = (static_cast<int64_t>(max_len) + n_tok + kSlice - 1) / kSlice;
    const dim3 grid(static_cast<uint32_t>(static_cast<int64_t>(B) * K1),
                    static_cast<uint32_t>(slices < 1 ? 1 : (slices > kMaxSlices ? kMaxSlices : slices)));
    dispatch_dtype(dtype, [&](auto dt) {
        hipLaunchKernelGGL((k_no_repeat_ngram_rows<decltype(dt)::value>), grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                           logits, ld_seq, ld_row, K1, V, ngram_n, n_shared, row_start, tokens, ld_tokens, seq_len, start, max_len,
                           step_tok, ld_tok, n_prev);
    });
    return launch_status();
}
