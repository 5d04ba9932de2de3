// lookup.hip -- prompt-lookup drafting (HF generate's `prompt_lookup_num_tokens`, vLLM's `ngram` method), gfx950 / wave64: the
// proposals of a speculative step without a draft model.  The last tokens of a row are searched earlier in the row's own
// prompt and output, and what followed them there is proposed.
//
// Row b has the history H = tokens[b][row_start[b] .. L), L = clamp(seq_len[b], start, max_len), row_start[b] clamped into
// [0, start] (NULL: start) -- asd_no_repeat_ngram_rows' history without proposals: the real prompt ids, then the committed
// tokens.  With len = |H|, N = max_ngram, n0 = min_ngram, every e in [1, len - 1] has the match length
//     m(e) = the number of k = 0, 1, .. < min(e, N) with H[e-1-k] == H[len-1-k], counted until the first failure,
// and the winner e* maximises (m(e), e): the longest match, then the most recent.  It is valid when m(e*) >= n0.  Then, with
// p = len - e*, proposal i is H[e* + (i mod p)] for i < K (an overlapping copy: a loop of period p is proposed whole);
// otherwise every proposal is H[len-1], or 0 when len == 0.  matched[b] = m(e*), or 0 without a valid winner.
//
// ONE WORKGROUP OF 1024 LANES PER ROW, no workspace, nothing shared between workgroups.
//   The scan reads the history STRAIGHT FROM L2 in 16-byte vectors; there is no LDS tile.  A lane owns four adjacent
//   candidates: the vector at an address that is a multiple of 16 bytes holds the tokens H[e-1] of its four e.  It compares
//   them with the last token of the row first -- almost every position ends there -- and only a lane with a hit loads the two
//   vectors in front of its own (the halo of N - 1 <= 7 tokens), which its neighbour lane has just pulled through the same
//   cache lines, and walks backwards in registers against the N suffix tokens every lane holds (uniform loads).  Why not LDS
//   tiles (dry.hip's way): a tile would be written once and read once per position -- the walk is rare -- so LDS would add a
//   store, a barrier per tile and a second read to a pass that is one load and one compare per four positions; the halo is 28
//   bytes against a 16 KB tile, and the only reuse there is, the neighbour's vector, is served by the vector cache.  A vector
//   that would reach outside [row_start, L) is replaced by guarded scalar loads: nothing outside the row's history is read,
//   whatever the alignment of the row.
//   A lane's running best is one 64-bit key (m << 32) | e, kept in registers across the tiles of ASD_LOOKUP_TILE candidates
//   (four per lane) a long history takes; the keys are reduced by a cross-lane max inside each wave and once across the 16
//   waves through LDS (16 keys, one barrier).
//   Lanes 0 .. K-1 then write the proposals by the closed form above; lane 0 writes matched[b] and adds matched > 0 to
//   counter[b] when a counter is given.
// THE ONE-HOT DRAFT ROWS, kept sparsely by the same launch: with `onehot` given ([B, K, V] in the logits' dtype, element
// (b, i, v) at b*ld_seq + i*ld_row + v), lane i reads old = tok[b][i] BEFORE it writes the new proposal, stores -inf at
// (b, i, old) when old is in [0, V), then 0 at (b, i, new) when new is in [0, V).  The caller fills `onehot` with -inf and `tok`
// with -1 once; every later step costs 2 B K element stores instead of a B K V rewrite, and softmax of such a row is exactly
// the one-hot distribution of the proposal, which the residual kernels take as any other draft row.
// Damaged device data never leaves the arrays: seq_len and row_start are clamped, a token outside [0, V) is compared and
// proposed as a plain integer but never used as a store index.  `tokens` is only read.

#include <hip/hip_runtime.h>

#include "common.hpp"

namespace asd {
namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxN = ASD_MAX_LOOKUP_NGRAM;
constexpr int kMaxK = ASD_MAX_LOOKUP_TOKENS;
constexpr int kTile = ASD_LOOKUP_TILE;           // candidates per pass of the workgroup: four per lane

static_assert(kTile == 4 * kThreads, "a lane owns one 16-byte vector of a tile");
static_assert(kMaxN == 8, "the halo is two vectors: N - 1 <= 7 tokens in front of a lane's own");
static_assert(kMaxK <= 64, "the proposals are written by one wave");

// row[q .. q+4) where the vector lies inside [lo, hi): one 16-byte load (row + q is 16-byte aligned: the caller's grid);
// elsewhere guarded scalar loads, 0 for an index outside [lo, hi) -- such a value is never compared (the walk's bound)
__device__ __forceinline__ int4 load4(const int32_t* __restrict__ row, int q, int lo, int hi) {
    if (q >= lo && q + 4 <= hi) return *reinterpret_cast<const int4*>(row + q);
    int4 v;
    v.x = (q + 0 >= lo && q + 0 < hi) ? row[q + 0] : 0;
    v.y = (q + 1 >= lo && q + 1 < hi) ? row[q + 1] : 0;
    v.z = (q + 2 >= lo && q + 2 < hi) ? row[q + 2] : 0;
    v.w = (q + 3 >= lo && q + 3 < hi) ? row[q + 3] : 0;
    return v;
}

template <int DT>
__device__ __forceinline__ void put(void* p, int64_t at, bool zero) {
    if constexpr (DT == ASD_DTYPE_BF16) static_cast<uint16_t*>(p)[at] = zero ? uint16_t(0) : uint16_t(0xFF80u);
    else if constexpr (DT == ASD_DTYPE_F16) static_cast<uint16_t*>(p)[at] = zero ? uint16_t(0) : uint16_t(0xFC00u);
    else static_cast<float*>(p)[at] = zero ? 0.0f : -INFINITY;
}

// DT < 0: no one-hot rows (greedy decoding)
template <int DT>
__global__ __launch_bounds__(kThreads) void k_lookup_propose(const int32_t* __restrict__ tokens, int64_t ld_tokens,
                                                             const int32_t* __restrict__ row_start,
                                                             const int32_t* __restrict__ seq_len, int start, int max_len, int K,
                                                             int N, int n0, int32_t* __restrict__ tok, int64_t ld_tok,
                                                             int32_t* __restrict__ matched, int32_t* __restrict__ counter,
                                                             void* onehot, int64_t ld_seq, int64_t ld_row, int V) {
    __shared__ unsigned long long s_best[kWaves];

    const int tid = static_cast<int>(threadIdx.x);
    const int b = static_cast<int>(blockIdx.x);
    int L = seq_len[b];
    L = L < start ? start : (L > max_len ? max_len : L);     // start <= max_len <= ld_tokens: the launcher's checks
    int first = start;
    if (row_start) {
        first = row_start[b];
        first = first < 0 ? 0 : (first > start ? start : first);
    }
    const int len = L - first;                               // |H|; every index below lies in [first, L)
    const int32_t* const row = tokens + static_cast<int64_t>(b) * ld_tokens;

    // suf[k] = H[len-1-k] for k < min(N, len): uniform loads, the same registers in every lane
    int suf[kMaxN];
#pragma unroll
    for (int k = 0; k < kMaxN; ++k) suf[k] = (k < N && k < len) ? row[L - 1 - k] : 0;

    // candidate e in [1, len-1] <-> the index c = first + e - 1 of H[e-1] in the row, c in [first, L-2].  Lanes take vectors on
    // the grid of 16-byte aligned addresses: the first one may begin up to three elements in front of `first`.
    const int mis = static_cast<int>((reinterpret_cast<uintptr_t>(row) >> 2) & 3u);
    const int q_base = first - ((first + mis) & 3);          // >= -3; row + q_base is 16-byte aligned
    unsigned long long best = 0;                             // (m << 32) | e; 0: no candidate matches its last token
    for (int q = q_base + 4 * tid; q <= L - 2; q += kTile) {                  // q + kTile < 2^31: the launcher's check
        const int4 own = load4(row, q, first, L);
        int w[12];                                           // w[8 + j] = row[q + j]; w[0 .. 8) = row[q-8 .. q): the halo
        w[8] = own.x, w[9] = own.y, w[10] = own.z, w[11] = own.w;
        bool hit = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) hit |= q + j >= first && q + j <= L - 2 && w[8 + j] == suf[0];
        if (!hit) continue;
        if (N > 1) {                                         // only a hit walks backwards: the two vectors in front
            const int4 h1 = load4(row, q - 4, first, L), h0 = load4(row, q - 8, first, L);
            w[0] = h0.x, w[1] = h0.y, w[2] = h0.z, w[3] = h0.w;
            w[4] = h1.x, w[5] = h1.y, w[6] = h1.z, w[7] = h1.w;
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) w[k] = 0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = q + j;
            if (c < first || c > L - 2 || w[8 + j] != suf[0]) continue;
            const int e = c - first + 1;
            const int lim = e < N ? e : N;                   // k < min(e, N): the walk never leaves H, nor meets the suffix itself
            int m = 1;
            bool run = true;
#pragma unroll
            for (int k = 1; k < kMaxN; ++k) {
                run = run && k < lim && w[8 + j - k] == suf[k];
                m += run ? 1 : 0;
            }
            const unsigned long long key = (static_cast<unsigned long long>(m) << 32) | static_cast<uint32_t>(e);
            best = key > best ? key : best;
        }
    }
    // the maximum inside each wave, then once across the 16 waves through LDS
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long other = __shfl_xor(best, d, 64);
        best = other > best ? other : best;
    }
    if ((tid & 63) == 0) s_best[tid >> 6] = best;
    __syncthreads();
    if (tid >= kMaxK) return;                                // the outputs: wave 0's first lanes
#pragma unroll
    for (int wv = 0; wv < kWaves; ++wv) best = s_best[wv] > best ? s_best[wv] : best;
    const int m_win = static_cast<int>(best >> 32);
    const int e_win = static_cast<int>(best & 0xFFFFFFFFull);                 // in [1, len-1] where m_win >= 1
    const bool valid = m_win >= n0;                          // n0 >= 1: never with best == 0
    if (tid < K) {
        int t = len > 0 ? row[L - 1] : 0;
        if (valid) {
            const int p = len - e_win;                       // >= 1
            t = row[first + e_win + tid % p];                // e* + (i mod p) <= len - 1
        }
        int32_t* const slot = tok + static_cast<int64_t>(b) * ld_tok + tid;
        if constexpr (DT >= 0) {
            const int old = *slot;
            const int64_t at = static_cast<int64_t>(b) * ld_seq + static_cast<int64_t>(tid) * ld_row;
            if (old >= 0 && old < V) put<DT>(onehot, at + old, false);
            if (t >= 0 && t < V) put<DT>(onehot, at + t, true);
        }
        *slot = t;
    }
    if (tid == 0) {
        matched[b] = valid ? m_win : 0;
        if (counter) counter[b] += valid ? 1 : 0;
    }
}

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT int asd_lookup_propose(const int32_t* tokens, int64_t ld_tokens, const int32_t* row_start, const int32_t* seq_len, int B,
                                  int start, int max_len, int K, int max_ngram, int min_ngram, int32_t* tok, int64_t ld_tok,
                                  int32_t* matched, int32_t* counter, void* onehot, int dtype, int64_t ld_seq, int64_t ld_row, int V,
                                  void* stream) {
    if (B < 0 || start < 0 || max_len < 0 || V < 0 || K < 1 || max_ngram < 1 || min_ngram < 1 || min_ngram > max_ngram)
        return ASD_ERR_INVALID_ARG;
    if (B == 0) return ASD_OK;
    if (K > kMaxK || max_ngram > kMaxN) return ASD_ERR_UNSUPPORTED;
    const int esz = onehot ? dtype_size(dtype) : 4;
    if (esz == 0) return ASD_ERR_UNSUPPORTED;
    if (max_len > INT32_MAX - 2 * kTile) return ASD_ERR_UNSUPPORTED;          // the scan counts in int32, a tile at a time
    if (!tokens || !seq_len || !tok || !matched) return ASD_ERR_INVALID_ARG;
    if (ld_tokens < max_len || start > max_len || ld_tok < K) return ASD_ERR_INVALID_ARG;
    if (onehot && (V < 1 || ld_row < V || ld_seq < static_cast<int64_t>(K) * ld_row)) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(tokens, 4) || !aligned_to(row_start, 4) || !aligned_to(seq_len, 4) || !aligned_to(tok, 4) ||
        !aligned_to(matched, 4) || !aligned_to(counter, 4) || !aligned_to(onehot, static_cast<size_t>(esz)))
        return ASD_ERR_ALIGNMENT;
    const dim3 grid(static_cast<uint32_t>(B));
    auto launch = [&](auto dt) {
        hipLaunchKernelGGL((k_lookup_propose<decltype(dt)::value>), grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), tokens,
                           ld_tokens, row_start, seq_len, start, max_len, K, max_ngram, min_ngram, tok, ld_tok, matched, counter,
                           onehot, ld_seq, ld_row, V);
    };
    if (onehot) dispatch_dtype(dtype, launch);
    else launch(std::integral_constant<int, -1>{});
    return launch_status();
}
