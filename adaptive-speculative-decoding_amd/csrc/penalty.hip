// penalty.hip -- the stateful penalties ahead of the samplers (vLLM's `apply_penalties`: repetition_penalty, presence_penalty,
// frequency_penalty), gfx950: asd_penalty_rows edits the logits in place from a per-row history, asd_penalty_commit adds a
// step's committed tokens to that history.
//
// STATE, per sequence b: seen[b] is W = (V + 31) / 32 mask words in asd_logit_mask_rows' layout -- bit v & 31 of word v >> 5 SET
// when token v occurs in the row's prompt or among its committed generated tokens -- and counts[b][v] is the number of
// occurrences of v among the committed generated tokens (the prompt is not counted).  counts[b][v] > 0 implies the bit: only
// asd_penalty_commit writes either, and it writes both.  params[b] = (rep, pres, freq).
//
// asd_penalty_rows.  logits[b][j][v] lies at b*ld_seq + j*ld_row + v (asd_logit_edit_rows' addressing).  Position j of
// sequence b has the history: the state, and the step's proposals step_tok[b][0 .. n_prev + j) -- not committed yet, kept in no
// state, so a rejected proposal leaves no trace.  Token v is SEEN at (b, j) when its bit is set or it is among those proposals;
// c is counts[b][v] plus its occurrences among them.  In f32, in this order, one rounding to the dtype at the end (this file
// is compiled with -ffp-contract=off: no multiply-add is fused; the division is the correctly rounded one):
//     y = x
//     if seen and rep != 1:   y = x > 0 ? x / rep : x * rep
//     if c > 0:               y = y - freq * (float)c;   y = y - pres
// Nothing is stored where y == x (so -inf stays -inf, and an unseen element keeps its bits); a result that rounds to +inf is
// stored as the dtype's largest finite value (the samplers forbid +inf).
//
// Geometry: grid B x S.  A row's W mask words are cut into S slices of whole words; the workgroup (b, s) owns the elements of
// its slice's words at ALL K1 positions, so the cost follows the number of distinct seen tokens: a lane reads one word per
// round (the scan is 19 KB per row at V = 152064) and works only on its set bits.
// Ownership, which makes every element the business of at most one lane of one workgroup in a launch (no atomics; every
// access an ordinary per-lane vector-memory load or store):
//   * a SET bit belongs to the lane that scans its word: it gathers counts[b][v], counts v among the proposals (an LDS copy of
//     the at most 64 ids) position by position, and edits element v of each of the K1 positions;
//   * a proposal whose bit is CLEAR belongs to the workgroup whose slice holds its word, and there to the lane of its first
//     occurrence t in step_tok[b][:]: that lane edits the positions j with n_prev + j > t, the ones that see it.
// The result does not depend on S: nothing is reduced, and no element has two owners whatever the cut.
//
// asd_penalty_commit.  One workgroup per sequence behind the step's commit kernel: the n_commit[b] tokens at
// tokens[b][seq_len[b] - n_commit[b] .. seq_len[b]) enter the state.  A step may commit one token twice: lane i owns token i
// only when no earlier lane holds the same id, and adds the id's multiplicity within the step to counts (a plain load and
// store); two ids may share a mask word: the bit is set with a per-lane vector atomic OR.

#include <hip/hip_runtime.h>

#include "common.hpp"

namespace asd {
namespace {

constexpr int kThreads = 256;            // asd_penalty_rows: one mask word per lane and round
constexpr int kSliceWords = kThreads;    // words per slice: whole rounds of the workgroup (8192 tokens)
constexpr int kMaxTok = ASD_MAX_DRAFT_LEN;       // proposals a launch may see: the LDS copy
constexpr int kCommitThreads = 128;      // asd_penalty_commit: one candidate per lane, at most ASD_MAX_DRAFT_LEN + 1
constexpr int kMaxCommit = ASD_MAX_DRAFT_LEN + 1;

// round to nearest even, the conversion of torch's .to(bfloat16) (logit_edit.hip's); a NaN stays a (quiet) NaN
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return static_cast<uint16_t>((u >> 16) | 0x0040u);
    return static_cast<uint16_t>((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

struct RowParams {
    float rep, pres, freq;
};

// the arithmetic of the header, on one element
__device__ __forceinline__ float penalised(float x, const RowParams& p, bool seen, int c) {
    float y = x;
    if (seen && p.rep != 1.0f) y = x > 0.0f ? x / p.rep : x * p.rep;
    if (c > 0) {
        y = y - p.freq * static_cast<float>(c);
        y = y - p.pres;
    }
    return y;
}

template <int DT>
__device__ __forceinline__ void penalise_one(void* logits, int64_t at, const RowParams& p, bool seen, int c) {
    if constexpr (DT == ASD_DTYPE_BF16) {
        uint16_t* const q = static_cast<uint16_t*>(logits) + at;
        const float x = __uint_as_float(static_cast<uint32_t>(*q) << 16);
        const float y = penalised(x, p, seen, c);
        if (y == x) return;
        const uint16_t r = f32_to_bf16(y);
        *q = r == 0x7F80u ? static_cast<uint16_t>(0x7F7Fu) : r;
    } else if constexpr (DT == ASD_DTYPE_F16) {
        _Float16* const q = static_cast<_Float16*>(logits) + at;
        const float x = static_cast<float>(*q);
        const float y = penalised(x, p, seen, c);
        if (y == x) return;
        const uint16_t r = __builtin_bit_cast(uint16_t, static_cast<_Float16>(y));       // v_cvt_f16_f32: to nearest even
        *q = __builtin_bit_cast(_Float16, r == 0x7C00u ? static_cast<uint16_t>(0x7BFFu) : r);
    } else {
        float* const q = static_cast<float*>(logits) + at;
        const float x = *q;
        const float y = penalised(x, p, seen, c);
        if (y == x) return;
        *q = y == INFINITY ? 3.402823466e+38f : y;
    }
}

template <int DT>
__global__ __launch_bounds__(kThreads) void k_penalty_rows(void* logits, int64_t ld_seq, int64_t ld_row, int K1, int V,
                                                           const uint32_t* __restrict__ seen,
                                                           const int32_t* __restrict__ counts,
                                                           const float* __restrict__ params,
                                                           const int32_t* __restrict__ step_tok, int64_t ld_tok, int n_prev,
                                                           int words_per_slice) {
    __shared__ int32_t s_tok[kMaxTok];
    const int b = static_cast<int>(blockIdx.x);
    const int tid = static_cast<int>(threadIdx.x);
    RowParams p{params[3 * b], params[3 * b + 1], params[3 * b + 2]};
    if (!(p.rep > 0.0f)) p.rep = 1.0f;                              // <= 0 or NaN: no repetition penalty
    if (p.rep == 1.0f && p.pres == 0.0f && p.freq == 0.0f) return;  // a neutral row (uniform over the workgroup)
    const int W = static_cast<int>((static_cast<int64_t>(V) + 31) >> 5);
    const int64_t w0 = static_cast<int64_t>(blockIdx.y) * words_per_slice;
    if (w0 >= W) return;
    const int64_t w1 = w0 + words_per_slice < W ? w0 + words_per_slice : W;
    // the proposals the LAST position sees; the launcher has checked n_prev + K1 - 1 <= n_tok <= kMaxTok
    int n_see = step_tok ? n_prev + K1 - 1 : 0;
    n_see = n_see < 0 ? 0 : (n_see > kMaxTok ? kMaxTok : n_see);
    if (tid < n_see) s_tok[tid] = step_tok[static_cast<int64_t>(b) * ld_tok + tid];
    __syncthreads();
    const int n_first = n_prev < n_see ? n_prev : n_see;            // the proposals position 0 sees

    const uint32_t* const bits = seen + static_cast<int64_t>(b) * W;
    const int32_t* const cnt = counts + static_cast<int64_t>(b) * V;
    const int64_t base = static_cast<int64_t>(b) * ld_seq;

    // ---- the set bits of the slice: the lane that scans a word owns its tokens at every position
    for (int64_t w = w0 + tid; w < w1; w += kThreads) {
        uint32_t word = bits[w];
        if (w == W - 1 && (V & 31)) word &= (1u << (V & 31)) - 1u;   // bits at v >= V are never looked at
        while (word) {
            const int bit = __ffs(word) - 1;
            word &= word - 1u;
            const int v = static_cast<int>(w << 5) + bit;
            int c = cnt[v];
            for (int t = 0; t < n_first; ++t) c += s_tok[t] == v;
            for (int j = 0; j < K1; ++j) {
                if (j > 0 && n_prev + j - 1 < n_see) c += s_tok[n_prev + j - 1] == v;
                penalise_one<DT>(logits, base + static_cast<int64_t>(j) * ld_row + v, p, true, c);
            }
        }
    }

    // ---- the proposals whose bit is clear: lane t owns proposal t when it is the id's first occurrence and this slice holds it
    if (tid < n_see) {
        const int v = s_tok[tid];
        if (v < 0 || v >= V) return;                                 // never written
        const int64_t w = v >> 5;
        if (w < w0 || w >= w1) return;                               // another workgroup's
        if ((bits[w] >> (v & 31)) & 1u) return;                      // seen already: the scan's
        for (int t = 0; t < tid; ++t)
            if (s_tok[t] == v) return;                               // an earlier lane's
        // positions that see proposal tid: n_prev + j > tid
        int j0 = tid - n_prev + 1;
        j0 = j0 < 0 ? 0 : j0;
        int c = cnt[v];
        for (int t = 0; t < n_prev + j0 && t < n_see; ++t) c += s_tok[t] == v;
        for (int j = j0; j < K1; ++j) {
            if (j > j0 && n_prev + j - 1 < n_see) c += s_tok[n_prev + j - 1] == v;
            penalise_one<DT>(logits, base + static_cast<int64_t>(j) * ld_row + v, p, true, c);
        }
    }
}

__global__ __launch_bounds__(kCommitThreads) void k_penalty_commit(const int32_t* __restrict__ tokens, int64_t ld_tokens,
                                                                   const int32_t* __restrict__ seq_len,
                                                                   const int32_t* __restrict__ n_commit, int V, int max_len,
                                                                   uint32_t* seen, int32_t* counts) {
    __shared__ int32_t s_tok[kCommitThreads];
    const int b = static_cast<int>(blockIdx.x);
    const int tid = static_cast<int>(threadIdx.x);
    int n = n_commit[b];
    n = n < 0 ? 0 : (n > kMaxCommit ? kMaxCommit : n);              // 0 for a finished row: its state is frozen
    if (n == 0) return;
    const int64_t first = static_cast<int64_t>(seq_len[b]) - n;
    if (tid < n) {
        int64_t pos = first + tid;
        pos = pos < 0 ? 0 : (pos >= max_len ? max_len - 1 : pos);    // never outside the row
        s_tok[tid] = tokens[static_cast<int64_t>(b) * ld_tokens + pos];
    }
    __syncthreads();
    if (tid >= n) return;
    const int v = s_tok[tid];
    if (v < 0 || v >= V) return;
    int mult = 0;
    for (int t = 0; t < n; ++t) {
        if (s_tok[t] != v) continue;
        if (t < tid) return;                                         // an earlier lane owns this id
        ++mult;
    }
    const int W = static_cast<int>((static_cast<int64_t>(V) + 31) >> 5);
    int32_t* const c = counts + static_cast<int64_t>(b) * V + v;
    *c = *c + mult;
    atomicOr(seen + static_cast<int64_t>(b) * W + (v >> 5), 1u << (v & 31));
}

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT int asd_penalty_rows(void* logits, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V,
                                const uint32_t* seen, const int32_t* counts, const float* params, const int32_t* step_tok,
                                int64_t ld_tok, int n_tok, int n_prev, void* stream) {
    if (B < 0 || K1 < 0 || V < 0 || n_tok < 0 || n_prev < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0 || K1 == 0 || V == 0) return ASD_OK;
    const int esz = dtype_size(dtype);
    if (esz == 0) return ASD_ERR_UNSUPPORTED;
    if (n_tok > kMaxTok) return ASD_ERR_UNSUPPORTED;
    if (!logits || !seen || !counts || !params) return ASD_ERR_INVALID_ARG;
    if (ld_row < V || ld_seq < static_cast<int64_t>(K1) * ld_row) return ASD_ERR_INVALID_ARG;
    if (!step_tok && n_prev != 0) return ASD_ERR_INVALID_ARG;
    if (step_tok && (static_cast<int64_t>(n_prev) + K1 - 1 > n_tok || ld_tok < n_tok)) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(logits, static_cast<size_t>(esz)) || !aligned_to(seen, 4) || !aligned_to(counts, 4) || !aligned_to(params, 4) ||
        !aligned_to(step_tok, 4))
        return ASD_ERR_ALIGNMENT;
    const int64_t W = (static_cast<int64_t>(V) + 31) / 32;
    int64_t words = W < kSliceWords ? W : kSliceWords;
    while ((W + words - 1) / words > 65535) words += kSliceWords;   // gridDim.y
    const dim3 grid(static_cast<uint32_t>(B), static_cast<uint32_t>((W + words - 1) / words));
    dispatch_dtype(dtype, [&](auto dt) {
        hipLaunchKernelGGL((k_penalty_rows<decltype(dt)::value>), grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), logits,
                           ld_seq, ld_row, K1, V, seen, counts, params, step_tok, ld_tok, n_prev, static_cast<int>(words));
    });
    return launch_status();
}

ASD_EXPORT int asd_penalty_commit(const int32_t* tokens, int64_t ld_tokens, const int32_t* seq_len, const int32_t* n_commit,
                                  int B, int V, int max_len, uint32_t* seen, int32_t* counts, void* stream) {
    if (B < 0 || V < 0 || max_len < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0 || V == 0 || max_len == 0) return ASD_OK;
    if (!tokens || !seq_len || !n_commit || !seen || !counts) return ASD_ERR_INVALID_ARG;
    if (ld_tokens < max_len) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(tokens, 4) || !aligned_to(seq_len, 4) || !aligned_to(n_commit, 4) || !aligned_to(seen, 4) || !aligned_to(counts, 4))
        return ASD_ERR_ALIGNMENT;
    hipLaunchKernelGGL(k_penalty_commit, dim3(static_cast<uint32_t>(B)), dim3(kCommitThreads), 0, static_cast<hipStream_t>(stream),
                       tokens, ld_tokens, seq_len, n_commit, V, max_len, seen, counts);
    return launch_status();
}
