// dry.hip -- the DRY ("don't repeat yourself") repetition penalty ahead of the samplers, gfx950 / wave64: a token is penalised
// in proportion to the length of the repetition it would extend.
//
// logits[b][j][v] lies at b*ld_seq + j*ld_row + v (asd_bad_words_rows' addressing; bf16 / f16 / f32).  The history of position
// j of sequence b is asd_no_repeat_ngram_rows':
//   H = tokens[b][row_start[b] .. L)  ++  step_tok[b][0 .. n_prev + j),     L = clamp(seq_len[b], start, max_len)
// and H' its last `range` tokens (range == 0: all of it), len = |H'|, last = H'[len-1].  Record b holds {on, allowed_length,
// range, n_breakers, breakers[32], pen[CAP+1]} with CAP = ASD_DRY_MAX_MATCH.  For every i in [0, len-2] with H'[i] == last the
// follower t = H'[i+1] is a candidate with match length m_i = the number of k = 0, 1, .. < min(i+1, CAP) for which
// H'[i-k] == H'[len-1-k] and H'[len-1-k] is no breaker, counted until the first failure; M_t = max m_i; and where
// M_t >= allowed_length, x_t <- max(x_t - pen[M_t], lowest finite) in f32, rounded once to the dtype.  A breaker or a token
// outside [0, V) is no follower; -inf and NaN elements stay.  The device evaluates no pow: pen[] is the host's table.
//
// One workgroup of 1024 lanes serves one (b, j); nothing is shared between workgroups and there is no workspace.
//   1. Wave 0 writes the suffix to LDS in REVERSE order, s_suf[k] = H'[len-1-k], and one ballot cuts it at the first breaker
//      (or at CAP, or at len): the walk below then needs no breaker test.  A suffix shorter than allowed_length ends the
//      workgroup: no match can reach the threshold.
//   2. The history passes through LDS in tiles of kTile positions with a halo of CAP - 1 in front and the follower behind, so
//      that every walk reads LDS only.  A lane compares H'[i] with `last` first -- almost every position ends there -- and
//      a hit walks backwards against s_suf.  An all-equal history walks CAP steps per position in lock step: len * CAP compares.
//   3. The maximum per follower is formed ON CHIP: an LDS hash table of kSlots (token, m) pairs, a slot claimed by one
//      compare-and-swap on its key, the length merged by one atomic max on its value (skipped where the slot already holds as
//      much, which keeps an all-equal history from serialising on one address).  Which slot a token gets depends on the
//      schedule; the set of (token, max) pairs does not.
//   4. One lane per occupied slot does the one read-modify-write of that token's logit.
// A history with more distinct penalised followers than kLoad does not fit: the pass then sets a flag, applies NOTHING, and
// the token ids are split by their low bits -- class (r, R) = { t : t mod R == r } becomes (r, 2R) and (r + R, 2R) -- each of
// which scans the history again on its own.  The classes are walked as a binary tree without a stack; every token belongs to
// exactly one class that fits, so it is written exactly once with its exact maximum, however long the history.
// Damaged device data never leaves the arrays: seq_len[b] and row_start[b] are clamped as the n-gram kernel clamps them,
// allowed_length into [1, CAP], n_breakers into [0, 32], a negative range counts as 0, and a history token outside [0, V) is
// compared but never becomes a key.  `tokens` and the records are only read.

#include <hip/hip_runtime.h>

#include "common.hpp"

namespace asd {
namespace {

constexpr int kThreads = 1024;
constexpr int kCap = ASD_DRY_MAX_MATCH;
constexpr int kMaxBreakers = ASD_MAX_DRY_BREAKERS;
constexpr int kTile = 4096;                      // candidate positions per pass through LDS: four per lane
constexpr int kTileLds = kTile + kCap;           // ... with the halo of kCap - 1 in front and the last follower behind
constexpr int kSlots = 2048;                     // (token, m) slots of the LDS table, a power of two
constexpr int kLoad = kSlots / 2;                // distinct followers one pass may hold: the table stays half empty
constexpr int kEmpty = -1;

static_assert(kCap == 64, "wave 0 holds the suffix: one lane per token, one ballot word");
static_assert((kSlots & (kSlots - 1)) == 0 && kSlots == 1 << 11, "the table: the hash keeps 11 bits");

// round to nearest even, the conversion of torch's .to(bfloat16) (penalty.hip's); a NaN stays a (quiet) NaN
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return static_cast<uint16_t>((u >> 16) | 0x0040u);
    return static_cast<uint16_t>((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// x <- max(x - pen, lowest finite), in f32, rounded once; an element that is not finite (-inf, NaN, +inf) stays as it is
template <int DT>
__device__ __forceinline__ void penalise_one(void* logits, int64_t at, float pen) {
    if constexpr (DT == ASD_DTYPE_BF16) {
        uint16_t* const q = static_cast<uint16_t*>(logits) + at;
        const float x = __uint_as_float(static_cast<uint32_t>(*q) << 16);
        if (!(fabsf(x) < INFINITY)) return;
        const float y = x - pen;                 // (pen may be +inf: y is -inf then, and is clamped)
        *q = y < -3.3895313892515355e+38f ? static_cast<uint16_t>(0xFF7Fu) : f32_to_bf16(y);
    } else if constexpr (DT == ASD_DTYPE_F16) {
        _Float16* const q = static_cast<_Float16*>(logits) + at;
        const float x = static_cast<float>(*q);
        if (!(fabsf(x) < INFINITY)) return;
        const float y = x - pen;
        *q = y < -65504.0f ? static_cast<_Float16>(-65504.0f) : static_cast<_Float16>(y);      // v_cvt_f16_f32: to nearest even
    } else {
        float* const q = static_cast<float*>(logits) + at;
        const float x = *q;
        if (!(fabsf(x) < INFINITY)) return;
        const float y = x - pen;
        *q = y < -3.402823466e+38f ? -3.402823466e+38f : y;
    }
}

template <int DT>
__global__ __launch_bounds__(kThreads) void k_dry_rows(void* logits, int64_t ld_seq, int64_t ld_row, int K1, int V,
                                                       const asd_dry_rec* __restrict__ recs,
                                                       const int32_t* __restrict__ row_start,
                                                       const int32_t* __restrict__ tokens, int64_t ld_tokens,
                                                       const int32_t* __restrict__ seq_len, int start, int max_len,
                                                       const int32_t* __restrict__ step_tok, int64_t ld_tok, int n_prev) {
    __shared__ int32_t s_tile[kTileLds];         // s_tile[q] = H'[i0 - (kCap - 1) + q]
    __shared__ int32_t s_key[kSlots];            // a follower's token id, or kEmpty
    __shared__ int32_t s_val[kSlots];            // its longest match so far
    __shared__ int32_t s_suf[kCap];              // s_suf[k] = H'[len - 1 - k], k < s_n_suf
    __shared__ int32_t s_brk[kMaxBreakers];
    __shared__ float s_pen[kCap + 1];
    __shared__ int32_t s_n_suf, s_claimed, s_overflow;

    const int tid = static_cast<int>(threadIdx.x);
    const int row = static_cast<int>(blockIdx.x);
    const int b = static_cast<int>(static_cast<uint32_t>(row) / static_cast<uint32_t>(K1));
    const int j = row - b * K1;
    const asd_dry_rec* const rec = recs + b;
    if (rec->on == 0) return;                                // the row is off (uniform: the whole workgroup leaves)
    int allowed = rec->allowed_length;
    allowed = allowed < 1 ? 1 : (allowed > kCap ? kCap : allowed);
    int n_brk = rec->n_breakers;
    n_brk = n_brk < 0 ? 0 : (n_brk > kMaxBreakers ? kMaxBreakers : n_brk);
    const int range = rec->range;
    int L = seq_len[b];
    L = L < start ? start : (L > max_len ? max_len : L);     // start <= max_len <= ld_tokens: the launcher's checks
    int first = start;
    if (row_start) {
        first = row_start[b];
        first = first < 0 ? 0 : (first > start ? start : first);
    }
    const int n_com = L - first;                             // real prompt ids and committed generated tokens: one run of `tokens`
    const int n_see = step_tok ? n_prev + j : 0;             // proposals this position sees; n_prev + K1 - 1 <= n_tok: the launcher's
    const int len_h = n_com + n_see;                         // <= max_len + n_tok < 2^31 - kTileLds: the launcher's
    const int off = (range > 0 && len_h > range) ? len_h - range : 0;
    const int len = len_h - off;                             // |H'|
    if (len < 2) return;
    const int32_t* const committed = tokens + static_cast<int64_t>(b) * ld_tokens + first;
    const int64_t proposed = static_cast<int64_t>(b) * ld_tok - n_com;
    // H'[p] for 0 <= p < len, piecewise: a match may lie in `tokens`, in `step_tok`, or across both
    auto hist = [&](int p) -> int {
        const int h = off + p;
        return h < n_com ? committed[h] : step_tok[proposed + h];
    };
    auto is_breaker = [&](int t) -> bool {
        bool hit = false;
        for (int k = 0; k < n_brk; ++k) hit |= s_brk[k] == t;
        return hit;
    };

    if (tid < n_brk) s_brk[tid] = rec->breakers[tid];
    if (tid >= 64 && tid < 64 + kCap + 1) s_pen[tid - 64] = rec->pen[tid - 64];
    __syncthreads();
    if (tid < kCap) {                                        // wave 0: the suffix in reverse, cut at the first breaker
        const bool have = tid < len;
        const int t = have ? hist(len - 1 - tid) : 0;
        s_suf[tid] = t;
        const bool stop = !have || is_breaker(t);
        const unsigned long long cut = __ballot(stop);
        if (tid == 0) s_n_suf = cut ? __ffsll(cut) - 1 : kCap;
    }
    __syncthreads();
    const int n_suf = s_n_suf;                               // 0: `last` is a breaker
    if (n_suf < allowed) return;                             // no match can reach allowed_length (uniform)
    const int last = s_suf[0];
    const int64_t out = static_cast<int64_t>(b) * ld_seq + static_cast<int64_t>(j) * ld_row;
    const int n_cand = len - 1;                              // candidate positions i in [0, len - 2]

    // the classes of token ids, (r, R) = { t : (t & (R - 1)) == r }, walked as a binary tree; (0, 1) is every token
    uint32_t r = 0, R = 1;
    for (;;) {
        for (int s = tid; s < kSlots; s += kThreads) {
            s_key[s] = kEmpty;
            s_val[s] = 0;
        }
        if (tid == 0) {
            s_claimed = 0;
            s_overflow = 0;
        }
        __syncthreads();
        for (int i0 = 0; i0 < n_cand; i0 += kTile) {
            const int p_end = (n_cand - i0 > kTile ? i0 + kTile : n_cand) + 1;       // one past the last follower; <= len
            for (int q = tid; q < kTileLds; q += kThreads) {
                const int p = i0 - (kCap - 1) + q;
                if (p >= 0 && p < p_end) s_tile[q] = hist(p);
            }
            __syncthreads();
            for (int i = i0 + tid; i < p_end - 1; i += kThreads) {
                const int32_t* const at = s_tile + (i - i0 + kCap - 1);              // at[-k] = H'[i - k], at[1] = the follower
                if (at[0] != last) continue;
                const int t = at[1];
                if (t < 0 || t >= V || (static_cast<uint32_t>(t) & (R - 1)) != r) continue;
                const int m_max = i + 1 < n_suf ? i + 1 : n_suf;
                int m = 1;
                while (m < m_max && at[-m] == s_suf[m]) ++m;
                if (m < allowed || is_breaker(t)) continue;
                if (__atomic_load_n(&s_overflow, __ATOMIC_RELAXED)) continue;        // the pass is lost: it will be split
                uint32_t s = (static_cast<uint32_t>(t) * 2654435761u) >> 21;         // 11 bits: kSlots
                int probes = 0;
                for (; probes < kSlots; ++probes) {
                    int k = __atomic_load_n(&s_key[s], __ATOMIC_RELAXED);
                    if (k == kEmpty) {
                        k = atomicCAS(&s_key[s], kEmpty, t);
                        if (k == kEmpty) {
                            if (atomicAdd(&s_claimed, 1) >= kLoad) atomicExch(&s_overflow, 1);
                            k = t;
                        }
                    }
                    if (k == t) break;
                    s = (s + 1) & (kSlots - 1);
                }
                if (probes == kSlots) {                      // (a full table: more lanes claimed at once than kSlots - kLoad)
                    atomicExch(&s_overflow, 1);
                    continue;
                }
                if (__atomic_load_n(&s_val[s], __ATOMIC_RELAXED) < m) atomicMax(&s_val[s], m);
            }
            __syncthreads();
        }
        const bool overflow = s_overflow != 0;
        if (!overflow) {
            for (int s = tid; s < kSlots; s += kThreads) {
                const int t = s_key[s];
                if (t != kEmpty) penalise_one<DT>(logits, out + t, s_pen[s_val[s]]);   // allowed <= s_val[s] <= n_suf <= kCap
            }
        }
        __syncthreads();                                     // the table is read; the next class clears it
        if (overflow) {
            R <<= 1;                                         // the left child (r, 2R); R stays below 2V: a class of one id fits
            continue;
        }
        while (R > 1 && (r & (R >> 1))) {                    // a right child is done: so is its parent
            r -= R >> 1;
            R >>= 1;
        }
        if (R == 1) break;
        r += R >> 1;                                         // the sibling
    }
}

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT int asd_dry_rows(void* logits, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V, const asd_dry_rec* recs,
                            const int32_t* row_start, const int32_t* tokens, int64_t ld_tokens, const int32_t* seq_len, int start,
                            int max_len, const int32_t* step_tok, int64_t ld_tok, int n_tok, int n_prev, void* stream) {
    if (B < 0 || K1 < 0 || V < 0 || n_tok < 0 || n_prev < 0 || start < 0 || max_len < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0 || K1 == 0 || V == 0) return ASD_OK;
    const int esz = dtype_size(dtype);
    if (esz == 0) return ASD_ERR_UNSUPPORTED;
    if (n_tok > ASD_MAX_DRAFT_LEN) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(B) * K1 > INT32_MAX) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(max_len) + n_tok > INT32_MAX - kTileLds) return ASD_ERR_UNSUPPORTED;   // the scan counts in int32
    if (!logits || !recs || !tokens || !seq_len) return ASD_ERR_INVALID_ARG;
    if (ld_row < V || ld_seq < static_cast<int64_t>(K1) * ld_row || ld_tokens < max_len || start > max_len) return ASD_ERR_INVALID_ARG;
    if (!step_tok && n_prev != 0) return ASD_ERR_INVALID_ARG;
    if (step_tok && (static_cast<int64_t>(n_prev) + K1 - 1 > n_tok || ld_tok < n_tok)) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(logits, static_cast<size_t>(esz)) || !aligned_to(recs, 4) || !aligned_to(row_start, 4) || !aligned_to(tokens, 4) ||
        !aligned_to(seq_len, 4) || !aligned_to(step_tok, 4))
        return ASD_ERR_ALIGNMENT;
    const dim3 grid(static_cast<uint32_t>(static_cast<int64_t>(B) * K1));
    dispatch_dtype(dtype, [&](auto dt) {
        hipLaunchKernelGGL((k_dry_rows<decltype(dt)::value>), grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), logits,
                           ld_seq, ld_row, K1, V, recs, row_start, tokens, ld_tokens, seq_len, start, max_len, step_tok, ld_tok,
                           n_prev);
    });
    return launch_status();
}
