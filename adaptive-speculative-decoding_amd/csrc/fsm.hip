// fsm.hip -- guided decoding ahead of the samplers, gfx950: a token-level deterministic automaton per sequence whose state
// lives on the device, because inside a speculative step the mask of position j depends on the proposals 0 .. j-1, which exist
// only there.  Three entry points:
//
//   asd_fsm_mask_rows   position j of sequence b is masked in place with row pos_state[b][first + j] of state_bits [S, W]:
//                       asd_logit_mask_rows with a mask index per (b, j) instead of per b.  The write stream is the SAME code
//                       (mask_slice of logit_mask_device.hpp): 16-byte all-clear stores, blended mixed chunks, head / tail
//                       handling, slice geometry.  A state outside [0, S) leaves the position alone.
//   asd_fsm_advance     pos_state[b][k + 1] = delta(pos_state[b][k], step_tok[b][k]): behind proposal k of a step.
//   asd_fsm_commit      behind the step's commit, for a sequence with c = n_commit[b] > 0 (clamped to ld_state):
//                       pos_state[b][0] = delta(pos_state[b][c - 1], tokens[b][seq_len[b] - 1]).  One transition is enough:
//                       the first c - 1 committed tokens of a step are its accepted proposals 0 .. c-2 (stops and limits cut
//                       from the end), so column c - 1 already is the state behind them.  c == 0: the state stays.
//
// The automaton is CSR: state s owns the edges [state_first[s], state_first[s + 1]) of edge_tok (ascending, distinct) /
// edge_next, and state_other[s] is the next state of every token without an edge.  delta(s, t):
//     s outside [0, S)                      -> s   (a sequence without an automaton holds -1; damaged data)
//     t has an edge in s                    -> that edge's next state
//     t has no edge in s                    -> state_other[s]
//     that result outside [0, S) (-1: the token is forbidden in s), or t outside [0, V)   -> s
// The last line cannot occur in correct operation (every proposal was drawn from masked logits); mapping it to "s unchanged"
// means a sequence never loses its non-empty mask.
//
// The two small kernels sit on the SERIAL draft path, where latency counts and bytes do not: one wave per sequence, and the
// wave searches the state's sorted edge range cooperatively -- per round every lane probes one edge, `step` edges apart, one
// wave ballot finds a probe that == t (a hit ends the search), a second counts the probes that are < t, and the range shrinks
// to the `step - 1` edges behind the last such probe: at most ceil(log64(n)) dependent rounds (3 at a vocabulary-sized state)
// against 18 for a per-lane binary search.  No LDS, no atomics; the result is one ordinary per-lane vector-memory store by lane 0.  Every index formed from device data is clamped
// (bad_words.hip's rule): the edge range into [0, E], seq_len into [1, max_len], n_commit into [1, ld_state]; tokens and states
// are compared as plain integers and a state indexes the tables only inside [0, S).

#include <hip/hip_runtime.h>

#include "common.hpp"
#include "logit_mask_device.hpp"

namespace asd {
namespace {

using namespace mask_stream;

constexpr int kWave = 64;

template <int DT>
__global__ __launch_bounds__(kThreads) void k_fsm_mask_rows(void* logits, int64_t ld_seq, int64_t ld_row, int K1, int V,
                                                            const uint32_t* __restrict__ state_bits, int S,
                                                            const int32_t* __restrict__ pos_state, int64_t ld_state, int first,
                                                            int words_per_slice) {
    using T = typename Elem<DT>::type;
    const int row = static_cast<int>(blockIdx.x);
    const int b = static_cast<int>(static_cast<uint32_t>(row) / static_cast<uint32_t>(K1));
    const int j = row - b * K1;
    const int s = pos_state[static_cast<int64_t>(b) * ld_state + first + j];      // first + K1 <= ld_state: the launcher's check
    if (s < 0 || s >= S) return;                                    // no automaton, or a damaged state: the position is not touched
    const int W = static_cast<int>((static_cast<int64_t>(V) + 31) >> 5);
    mask_slice<DT>(static_cast<T*>(logits) + static_cast<int64_t>(b) * ld_seq + static_cast<int64_t>(j) * ld_row,
                   state_bits + static_cast<int64_t>(s) * W, V, words_per_slice);
}

struct Tables {
    const int32_t* __restrict__ state_first;     // [S + 1]
    const int32_t* __restrict__ edge_tok;        // [E]
    const int32_t* __restrict__ edge_next;       // [E]
    const int32_t* __restrict__ state_other;     // [S]
    int S, E, V;
};

// delta(s, t) by the whole wave; s and t are wave-uniform, and so is everything derived from the ballots: every lane returns
// the same value.
__device__ __forceinline__ int delta(const Tables& a, int s, int t, int lane) {
    if (s < 0 || s >= a.S) return s;
    if (t < 0 || t >= a.V) return s;
    int lo = a.state_first[s], hi = a.state_first[s + 1];
    lo = lo < 0 ? 0 : (lo > a.E ? a.E : lo);                        // never outside the edge tables
    hi = hi < lo ? lo : (hi > a.E ? a.E : hi);
    int next = a.state_other[s];
    while (hi > lo) {                                               // the range shrinks to fewer than `step` edges per round
        const int n = hi - lo;
        const int step = (n + kWave - 1) / kWave;
        const int64_t at = static_cast<int64_t>(lo) + static_cast<int64_t>(lane) * step;
        const bool probing = at < hi;                               // ceil(n / step) <= 64 lanes probe
        const int e = probing ? a.edge_tok[at] : 0;
        const unsigned long long hit = __ballot(probing && e == t);
        if (hit) {                                                  // distinct ids: one lane at most
            const int owner = __ffsll(static_cast<long long>(hit)) - 1;
            next = a.edge_next[static_cast<int64_t>(lo) + static_cast<int64_t>(owner) * step];
            break;
        }
        const int below = __popcll(__ballot(probing && e < t));     // ascending ids: the probes below t come first
        if (below == 0) break;                                      // t lies in front of the range
        const int64_t from = static_cast<int64_t>(lo) + static_cast<int64_t>(below - 1) * step + 1;    // behind the last probe below t
        const int64_t to = from + step - 1;                         // in front of the next probe (or the end)
        lo = static_cast<int>(from);                                // from <= hi: probe below - 1 lay inside the range
        hi = static_cast<int>(to < hi ? to : hi);
    }
    return (next < 0 || next >= a.S) ? s : next;                    // forbidden (-1), or damaged: the state stays
}

__global__ __launch_bounds__(kWave) void k_fsm_advance(Tables a, int32_t* __restrict__ pos_state, int64_t ld_state, int k,
                                                       const int32_t* __restrict__ step_tok, int64_t ld_tok) {
    const int64_t b = blockIdx.x;
    const int lane = static_cast<int>(threadIdx.x);
    int32_t* const st = pos_state + b * ld_state;
    const int next = delta(a, st[k], step_tok[b * ld_tok + k], lane);             // k + 1 < ld_state, k < n_tok <= ld_tok: the launcher's
    if (lane == 0) st[k + 1] = next;
}

__global__ __launch_bounds__(kWave) void k_fsm_commit(Tables a, int32_t* __restrict__ pos_state, int64_t ld_state,
                                                      const int32_t* __restrict__ tokens, int64_t ld_tokens,
                                                      const int32_t* __restrict__ seq_len, const int32_t* __restrict__ n_commit,
                                                      int max_len) {
    const int64_t b = blockIdx.x;
    const int lane = static_cast<int>(threadIdx.x);
    int c = n_commit[b];
    if (c <= 0) return;                                             // a finished sequence: the state is frozen
    c = c > ld_state ? static_cast<int>(ld_state) : c;
    int L = seq_len[b];
    L = L < 1 ? 1 : (L > max_len ? max_len : L);                    // 1 <= max_len <= ld_tokens: the launcher's checks
    int32_t* const st = pos_state + b * ld_state;
    const int next = delta(a, st[c - 1], tokens[b * ld_tokens + L - 1], lane);
    if (lane == 0) st[0] = next;
}

// what the two small launchers check alike, in this order; B == 0 is answered by the callers in between
int check_tables(const int32_t* state_first, const int32_t* edge_tok, const int32_t* edge_next, const int32_t* state_other, int E) {
    if (!state_first || !state_other || (E > 0 && (!edge_tok || !edge_next))) return ASD_ERR_INVALID_ARG;
    return ASD_OK;
}

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT int asd_fsm_mask_rows(void* logits, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V,
                                 const uint32_t* state_bits, int S, const int32_t* pos_state, int64_t ld_state, int first,
                                 void* stream) {
    if (B < 0 || K1 < 0 || V < 0 || S < 0 || first < 0 || ld_state < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0 || K1 == 0 || V == 0 || S == 0) return ASD_OK;
    const int esz = dtype_size(dtype);
    if (esz == 0) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(B) * K1 > INT32_MAX) return ASD_ERR_UNSUPPORTED;
    if (!logits || !state_bits || !pos_state) return ASD_ERR_INVALID_ARG;
    if (ld_row < V || ld_seq < static_cast<int64_t>(K1) * ld_row) return ASD_ERR_INVALID_ARG;
    if (static_cast<int64_t>(first) + K1 > ld_state) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(logits, static_cast<size_t>(esz)) || !aligned_to(state_bits, 4) || !aligned_to(pos_state, 4)) return ASD_ERR_ALIGNMENT;
    const int64_t rows = static_cast<int64_t>(B) * K1;
    const int W = static_cast<int>((static_cast<int64_t>(V) + 31) / 32);
    const int words_per_slice = slice_words(rows, V, current_device_cus());
    const int n_slices = (W + words_per_slice - 1) / words_per_slice;
    const dim3 grid(static_cast<uint32_t>(rows), static_cast<uint32_t>(n_slices));
    dispatch_dtype(dtype, [&](auto dt) {
        hipLaunchKernelGGL((k_fsm_mask_rows<decltype(dt)::value>), grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), logits,
                           ld_seq, ld_row, K1, V, state_bits, S, pos_state, ld_state, first, words_per_slice);
    });
    return launch_status();
}

ASD_EXPORT int asd_fsm_advance(const int32_t* state_first, const int32_t* edge_tok, const int32_t* edge_next,
                               const int32_t* state_other, int S, int E, int V, int32_t* pos_state, int64_t ld_state, int B, int k,
                               const int32_t* step_tok, int64_t ld_tok, int n_tok, void* stream) {
    if (B < 0 || S < 0 || E < 0 || V < 0 || k < 0 || n_tok < 0 || ld_state < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0) return ASD_OK;
    if (n_tok > ASD_MAX_DRAFT_LEN) return ASD_ERR_UNSUPPORTED;
    if (check_tables(state_first, edge_tok, edge_next, state_other, E) != ASD_OK || !pos_state || !step_tok) return ASD_ERR_INVALID_ARG;
    if (static_cast<int64_t>(k) + 1 >= ld_state || k >= n_tok || ld_tok < n_tok) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(state_first, 4) || !aligned_to(edge_tok, 4) || !aligned_to(edge_next, 4) || !aligned_to(state_other, 4) ||
        !aligned_to(pos_state, 4) || !aligned_to(step_tok, 4))
        return ASD_ERR_ALIGNMENT;
    const Tables a{state_first, edge_tok, edge_next, state_other, S, E, V};
    hipLaunchKernelGGL(k_fsm_advance, dim3(static_cast<uint32_t>(B)), dim3(kWave), 0, static_cast<hipStream_t>(stream), a, pos_state,
                       ld_state, k, step_tok, ld_tok);
    return launch_status();
}

ASD_EXPORT int asd_fsm_commit(const int32_t* state_first, const int32_t* edge_tok, const int32_t* edge_next,
                              const int32_t* state_other, int S, int E, int V, int32_t* pos_state, int64_t ld_state, int B,
                              const int32_t* tokens, int64_t ld_tokens, const int32_t* seq_len, const int32_t* n_commit, int max_len,
                              void* stream) {
    if (B < 0 || S < 0 || E < 0 || V < 0 || max_len < 0 || ld_state < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0) return ASD_OK;
    if (check_tables(state_first, edge_tok, edge_next, state_other, E) != ASD_OK || !pos_state || !tokens || !seq_len || !n_commit)
        return ASD_ERR_INVALID_ARG;
    if (ld_state < 1 || max_len < 1 || ld_tokens < max_len) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(state_first, 4) || !aligned_to(edge_tok, 4) || !aligned_to(edge_next, 4) || !aligned_to(state_other, 4) ||
        !aligned_to(pos_state, 4) || !aligned_to(tokens, 4) || !aligned_to(seq_len, 4) || !aligned_to(n_commit, 4))
        return ASD_ERR_ALIGNMENT;
    const Tables a{state_first, edge_tok, edge_next, state_other, S, E, V};
    hipLaunchKernelGGL(k_fsm_commit, dim3(static_cast<uint32_t>(B)), dim3(kWave), 0, static_cast<hipStream_t>(stream), a, pos_state,
                       ld_state, tokens, ld_tokens, seq_len, n_commit, max_len);
    return launch_status();
}
