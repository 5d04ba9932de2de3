// commit.hip -- SURVEY §8(f) N3: the step after accept.  The reference's cache manager only has the
// name (src/serving/cache_manager.py:149-190 `truncate_at_stage` trims a dict of strings); in a
// token-level loop the rollback of a per-sequence KV cache is a LENGTH update: entries past the accepted
// prefix stay where they are and are overwritten by the next step (queries never look past their own
// position).  This kernel does the whole bookkeeping of one step on the device, so the loop needs no
// host synchronisation to learn n_acc:
//   row b of the token buffer receives tok[b, 0 .. n_acc[b]) followed by drawn[b] at seq_len[b],
//   seq_len[b] += n_acc[b] + 1  (clamped to max_len; tokens past max_len are dropped),
//   n_commit[b] = number of tokens actually appended.
// asd_commit_step_stop ends a row at a stop id, asd_commit_step_finish at a multi-token stop sequence of the row's own list or at
// the row's own length limit.
// One wave per sequence (K <= 64): lane k moves draft token k.  Integer work: bit-exact vs the oracle.
// All four entry points run ONE row body, k_commit; they differ in an END RULE, a compile-time policy that says where the append
// is cut: nowhere (EndNever), behind a stop id (EndAtIds), or where a stop sequence ends (EndAtSequences).
#include "common.hpp"

namespace asd {
namespace {

// What the four entry points share.  A pointer that an entry point does not have is NULL, and the instantiation that serves
// it contains no read of it (kLp, End::kEnds).
struct CommitArgs {
    const int32_t* tok;
    const float* lp_tok;
    const int32_t* n_acc;
    const int32_t* drawn;
    const float* lp_drawn;
    int K;
    int32_t* seq_len;
    int32_t* out_tokens;
    float* out_lp;
    int64_t ld_out;
    int32_t* n_commit;
    int32_t* finished;
    int32_t* n_finished;
    int32_t max_len;
};

// An end rule supplies three things.  limit(b, max_len): the length at which row b is full.  cut(...): the index of the first
// of the row's `fit` committed candidates that ends it (-1: none), where candidate k < na is draft token k, held by lane k
// in `c` (0 in the other lanes), and candidate na is the drawn token d; `which` receives the index of the owned sequence
// that did it.  record(b, which): lane 0's note of that sequence.  kEnds = false: rows never end, and the body keeps no
// finished flag at all.
struct EndNever {
    static constexpr bool kEnds = false;
    __device__ int limit(int, int max_len) const { return max_len; }
    __device__ int cut(int, int, int, int, int, int32_t, int32_t, const int32_t*, int&) const { return -1; }
    __device__ void record(int, int) const {}
};

// One ballot finds the first committed candidate that is a stop id: lane k tests draft token k; the drawn token, candidate na,
// is tested by every lane alike, so K = 64 needs no 65th lane.
struct EndAtIds {
    static constexpr bool kEnds = true;
    const int32_t* stop_ids;
    int n_stop;

    __device__ int limit(int, int max_len) const { return max_len; }
    __device__ int cut(int, int lane, int na, int fit, int, int32_t c, int32_t d, const int32_t*, int&) const {
        bool c_stops = false, d_stops = false;
        for (int s = 0; s < n_stop; ++s) {
            const int32_t id = stop_ids[s];
            c_stops |= c == id;
            d_stops |= d == id;
        }
        // rejected draft tokens (lane >= na) and candidates cut off by the limit (index >= fit) never stop a row
        const unsigned long long hits = __ballot(c_stops && lane < na && lane < fit);
        return hits ? __ffsll(hits) - 1 : ((d_stops && na < fit) ? na : -1);
    }
    __device__ void record(int, int) const {}
};

// Multi-token stop sequences, per-row sequence lists and a per-row length limit.
// The wave keeps the row's window in LDS: kHist = ASD_MAX_STOP_SEQ_LEN - 1 history tokens (stream positions len - kHist .. len - 1;
// read only inside [max(start, 0), len), anything else holds 0 and is never compared: a match that would begin in front of
// `start` is refused by its position) followed by the up to 65 candidates.  Lane j asks "does an owned sequence end at candidate
// j" by comparing backwards from slot kHist + j; candidate 64 (K = 64 with every draft token accepted: the drawn token) has no
// lane of its own and is tested by all lanes alike, only when no earlier candidate matched.  One ballot and a find-first-set give
// j*; a shuffle brings the matched sequence's index from lane j*.  Slots behind the drawn token are never read (a window ends
// at its own candidate and j < fit <= na + 1), so rejected draft tokens take no part.
struct EndAtSequences {
    static constexpr bool kEnds = true;
    static constexpr int kHist = ASD_MAX_STOP_SEQ_LEN - 1;
    const int32_t* seq_tok;
    const int32_t* seq_n;
    int n_seq;
    const int32_t* row_first;
    const int32_t* row_max_len;
    int32_t start;
    int32_t* matched;

    __device__ int limit(int b, int max_len) const {
        if (!row_max_len) return max_len;
        const int own = row_max_len[b] < 0 ? 0 : row_max_len[b];
        return own < max_len ? own : max_len;
    }

    // -> index (within the row's list) of the first owned sequence that ends at candidate j, or -1
    __device__ __forceinline__ int first_seq_ending_at(const int32_t* win, int j, int len, int first, int n_own) const {
        for (int s = 0; s < n_own; ++s) {
            const int m = seq_n[first + s];
            if (m < 1 || m > ASD_MAX_STOP_SEQ_LEN) continue;
            if (len + j - m + 1 < start) continue;                    // no token of a match lies in the prompt
            const int32_t* const want = seq_tok + static_cast<int64_t>(first + s) * ASD_MAX_STOP_SEQ_LEN;
            const int32_t* const have = win + kHist + j - m + 1;     // >= win: m <= kHist + 1
            bool same = true;
            for (int i = 0; i < m; ++i) same &= have[i] == want[i];
            if (same) return s;
        }
        return -1;
    }

    __device__ __forceinline__ int cut(int b, int lane, int na, int fit, int len, int32_t c, int32_t d, const int32_t* row,
                                       int& which) const {
        __shared__ int32_t win[kHist + ASD_MAX_DRAFT_LEN + 1];
        // the row's sequences: [first, first + n_own) of the n_seq uploaded, at most ASD_MAX_STOP_SEQS, never outside the arrays
        int first = 0, n_own = n_seq;
        if (row_first) {
            first = row_first[b];
            n_own = row_first[b + 1] - first;
        }
        if (first < 0 || first > n_seq) n_own = 0;
        n_own = n_own > n_seq - first ? n_seq - first : n_own;
        n_own = n_own < 0 ? 0 : (n_own > ASD_MAX_STOP_SEQS ? ASD_MAX_STOP_SEQS : n_own);
        if (n_own <= 0 || fit <= 0) return -1;           // wave-uniform
        if (lane < kHist) {
            const int64_t pos = static_cast<int64_t>(len) - kHist + lane;
            win[lane] = (pos >= start && pos >= 0) ? row[pos] : 0;           // pos < len < limit <= ld_out
        }
        if (lane <= na) win[kHist + lane] = lane < na ? c : d;       // slot na: the drawn token (lane 64 does not exist: below)
        if (lane == 0 && na == 64) win[kHist + 64] = d;
        __syncthreads();
        const int mine = lane < fit ? first_seq_ending_at(win, lane, len, first, n_own) : -1;
        const unsigned long long hits = __ballot(mine >= 0);
        if (hits) {
            const int j = __ffsll(hits) - 1;
            which = __shfl(mine, j);
            return j;
        }
        if (fit <= 64) return -1;
        which = first_seq_ending_at(win, 64, len, first, n_own);             // candidate 64, by every lane alike
        return which >= 0 ? 64 : -1;
    }
    __device__ void record(int b, int which) const {
        if (matched) matched[b] = which;
    }
};

// The row body.  kLp: the log-probs of the committed tokens take the same path into row b of `out_lp` -- lp_tok[b, k] beside
// draft token k, lp_drawn[b] beside the drawn token -- so a stage that reports per-token log-probs needs no read-back.
// End::kEnds: lane 0 records why the row ended, finished[b] = 1 (stop) / 2 (length), with one ordinary atomic add on
// *n_finished at the 0 -> non-zero transition; a row that enters finished is left as it is.
template <bool kLp, class End>
__global__ __launch_bounds__(64) void k_commit(const CommitArgs a, const End end) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    const int len = a.seq_len[b];                    // every lane reads the old length and flag before lane 0 rewrites them
    if constexpr (End::kEnds) {
        if (a.finished[b] != 0) {                    // wave-uniform
            if (lane == 0 && a.n_commit) a.n_commit[b] = 0;
            return;
        }
    }
    const int limit = end.limit(b, a.max_len);
    int na = a.n_acc[b];
    na = na < 0 ? 0 : (na > a.K ? a.K : na);
    int fit = limit - len;                           // candidates that fit: 0 for a row at or past its limit
    fit = fit < 0 ? 0 : (fit > na + 1 ? na + 1 : fit);
    const int64_t at_in = static_cast<int64_t>(b) * a.K + lane;      // this lane's draft token and its log-prob
    const int64_t at_out = static_cast<int64_t>(b) * a.ld_out + len;  // the row's first free slot
    const int32_t d = a.drawn[b];
    const int32_t c = lane < na ? a.tok[at_in] : 0;                   // (not d: the scatter must not wait for d's load)
    int32_t* row = a.out_tokens + static_cast<int64_t>(b) * a.ld_out;
    int which = -1;
    const int j = end.cut(b, lane, na, fit, len, c, d, row, which);
    const int appended = j >= 0 ? j + 1 : fit;
    if (lane < na && lane < appended) {
        row[len + lane] = c;
        if constexpr (kLp) a.out_lp[at_out + lane] = a.lp_tok[at_in];
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        if (na < appended) {
            row[len + na] = d;
            if constexpr (kLp) a.out_lp[at_out + na] = a.lp_drawn[b];
        }
        a.seq_len[b] = len + appended;
        if (a.n_commit) a.n_commit[b] = appended;
        if constexpr (End::kEnds) {
            const int32_t reason = j >= 0 ? 1 : (len + appended >= limit ? 2 : 0);     // stop wins on the last free slot
            if (reason) {
                a.finished[b] = reason;
                if (a.n_finished) atomicAdd(a.n_finished, 1);
            }
            if (j >= 0) end.record(b, which);
        }
    }
}

// asd_commit_top_logprobs: the top-N table of a step follows the step's commit.  It runs BEHIND asd_commit_step_lp /
// asd_commit_step_stop and reads what they left: seq_len[b] (already advanced) and n_commit[b].  Row j < n_commit[b] of
// top[b] -- the distribution the step's j-th committed token came from -- goes to position seq_len[b] - n_commit[b] + j of
// out[b].  One wave per sequence walks the n_commit * N entries; bits are copied.
__global__ __launch_bounds__(64) void k_commit_top_logprobs(const int32_t* top_id, const float* top_lp, const int32_t* seq_len,
                                                            const int32_t* n_commit, int B, int K1, int N, int32_t* out_id,
                                                            float* out_lp, int max_len) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    const int nc = n_commit[b];
    const int64_t first = static_cast<int64_t>(seq_len[b]) - nc;
    const int rows = nc < 0 ? 0 : (nc > K1 ? K1 : nc);
    const int32_t* const src_id = top_id + static_cast<int64_t>(b) * K1 * N;
    const float* const src_lp = top_lp + static_cast<int64_t>(b) * K1 * N;
    for (int e = lane; e < rows * N; e += 64) {
        const int j = e / N;
        const int64_t pos = first + j;
        if (pos < 0 || pos >= max_len) continue;
        const int64_t at = (static_cast<int64_t>(b) * max_len + pos) * N + (e - j * N);
        out_id[at] = src_id[e];
        out_lp[at] = src_lp[e];
    }
}

// The argument ladder of the four entry points.  Its order is part of the contract: sizes, the empty batch, limits, pointers
// (the lp pointers where the entry has them, then `finished`, then the entry's tables), ld_out.  An entry point passes the
// verdicts on its own arguments: own_sizes (none negative), own_limits (none above its maximum), own_tables (none missing).
int check_commit(const CommitArgs& a, int B, bool lp, bool ends, bool own_sizes, bool own_limits, bool own_tables) {
    if (B < 0 || a.K < 0 || a.max_len < 0 || !own_sizes) return ASD_ERR_INVALID_ARG;
    if (B == 0) return ASD_OK;
    if (a.K > ASD_MAX_DRAFT_LEN || !own_limits) return ASD_ERR_UNSUPPORTED;
    if ((a.K > 0 && !a.tok) || !a.n_acc || !a.drawn || !a.seq_len || !a.out_tokens) return ASD_ERR_INVALID_ARG;
    if (lp && ((a.K > 0 && !a.lp_tok) || !a.lp_drawn || !a.out_lp)) return ASD_ERR_INVALID_ARG;
    if ((ends && !a.finished) || !own_tables) return ASD_ERR_INVALID_ARG;
    if (a.ld_out < a.max_len) return ASD_ERR_INVALID_ARG;
    return ASD_OK;
}

// rc: check_commit's verdict; the empty batch passes it and launches nothing
template <bool kLp, class End>
int launch_commit(int rc, const CommitArgs& a, int B, const End& end, void* stream) {
    if (rc != ASD_OK || B == 0) return rc;
    hipLaunchKernelGGL((k_commit<kLp, End>), dim3(B), dim3(64), 0, static_cast<hipStream_t>(stream), a, end);
    return launch_status();
}

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT int asd_commit_step(const int32_t* tok, const int32_t* n_acc, const int32_t* drawn, int B, int K,
                               int32_t* seq_len, int32_t* out_tokens, int64_t ld_out, int32_t* n_commit, int32_t max_len,
                               void* stream) {
    const CommitArgs a{tok,     nullptr,    n_acc,   drawn,    nullptr, K,      seq_len,
                       out_tokens, nullptr, ld_out, n_commit, nullptr, nullptr, max_len};
    return launch_commit<false>(check_commit(a, B, false, false, true, true, true), a, B, EndNever{}, stream);
}

ASD_EXPORT int asd_commit_step_lp(const int32_t* tok, const float* lp_tok, const int32_t* n_acc, const int32_t* drawn,
                                  const float* lp_drawn, int B, int K, int32_t* seq_len, int32_t* out_tokens, float* out_lp,
                                  int64_t ld_out, int32_t* n_commit, int32_t max_len, void* stream) {
    const CommitArgs a{tok,        lp_tok, n_acc,  drawn,    lp_drawn, K,       seq_len,
                       out_tokens, out_lp, ld_out, n_commit, nullptr,  nullptr, max_len};
    return launch_commit<true>(check_commit(a, B, true, false, true, true, true), a, B, EndNever{}, stream);
}

ASD_EXPORT int asd_commit_step_stop(const int32_t* tok, const float* lp_tok, const int32_t* n_acc, const int32_t* drawn,
                                    const float* lp_drawn, int B, int K, const int32_t* stop_ids, int n_stop, int32_t* seq_len,
                                    int32_t* out_tokens, float* out_lp, int64_t ld_out, int32_t* n_commit, int32_t* finished,
                                    int32_t* n_finished, int32_t max_len, void* stream) {
    const CommitArgs a{tok,        lp_tok, n_acc,  drawn,    lp_drawn, K,          seq_len,
                       out_tokens, out_lp, ld_out, n_commit, finished, n_finished, max_len};
    const int rc = check_commit(a, B, true, true, n_stop >= 0, n_stop <= ASD_MAX_STOP_IDS, n_stop <= 0 || stop_ids);
    return launch_commit<true>(rc, a, B, EndAtIds{stop_ids, n_stop}, stream);
}

ASD_EXPORT int asd_commit_step_finish(const int32_t* tok, const float* lp_tok, const int32_t* n_acc, const int32_t* drawn,
                                      const float* lp_drawn, int B, int K, const int32_t* seq_tok, const int32_t* seq_n, int n_seq,
                                      const int32_t* row_first, const int32_t* row_max_len, int32_t start, int32_t* seq_len,
                                      int32_t* out_tokens, float* out_lp, int64_t ld_out, int32_t* n_commit, int32_t* finished,
                                      int32_t* n_finished, int32_t* matched, int32_t max_len, void* stream) {
    const CommitArgs a{tok,        lp_tok, n_acc,  drawn,    lp_drawn, K,          seq_len,
                       out_tokens, out_lp, ld_out, n_commit, finished, n_finished, max_len};
    const int rc = check_commit(a, B, true, true, n_seq >= 0 && start >= 0, row_first || n_seq <= ASD_MAX_STOP_SEQS,
                                n_seq <= 0 || (seq_tok && seq_n));
    return launch_commit<true>(rc, a, B, EndAtSequences{seq_tok, seq_n, n_seq, row_first, row_max_len, start, matched}, stream);
}

ASD_EXPORT int asd_commit_top_logprobs(const int32_t* top_id, const float* top_lp, const int32_t* seq_len, const int32_t* n_commit,
                                       int B, int K1, int N, int32_t* out_id, float* out_lp, int max_len, void* stream) {
    if (B < 0 || K1 < 0 || N < 0 || max_len < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0) return ASD_OK;
    if (K1 > ASD_MAX_DRAFT_LEN + 1 || N > ASD_MAX_TOP_LOGPROBS) return ASD_ERR_UNSUPPORTED;
    if (K1 < 1 || N < 1) return ASD_ERR_INVALID_ARG;
    if (!top_id || !top_lp || !seq_len || !n_commit || !out_id || !out_lp) return ASD_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_commit_top_logprobs, dim3(B), dim3(64), 0, static_cast<hipStream_t>(stream), top_id, top_lp, seq_len,
                       n_commit, B, K1, N, out_id, out_lp, max_len);
    return launch_status();
}
