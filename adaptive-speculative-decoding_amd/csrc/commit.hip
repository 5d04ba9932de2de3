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
#include "common.hpp"

namespace asd {
namespace {

// kLp (asd_commit_step_lp): the log-probs of the committed tokens take the same path into row b of `out_lp` -- lp_tok[b, k]
// beside draft token k, lp_drawn[b] beside the drawn token -- so a stage that reports per-token log-probs needs no read-back.
template <bool kLp>
__global__ __launch_bounds__(64) void k_commit_step(const int32_t* tok, const float* lp_tok, const int32_t* n_acc,
                                                    const int32_t* drawn, const float* lp_drawn, int B, int K, int32_t* seq_len,
                                                    int32_t* out_tokens, float* out_lp, int64_t ld_out, int32_t* n_commit,
                                                    int32_t max_len) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    const int len = seq_len[b];                      // every lane reads the old length before lane 0 rewrites it
    int na = n_acc[b];
    na = na < 0 ? 0 : (na > K ? K : na);
    int32_t* row = out_tokens + static_cast<int64_t>(b) * ld_out;
    if (lane < na && len + lane < max_len) {
        row[len + lane] = tok[static_cast<int64_t>(b) * K + lane];
        if constexpr (kLp) out_lp[static_cast<int64_t>(b) * ld_out + len + lane] = lp_tok[static_cast<int64_t>(b) * K + lane];
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        if (len + na < max_len) {
            row[len + na] = drawn[b];
            if constexpr (kLp) out_lp[static_cast<int64_t>(b) * ld_out + len + na] = lp_drawn[b];
        }
        int appended = max_len - len;
        appended = appended < 0 ? 0 : (appended > na + 1 ? na + 1 : appended);
        seq_len[b] = len + appended;
        if (n_commit) n_commit[b] = appended;
    }
}

// asd_commit_step_stop: k_commit_step<true> with a stop set.  The wave finds the first committed candidate that is a stop id with
// one ballot (lane k tests draft token k; the drawn token, candidate n_acc, is tested by every lane alike, so K = 64 needs no
// 65th lane), cuts the append behind it, and lane 0 records why the row ended: finished[b] = 1 (stop) / 2 (length) and one
// ordinary atomic add on *n_finished at the 0 -> non-zero transition.  A row that enters finished is left as it is.
__global__ __launch_bounds__(64) void k_commit_step_stop(const int32_t* tok, const float* lp_tok, const int32_t* n_acc,
                                                         const int32_t* drawn, const float* lp_drawn, int B, int K,
                                                         const int32_t* stop_ids, int n_stop, int32_t* seq_len, int32_t* out_tokens,
                                                         float* out_lp, int64_t ld_out, int32_t* n_commit, int32_t* finished,
                                                         int32_t* n_finished, int32_t max_len) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    const int len = seq_len[b];                      // every lane reads the old length and flag before lane 0 rewrites them
    if (finished[b] != 0) {                          // wave-uniform
        if (lane == 0 && n_commit) n_commit[b] = 0;
        return;
    }
    int na = n_acc[b];
    na = na < 0 ? 0 : (na > K ? K : na);
    int fit = max_len - len;
    fit = fit < 0 ? 0 : (fit > na + 1 ? na + 1 : fit);
    const int32_t d = drawn[b];
    const int32_t c = lane < na ? tok[static_cast<int64_t>(b) * K + lane] : d;
    bool c_stops = false, d_stops = false;
    for (int s = 0; s < n_stop; ++s) {
        const int32_t id = stop_ids[s];
        c_stops |= c == id;
        d_stops |= d == id;
    }
    // rejected draft tokens (lane >= na) and candidates cut off by max_len (index >= fit) never stop a row
    const unsigned long long hits = __ballot(c_stops && lane < na && lane < fit);
    int j = hits ? __ffsll(hits) - 1 : ((d_stops && na < fit) ? na : -1);
    const int appended = j >= 0 ? j + 1 : fit;
    int32_t* row = out_tokens + static_cast<int64_t>(b) * ld_out;
    if (lane < na && lane < appended) {
        row[len + lane] = c;
        out_lp[static_cast<int64_t>(b) * ld_out + len + lane] = lp_tok[static_cast<int64_t>(b) * K + lane];
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        if (na < appended) {
            row[len + na] = d;
            out_lp[static_cast<int64_t>(b) * ld_out + len + na] = lp_drawn[b];
        }
        seq_len[b] = len + appended;
        if (n_commit) n_commit[b] = appended;
        const int32_t reason = j >= 0 ? 1 : (len + appended >= max_len ? 2 : 0);     // stop wins on the last free slot
        if (reason) {
            finished[b] = reason;
            if (n_finished) atomicAdd(n_finished, 1);
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

// asd_commit_step_finish: k_commit_step_stop with multi-token stop sequences, per-row sequence lists and a per-row length limit.
// The wave keeps the row's window in LDS: kHist = ASD_MAX_STOP_SEQ_LEN - 1 history tokens (stream positions len - kHist .. len - 1;
// read only inside [max(start, 0), len), anything else holds 0 and is never compared: a match that would begin in front of
// `start` is refused by its position) followed by the up to 65 candidates.  Lane j asks "does an owned sequence end at candidate
// j" by comparing backwards from slot kHist + j; candidate 64 (K = 64 with every draft token accepted: the drawn token) has no
// lane of its own and is tested by all lanes alike, only when no earlier candidate matched.  One ballot and a find-first-set give
// j*; a shuffle brings the matched sequence's index from lane j*.  Slots behind the drawn token are never read (a window ends
// at its own candidate and j < fit <= na + 1), so rejected draft tokens take no part.
constexpr int kHist = ASD_MAX_STOP_SEQ_LEN - 1;

// -> index (within the row's list) of the first owned sequence that ends at candidate j, or -1
__device__ __forceinline__ int first_seq_ending_at(const int32_t* win, int j, int len, int32_t start, const int32_t* seq_tok,
                                                   const int32_t* seq_n, int first, int n_own) {
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

__global__ __launch_bounds__(64) void k_commit_step_finish(const int32_t* tok, const float* lp_tok, const int32_t* n_acc,
                                                           const int32_t* drawn, const float* lp_drawn, int B, int K,
                                                           const int32_t* seq_tok, const int32_t* seq_n, int n_seq,
                                                           const int32_t* row_first, const int32_t* row_max_len, int32_t start,
                                                           int32_t* seq_len, int32_t* out_tokens, float* out_lp, int64_t ld_out,
                                                           int32_t* n_commit, int32_t* finished, int32_t* n_finished,
                                                           int32_t* matched, int32_t max_len) {
    __shared__ int32_t win[kHist + ASD_MAX_DRAFT_LEN + 1];
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    const int len = seq_len[b];                      // every lane reads the old length and flag before lane 0 rewrites them
    if (finished[b] != 0) {                          // wave-uniform
        if (lane == 0 && n_commit) n_commit[b] = 0;
        return;
    }
    int limit = max_len;
    if (row_max_len) {
        const int own = row_max_len[b] < 0 ? 0 : row_max_len[b];
        limit = own < max_len ? own : max_len;
    }
    int na = n_acc[b];
    na = na < 0 ? 0 : (na > K ? K : na);
    int fit = limit - len;
    fit = fit < 0 ? 0 : (fit > na + 1 ? na + 1 : fit);
    // the row's sequences: [first, first + n_own) of the n_seq uploaded ones, at most ASD_MAX_STOP_SEQS, never outside the arrays
    int first = 0, n_own = n_seq;
    if (row_first) {
        first = row_first[b];
        n_own = row_first[b + 1] - first;
    }
    if (first < 0 || first > n_seq) n_own = 0;
    n_own = n_own > n_seq - first ? n_seq - first : n_own;
    n_own = n_own < 0 ? 0 : (n_own > ASD_MAX_STOP_SEQS ? ASD_MAX_STOP_SEQS : n_own);
    const int32_t d = drawn[b];
    const int32_t c = lane < na ? tok[static_cast<int64_t>(b) * K + lane] : d;
    int32_t* row = out_tokens + static_cast<int64_t>(b) * ld_out;
    int j = -1, which = -1;
    if (n_own > 0 && fit > 0) {                      // wave-uniform
        if (lane < kHist) {
            const int64_t pos = static_cast<int64_t>(len) - kHist + lane;
            win[lane] = (pos >= start && pos >= 0) ? row[pos] : 0;           // pos < len < limit <= ld_out
        }
        if (lane <= na) win[kHist + lane] = c;       // slot na holds the drawn token (lane na == 64 does not exist: below)
        if (lane == 0 && na == 64) win[kHist + 64] = d;
        __syncthreads();
        const int mine = lane < fit ? first_seq_ending_at(win, lane, len, start, seq_tok, seq_n, first, n_own) : -1;
        const unsigned long long hits = __ballot(mine >= 0);
        if (hits) {
            j = __ffsll(hits) - 1;
            which = __shfl(mine, j);
        } else if (fit > 64) {                       // candidate 64, by every lane alike
            which = first_seq_ending_at(win, 64, len, start, seq_tok, seq_n, first, n_own);
            j = which >= 0 ? 64 : -1;
        }
    }
    const int appended = j >= 0 ? j + 1 : fit;
    if (lane < na && lane < appended) {
        row[len + lane] = c;
        out_lp[static_cast<int64_t>(b) * ld_out + len + lane] = lp_tok[static_cast<int64_t>(b) * K + lane];
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        if (na < appended) {
            row[len + na] = d;
            out_lp[static_cast<int64_t>(b) * ld_out + len + na] = lp_drawn[b];
        }
        seq_len[b] = len + appended;
        if (n_commit) n_commit[b] = appended;
        const int32_t reason = j >= 0 ? 1 : (len + appended >= limit ? 2 : 0);       // stop wins on the last free slot
        if (reason) {
            finished[b] = reason;
            if (n_finished) atomicAdd(n_finished, 1);
        }
        if (j >= 0 && matched) matched[b] = which;
    }
}

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT int asd_commit_step(const int32_t* tok, const int32_t* n_acc, const int32_t* drawn, int B, int K,
                               int32_t* seq_len, int32_t* out_tokens, int64_t ld_out, int32_t* n_commit, int32_t max_len,
                               void* stream) {
    if (B < 0 || K < 0 || max_len < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0) return ASD_OK;
    if (K > ASD_MAX_DRAFT_LEN) return ASD_ERR_UNSUPPORTED;
    if ((K > 0 && !tok) || !n_acc || !drawn || !seq_len || !out_tokens) return ASD_ERR_INVALID_ARG;
    if (ld_out < max_len) return ASD_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_commit_step<false>, dim3(B), dim3(64), 0, static_cast<hipStream_t>(stream), tok, nullptr, n_acc, drawn,
                       nullptr, B, K, seq_len, out_tokens, nullptr, ld_out, n_commit, max_len);
    return launch_status();
}

ASD_EXPORT int asd_commit_step_lp(const int32_t* tok, const float* lp_tok, const int32_t* n_acc, const int32_t* drawn,
                                  const float* lp_drawn, int B, int K, int32_t* seq_len, int32_t* out_tokens, float* out_lp,
                                  int64_t ld_out, int32_t* n_commit, int32_t max_len, void* stream) {
    if (B < 0 || K < 0 || max_len < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0) return ASD_OK;
    if (K > ASD_MAX_DRAFT_LEN) return ASD_ERR_UNSUPPORTED;
    if ((K > 0 && (!tok || !lp_tok)) || !n_acc || !drawn || !lp_drawn || !seq_len || !out_tokens || !out_lp) return ASD_ERR_INVALID_ARG;
    if (ld_out < max_len) return ASD_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_commit_step<true>, dim3(B), dim3(64), 0, static_cast<hipStream_t>(stream), tok, lp_tok, n_acc, drawn,
                       lp_drawn, B, K, seq_len, out_tokens, out_lp, ld_out, n_commit, max_len);
    return launch_status();
}

ASD_EXPORT int asd_commit_step_stop(const int32_t* tok, const float* lp_tok, const int32_t* n_acc, const int32_t* drawn,
                                    const float* lp_drawn, int B, int K, const int32_t* stop_ids, int n_stop, int32_t* seq_len,
                                    int32_t* out_tokens, float* out_lp, int64_t ld_out, int32_t* n_commit, int32_t* finished,
                                    int32_t* n_finished, int32_t max_len, void* stream) {
    if (B < 0 || K < 0 || max_len < 0 || n_stop < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0) return ASD_OK;
    if (K > ASD_MAX_DRAFT_LEN || n_stop > ASD_MAX_STOP_IDS) return ASD_ERR_UNSUPPORTED;
    if ((K > 0 && (!tok || !lp_tok)) || !n_acc || !drawn || !lp_drawn || !seq_len || !out_tokens || !out_lp) return ASD_ERR_INVALID_ARG;
    if (!finished || (n_stop > 0 && !stop_ids)) return ASD_ERR_INVALID_ARG;
    if (ld_out < max_len) return ASD_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_commit_step_stop, dim3(B), dim3(64), 0, static_cast<hipStream_t>(stream), tok, lp_tok, n_acc, drawn,
                       lp_drawn, B, K, stop_ids, n_stop, seq_len, out_tokens, out_lp, ld_out, n_commit, finished, n_finished, max_len);
    return launch_status();
}

ASD_EXPORT int asd_commit_step_finish(const int32_t* tok, const float* lp_tok, const int32_t* n_acc, const int32_t* drawn,
                                      const float* lp_drawn, int B, int K, const int32_t* seq_tok, const int32_t* seq_n, int n_seq,
                                      const int32_t* row_first, const int32_t* row_max_len, int32_t start, int32_t* seq_len,
                                      int32_t* out_tokens, float* out_lp, int64_t ld_out, int32_t* n_commit, int32_t* finished,
                                      int32_t* n_finished, int32_t* matched, int32_t max_len, void* stream) {
    if (B < 0 || K < 0 || max_len < 0 || n_seq < 0 || start < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0) return ASD_OK;
    if (K > ASD_MAX_DRAFT_LEN || (!row_first && n_seq > ASD_MAX_STOP_SEQS)) return ASD_ERR_UNSUPPORTED;
    if ((K > 0 && (!tok || !lp_tok)) || !n_acc || !drawn || !lp_drawn || !seq_len || !out_tokens || !out_lp) return ASD_ERR_INVALID_ARG;
    if (!finished || (n_seq > 0 && (!seq_tok || !seq_n))) return ASD_ERR_INVALID_ARG;
    if (ld_out < max_len) return ASD_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_commit_step_finish, dim3(B), dim3(64), 0, static_cast<hipStream_t>(stream), tok, lp_tok, n_acc, drawn,
                       lp_drawn, B, K, seq_tok, seq_n, n_seq, row_first, row_max_len, start, seq_len, out_tokens, out_lp, ld_out,
                       n_commit, finished, n_finished, matched, max_len);
    return launch_status();
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
