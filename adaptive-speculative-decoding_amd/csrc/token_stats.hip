// token_stats.hip -- per COMMITTED token of a step: the rank of the token, the arg-max and its log-prob, the entropy of the row's
// softmax, and optionally the row's top-N table, in ONE streaming pass over [B][K1][V] logits (the quality predictor's
// uncertainty inputs, and vLLM's rank of a sampled token), gfx950.
//
// top_logprobs.hip's pass (top_logprobs_device.hpp: same stream, same lists, same merges, same hand-off; mode kStats) with
//   rank    = prompt_logprobs.hip's count for g, the token the row may commit: tok[b, j] for j < a, drawn[b] for j == a,
//             a = clamp(n_acc[b], 0, K1 - 1);
//   arg-max = the table's slot 0; with N == 0 (mode kStatsOnly) no list is kept, only the best element per lane, which is that
//             slot's element, so the bits are asd_top_logprobs' all the same;
//   entropy = ln2 (log2 s - u / s) from a third running sum u carried beside (m2, s) -- see the header.  u is merged across
//             lanes, waves and slices in the fixed order of the pair; a slice's u travels in SlicePartial's spare word, so the
//             workspace has asd_prompt_logprobs' layout and byte counts.
// Rows j > a are never committed: their workgroups write the neutral outputs and leave, as the rows below `first` do there.

#include "top_logprobs_device.hpp"

namespace asd {
namespace {

template <int DT, bool kRows, int kMode>
__global__ __launch_bounds__(kThreads) void k_token_stats(const StatsParams p) {
    top_logprobs_row<DT, kRows, kMode>(p);
}

inline int stats_splits(int64_t R, int V, int esz, int splits) {
    return splits > 0 ? splits : choose_splits(R, V, esz, current_device_cus());
}
// whole rows need nothing: one 256-byte unit so that the pointer stays a valid, aligned argument
inline size_t stats_workspace(int B, int K1, int S) { return S > 1 ? layout(B, K1, S).total : 256; }

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT size_t asd_token_stats_workspace_bytes(int B, int K1, int V, int dtype, int splits) {
    const int esz = dtype_size(dtype);
    if (B <= 0 || K1 <= 0 || V <= 0 || esz == 0 || splits < 0 || splits > ASD_MAX_SPLITS) return 256;
    return stats_workspace(B, K1, stats_splits(static_cast<int64_t>(B) * K1, V, esz, splits));
}

ASD_EXPORT int asd_token_stats(const void* logits, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V,
                               const int32_t* tok, int64_t ld_tok, const int32_t* n_acc, const int32_t* drawn, float inv_temperature,
                               const float* inv_t_rows, int N, int splits, int32_t* stat_id, float* stat_val, int32_t* top_id,
                               float* top_lp, void* workspace, size_t workspace_bytes, void* stream) {
    if (B > 0 && K1 > 0 && (!stat_id || !stat_val || (N > 0 && (!top_id || !top_lp)))) return ASD_ERR_INVALID_ARG;
    if (!inv_t_rows && !valid_inv_temperature(inv_temperature)) return ASD_ERR_INVALID_ARG;
    if (B < 0 || K1 < 0 || V < 0 || N < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0 || K1 == 0) return ASD_OK;
    if (V == 0) return ASD_ERR_INVALID_ARG;
    const int esz = dtype_size(dtype);
    if (esz == 0) return ASD_ERR_UNSUPPORTED;
    if (N > ASD_MAX_TOP_LOGPROBS || splits < 0 || splits > ASD_MAX_SPLITS || K1 > ASD_MAX_DRAFT_LEN + 1) return ASD_ERR_UNSUPPORTED;
    if (!logits || !n_acc || !drawn || !workspace || (K1 > 1 && !tok)) return ASD_ERR_INVALID_ARG;
    if (ld_row < V || ld_seq < static_cast<int64_t>(K1) * ld_row || (K1 > 1 && ld_tok < K1 - 1)) return ASD_ERR_INVALID_ARG;
    if (static_cast<int64_t>(V) * esz >= (int64_t{1} << 31)) return ASD_ERR_UNSUPPORTED;      // 32-bit byte offsets within a row
    if (!aligned_to(logits, static_cast<size_t>(esz))) return ASD_ERR_ALIGNMENT;
    if (!aligned_to(workspace, 256)) return ASD_ERR_WORKSPACE;
    const int64_t R = static_cast<int64_t>(B) * K1;
    const int S = stats_splits(R, V, esz, splits);
    if (R * S > INT32_MAX) return ASD_ERR_UNSUPPORTED;
    if (workspace_bytes < stats_workspace(B, K1, S)) return ASD_ERR_WORKSPACE;

    StatsParams p{};
    p.logits = logits; p.ld_seq = ld_seq; p.ld_row = ld_row;
    p.K1 = K1; p.V = V; p.S = S; p.N = N;
    p.c2 = inv_t_rows ? 0.0f : log2_scale(inv_temperature);
    p.inv_t = inv_t_rows;
    p.top_id = top_id; p.top_lp = top_lp;
    p.tok = tok; p.ld_tok = ld_tok; p.n_acc = n_acc; p.drawn = drawn;
    p.stat_id = stat_id; p.stat_val = stat_val;

    hipStream_t st = static_cast<hipStream_t>(stream);
    if (S > 1) {               // (whole rows take no ticket)
        const Layout w = layout(B, K1, S);
        char* const ws = static_cast<char*>(workspace);
        p.row_tickets = reinterpret_cast<uint32_t*>(ws);
        p.partials = reinterpret_cast<SlicePartial*>(ws + w.ticket_bytes);
        if (hipMemsetAsync(workspace, 0, w.ticket_bytes, st) != hipSuccess) return ASD_ERR_HIP;
    }
    const dim3 grid(static_cast<uint32_t>(R), static_cast<uint32_t>(S));
    dispatch_dtype(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (N > 0) {
            if (inv_t_rows) hipLaunchKernelGGL((k_token_stats<DT, true, kStats>), grid, dim3(kThreads), 0, st, p);
            else hipLaunchKernelGGL((k_token_stats<DT, false, kStats>), grid, dim3(kThreads), 0, st, p);
        } else {
            if (inv_t_rows) hipLaunchKernelGGL((k_token_stats<DT, true, kStatsOnly>), grid, dim3(kThreads), 0, st, p);
            else hipLaunchKernelGGL((k_token_stats<DT, false, kStatsOnly>), grid, dim3(kThreads), 0, st, p);
        }
    });
    return launch_status();
}
