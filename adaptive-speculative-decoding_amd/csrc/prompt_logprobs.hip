// prompt_logprobs.hip -- the log-prob and the rank of one GIVEN token per row of [B][T][V] logits, and optionally the row's top-N
// table (SamplingParams(prompt_logprobs=N): scoring a prompt on the prefill's logits), gfx950.
//
// top_logprobs.hip's pass (top_logprobs_device.hpp: same stream, same lists, same merges, same hand-off) with two additions per
// scored row (b, t), g = target[b, t]:
//   lp   = row_logprob(x[g], c2, l2): a table slot's operations, so the bits of a slot that holds g;
//   rank = 1 + #{v : x[v] > x[g], or x[v] == x[g] and v < g}: the table's total order.  Every workgroup loads x[g] once ahead of
//          its stream and counts beside the lse and the list -- per wave, on the scalar unit: one v_cmp per element, s_bcnt1 and
//          s_add for the rest; the slices' counts travel in the slice partial.  Comparisons of stored values are exact, so the
//          rank does not depend on the geometry.
// With N == 0 (kScoreOnly) no list is kept.  A row with t < first[b] (left-padding) is not streamed: its workgroups write the
// neutral outputs and leave.  T is not bounded by the draft length, and the workspace is sized for the split count in use: whole
// rows (one slice) take no ticket and no partial.

#include "top_logprobs_device.hpp"

namespace asd {
namespace {

template <int DT, int kMode>
__global__ __launch_bounds__(kThreads) void k_prompt_logprobs(const PromptParams p) {
    top_logprobs_row<DT, false, kMode>(p);
}

inline int prompt_splits(int64_t R, int V, int esz, int splits) {
    return splits > 0 ? splits : choose_splits(R, V, esz, current_device_cus());
}
// whole rows need nothing: one 256-byte unit so that the pointer stays a valid, aligned argument
inline size_t prompt_workspace(int B, int T, int S) { return S > 1 ? layout(B, T, S).total : 256; }

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT size_t asd_prompt_logprobs_workspace_bytes(int B, int T, int V, int dtype, int splits) {
    const int esz = dtype_size(dtype);
    if (B <= 0 || T <= 0 || V <= 0 || esz == 0 || splits < 0 || splits > ASD_MAX_SPLITS) return 256;
    return prompt_workspace(B, T, prompt_splits(static_cast<int64_t>(B) * T, V, esz, splits));
}

ASD_EXPORT int asd_prompt_logprobs(const void* logits, int dtype, int64_t ld_seq, int64_t ld_row, int B, int T, int V,
                                   const int32_t* target, int64_t ld_target, const int32_t* first, float inv_temperature, int N,
                                   int splits, float* lp, int32_t* rank, int32_t* top_id, float* top_lp, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    if (B > 0 && T > 0 && (!lp || !rank || (N > 0 && (!top_id || !top_lp)))) return ASD_ERR_INVALID_ARG;
    if (!valid_inv_temperature(inv_temperature)) return ASD_ERR_INVALID_ARG;
    if (B < 0 || T < 0 || V < 0 || N < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0 || T == 0) return ASD_OK;
    if (V == 0) return ASD_ERR_INVALID_ARG;
    const int esz = dtype_size(dtype);
    if (esz == 0) return ASD_ERR_UNSUPPORTED;
    if (N > ASD_MAX_TOP_LOGPROBS || splits < 0 || splits > ASD_MAX_SPLITS) return ASD_ERR_UNSUPPORTED;
    if (!logits || !target || !workspace) return ASD_ERR_INVALID_ARG;
    if (ld_row < V || ld_seq < static_cast<int64_t>(T) * ld_row || ld_target < T) return ASD_ERR_INVALID_ARG;
    if (static_cast<int64_t>(V) * esz >= (int64_t{1} << 31)) return ASD_ERR_UNSUPPORTED;      // 32-bit byte offsets within a row
    if (!aligned_to(logits, static_cast<size_t>(esz))) return ASD_ERR_ALIGNMENT;
    if (!aligned_to(workspace, 256)) return ASD_ERR_WORKSPACE;
    const int64_t R = static_cast<int64_t>(B) * T;
    const int S = prompt_splits(R, V, esz, splits);
    if (R * S > INT32_MAX) return ASD_ERR_UNSUPPORTED;
    if (workspace_bytes < prompt_workspace(B, T, S)) return ASD_ERR_WORKSPACE;

    PromptParams p{};
    p.logits = logits; p.ld_seq = ld_seq; p.ld_row = ld_row;
    p.K1 = T; p.V = V; p.S = S; p.N = N;
    p.c2 = log2_scale(inv_temperature);
    p.top_id = top_id; p.top_lp = top_lp;
    p.target = target; p.ld_target = ld_target; p.first = first;
    p.lp = lp; p.rank = rank;

    hipStream_t st = static_cast<hipStream_t>(stream);
    if (S > 1) {               // (whole rows take no ticket)
        const Layout w = layout(B, T, S);
        char* const ws = static_cast<char*>(workspace);
        p.row_tickets = reinterpret_cast<uint32_t*>(ws);
        p.partials = reinterpret_cast<SlicePartial*>(ws + w.ticket_bytes);
        if (hipMemsetAsync(workspace, 0, w.ticket_bytes, st) != hipSuccess) return ASD_ERR_HIP;
    }
    const dim3 grid(static_cast<uint32_t>(R), static_cast<uint32_t>(S));
    dispatch_dtype(dtype, [&](auto dt) {
        if (N > 0) hipLaunchKernelGGL((k_prompt_logprobs<decltype(dt)::value, kScoreTop>), grid, dim3(kThreads), 0, st, p);
        else hipLaunchKernelGGL((k_prompt_logprobs<decltype(dt)::value, kScoreOnly>), grid, dim3(kThreads), 0, st, p);
    });
    return launch_status();
}
