// top_logprobs.hip -- the N most likely tokens of every target row and their log-probs (SamplingParams(logprobs=N),
// docs/guides/RESEARCH_PROTOCOL.md:272-277 of the reference), gfx950.
//
// One streaming pass over [B][K1][V] rows read IN PLACE (sequence stride ld_seq, row stride ld_row; bf16 / f16 / f32), in
// greedy.hip's geometry and with its hand-off.  Per row the pass keeps the online log-sum-exp pair (m2, s) of lse_device.hpp --
// the same operations in the same order as greedy.hip, so slot 0's log-prob has the bits of asd_verify_greedy's lp_argmax -- and
// the 8 largest logits as (value, id) pairs; the first N are written, with lp = row_logprob(value) over the WHOLE vocabulary.
//
// Order (a total order, so the ids do not depend on the geometry): value descending, then id ascending.  A NaN logit and a
// logit of -inf are never listed; a slot that cannot be filled holds id -1 and lp -inf.  Slot 0 is asd_verify_greedy's arg-max.
//
// The per-lane list.  Every lane keeps its 8 best pairs sorted in registers (two arrays that are only ever indexed by unrolled
// constants: nothing is in scratch).  A lane walks increasing ids, so an element enters only on a strict `>` against the lane's
// 8th best, and an equal value with a higher id never displaces an entry.  A 16-byte vector is tested once, with its maximum.
// With 512 lanes a row of 152064 logits leaves ~300 elements per lane: tested against the lane's own 8th best alone, one lane
// or another of a wave would insert at nearly every vector.  So the test has a second, wave-wide part: `bound`, the smallest of
// the maxima of the wave's eight 8-lane groups, refreshed once per batch (3 DPP steps, 8 readlanes).  Eight distinct elements
// are >= bound, so an element below it is not among the row's 8 best and is skipped; `>=`, not `>`: an element that ties with
// the bound may still win on its id.  The list of a lane is then the 8 best of what it did NOT skip, which is all a merge needs.
//
// Merging is one routine, wave_top: 8 rounds of "wave maximum of the heads, lowest id among the lanes that hold it, that lane
// pops its head".  Lanes -> wave on the lanes' lists; waves -> workgroup with lane w of wave 0 holding wave w's list (through
// LDS); slices -> row with lane sl of the finisher's wave 0 holding slice sl's list (through the workspace; splits <= 64).  The
// (m2, s) pairs are combined in wave order and in slice order, as in greedy.hip.
//
// Hand-off: greedy.hip's tickets.  Plain stores, vmcnt drain, barrier, one agent-scope release and a relaxed fetch_add by lane 0;
// the workgroup that draws the row's last ticket acquires, and its wave 0 reads the partials with vector loads.  Nobody waits.
// The tickets are zeroed by a hipMemsetAsync ahead of every launch.
//
// The device parts described above live in top_logprobs_device.hpp, which prompt_logprobs.hip shares; this file holds the kernel
// entry (mode kTopOnly of the shared row body) and the launchers.

#include "top_logprobs_device.hpp"

namespace asd {
namespace {

// kRows (asd_top_logprobs_rows): the scale of sequence b is formed from inv_t[b] by log2_scale's own f64 product
template <int DT, bool kRows = false>
__global__ __launch_bounds__(kThreads) void k_top_logprobs(const TopParams p) {
    top_logprobs_row<DT, kRows, kTopOnly>(p);
}

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT size_t asd_top_logprobs_workspace_bytes(int B, int K1, int N) {
    (void)N;
    if (B <= 0 || K1 <= 0) return 256;
    return layout(B, K1, ASD_MAX_SPLITS).total;
}

namespace {
// asd_top_logprobs (inv_t_rows == nullptr) and asd_top_logprobs_rows (the scalar unused)
int top_logprobs_launch(const void* logits, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V, float inv_temperature,
                        const float* inv_t_rows, bool per_row, int N, int splits, int32_t* top_id, float* top_lp, void* workspace,
                        size_t workspace_bytes, void* stream) {
    if (B > 0 && (!top_id || !top_lp)) return ASD_ERR_INVALID_ARG;
    if (per_row ? (B > 0 && !inv_t_rows) : !valid_inv_temperature(inv_temperature)) return ASD_ERR_INVALID_ARG;
    if (B < 0 || K1 < 0 || V < 0 || N < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0) return ASD_OK;
    if (V == 0 || K1 < 1 || N < 1) return ASD_ERR_INVALID_ARG;
    if (K1 > ASD_MAX_DRAFT_LEN + 1 || N > ASD_MAX_TOP_LOGPROBS) return ASD_ERR_UNSUPPORTED;
    const int esz = dtype_size(dtype);
    if (esz == 0) return ASD_ERR_UNSUPPORTED;
    if (splits < 0 || splits > ASD_MAX_SPLITS) return ASD_ERR_UNSUPPORTED;
    if (!logits || !workspace) return ASD_ERR_INVALID_ARG;
    if (ld_row < V || ld_seq < static_cast<int64_t>(K1) * ld_row) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(logits, static_cast<size_t>(esz))) return ASD_ERR_ALIGNMENT;
    if (!aligned_to(workspace, 256)) return ASD_ERR_WORKSPACE;
    const int64_t R = static_cast<int64_t>(B) * K1;
    if (static_cast<int64_t>(V) * esz >= (int64_t{1} << 31)) return ASD_ERR_UNSUPPORTED;      // 32-bit byte offsets within a row
    const int S = splits > 0 ? splits : choose_splits(R, V, esz, current_device_cus());
    if (R * S > INT32_MAX) return ASD_ERR_UNSUPPORTED;
    const Layout w = layout(B, K1, S);
    if (workspace_bytes < w.total) return ASD_ERR_WORKSPACE;

    TopParams p{};
    p.logits = logits; p.ld_seq = ld_seq; p.ld_row = ld_row;
    p.K1 = K1; p.V = V; p.S = S; p.N = N;
    p.c2 = per_row ? 0.0f : log2_scale(inv_temperature);
    p.inv_t = inv_t_rows;
    p.top_id = top_id; p.top_lp = top_lp;
    char* const ws = static_cast<char*>(workspace);
    p.row_tickets = reinterpret_cast<uint32_t*>(ws);
    p.partials = reinterpret_cast<SlicePartial*>(ws + w.ticket_bytes);

    hipStream_t st = static_cast<hipStream_t>(stream);
    if (S > 1) {               // (whole rows take no ticket)
        if (hipMemsetAsync(workspace, 0, w.ticket_bytes, st) != hipSuccess) return ASD_ERR_HIP;
    }
    const dim3 grid(static_cast<uint32_t>(R), static_cast<uint32_t>(S));
    dispatch_dtype(dtype, [&](auto dt) {
        if (per_row) hipLaunchKernelGGL((k_top_logprobs<decltype(dt)::value, true>), grid, dim3(kThreads), 0, st, p);
        else hipLaunchKernelGGL((k_top_logprobs<decltype(dt)::value>), grid, dim3(kThreads), 0, st, p);
    });
    return launch_status();
}
}  // namespace

ASD_EXPORT int asd_top_logprobs(const void* logits, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V,
                                float inv_temperature, int N, int splits, int32_t* top_id, float* top_lp, void* workspace,
                                size_t workspace_bytes, void* stream) {
    return top_logprobs_launch(logits, dtype, ld_seq, ld_row, B, K1, V, inv_temperature, nullptr, false, N, splits, top_id, top_lp,
                               workspace, workspace_bytes, stream);
}

ASD_EXPORT int asd_top_logprobs_rows(const void* logits, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V,
                                     const float* inv_temperature, int N, int splits, int32_t* top_id, float* top_lp,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    return top_logprobs_launch(logits, dtype, ld_seq, ld_row, B, K1, V, 1.0f, inv_temperature, true, N, splits, top_id, top_lp,
                               workspace, workspace_bytes, stream);
}
