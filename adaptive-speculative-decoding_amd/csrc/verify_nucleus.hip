// verify_nucleus.hip -- verify + accept against the TARGET's top-p nucleus (asd_verify_accept_top_p), gfx950.
// The reference samples every model with HF generate(do_sample=True, temperature=0.7, top_p=0.9)
// (src/training/generate_training_data.py:110-119, src/serving/real_model_pipeline.py:60,326,378), and HF's assisted
// generation runs the same warpers on the target's scores before the speculative test: the target is scored by the
// nucleus-renormalised softmax p^N, not by the full softmax(x / T) of asd_verify_accept_ex.  Specified in include/asd_hip.h.
//
// Two stream-ordered launches, nothing handed across workgroups (no workspace, no mailbox, no status word):
//   k_verify_nucleus  one 1024-lane workgroup per verified row r = b*K + k: phases 1-3 of k_draft_row (sample_device.hpp,
//                     nucleus_row_select: (m2, s), candidate lists above the mass floor, the mass-histogram select -> x*, L_N),
//                     then lp_t = log p^N(tok) (-inf below x*) and the accept test of finish_row
//   k_nucleus_finish  one wave per sequence: the ballot of the K accept flags -> n_acc, accept_bits, and the leading run of
//                     finite lp_t -> n_finite (the stop rule's n_valid)
// Because the select is the draft sampler's own code on the same row, x* and lp_t are the bits asd_draft_sample reports as
// nucleus_logit and log q(tok).  The row is read from HBM once (the later phases hit L2); the cost is the select's issue
// time, not bandwidth ("Target-side top-p").

#include "sample_device.hpp"

namespace asd {
namespace {

struct VnParams {
    const void* logits; int64_t ld;
    const int32_t* tok;
    const float* lp_d;
    const float* u;
    int B, K, V, nvec, n_tiles;
    float c2, top_p;
    int levels;               // 2: 16-bit logits; 3: f32 logits (the launcher routes top_p outside (0,1) elsewhere)
    float* lp_t;
    uint8_t* accept;
    int32_t* n_acc;
    uint64_t* bits;
    float* thr;               // [B*K] x* per row, or nullptr
    int32_t* n_finite;        // [B], or nullptr
    int top_k;                // k_verify_nucleus<DT, true> only (asd_verify_accept_top_k): 1 <= top_k < V; levels may then be 0
    float mp_delta;           // k_verify_nucleus<DT, *, true> only (asd_verify_accept_min_p): T ln(min_p) <= 0
};

// The body of k_verify_nucleus and of k_verify_nucleus_rows (the LDS is declared once, by the kernel)
template <int DT, bool kTopK, bool kMinP>
__device__ __forceinline__ void verify_nucleus_body(const VnParams& p, NucleusLds& sh) {
    using E = Elem<DT>;
    const int r = blockIdx.x, t = threadIdx.x;
    const u32x4* row = reinterpret_cast<const u32x4*>(static_cast<const char*>(p.logits) + static_cast<int64_t>(r) * p.ld * E::kBytes);
    // (kTopK: thr = max(x_k, x*_K) and L64 its normaliser -- the select of asd_draft_sample_top_k; kMinP: that of
    // asd_draft_sample_min_p, thr = max(thr_kp, x_max + mp_delta))
    const NucleusSel sel = nucleus_row_select<DT, kTopK, kMinP>(row, p.V, p.nvec, p.n_tiles, p.c2, p.top_p, p.levels, sh, t,
                                                                [](int) {}, p.top_k, p.mp_delta);
    if (t != 0) return;
    const int32_t tok = p.tok[r];
    const float x_tok = (tok >= 0 && tok < p.V) ? E::scalar(row, tok) : -INFINITY;
    // log p^N(tok) with the arithmetic of draft_pick_wave's log q(tok): the same bits for the token the draft sampler drew
    double lp = -INFINITY;
    if (!(x_tok < sel.thr)) lp = kLn2d * (static_cast<double>(x_tok) * static_cast<double>(p.c2) - sel.L64);   // (NaN stays NaN)
    if constexpr (kMinP) { if (lp > 0.0) lp = 0.0; }          // (draft_pick_wave's kClampLp: q = 1 never reads as log q > 0)
    const float lpf = static_cast<float>(lp);
    // finish_row's rule: p^N(tok) == 0 never accepts, not even at u == 0; NaN rejects by comparison
    const bool flag = lp > -INFINITY && log_u(p.u[r]) <= lp - static_cast<double>(p.lp_d[r]);
    p.lp_t[r] = lpf;
    p.accept[r] = flag ? 1 : 0;
    if (p.thr) p.thr[r] = sel.thr;
}

template <int DT, bool kTopK = false, bool kMinP = false>
__global__ __launch_bounds__(kDrThreads) void k_verify_nucleus(const VnParams p) {
    __shared__ NucleusLds sh;
    verify_nucleus_body<DT, kTopK, kMinP>(p, sh);
}

// asd_verify_accept_rows: row r = b*K + k takes the parameters of sequence b (rows[b], asd_sampling_rows_pack) and a
// workgroup-uniform branch on its mode into the body the scalar kernel of that mode runs.  A sequence that truncates nothing
// runs the <false, false> body with levels = 0: thr = -inf, lp_t from the sweep-1 normaliser (asd_draft_sample's lp bits).
template <int DT>
__global__ __launch_bounds__(kDrThreads) void k_verify_nucleus_rows(const VnParams p0, const SamplingRow* rows) {
    __shared__ NucleusLds sh;
    VnParams p = p0;
    const SamplingRow q = load_sampling_row(rows, static_cast<int>(blockIdx.x / static_cast<unsigned>(p0.K)));
    p.c2 = q.c2; p.top_p = q.top_p; p.levels = q.levels; p.top_k = q.top_k; p.mp_delta = q.mp_delta;
    if (q.clamp != 0u) {
        if (q.top_k > 0) verify_nucleus_body<DT, true, true>(p, sh);
        else verify_nucleus_body<DT, false, true>(p, sh);
    } else if (q.top_k > 0) verify_nucleus_body<DT, true, false>(p, sh);
    else verify_nucleus_body<DT, false, false>(p, sh);
}

// one wave per sequence: lane k < K reads row (b, k)'s flag and lp_t.  all_rows = 0: only n_finite (and nothing else) is written
__global__ __launch_bounds__(64) void k_nucleus_finish(const uint8_t* accept, const float* lp_t, int K, int all_rows,
                                                       int32_t* n_acc, uint64_t* bits, int32_t* n_finite) {
    const int b = blockIdx.x, lane = threadIdx.x;
    bool flag = false, fin = false;
    if (lane < K) {
        const float lp = lp_t[static_cast<int64_t>(b) * K + lane];
        fin = lp > -INFINITY && lp < INFINITY;
        if (all_rows) flag = accept[static_cast<int64_t>(b) * K + lane] != 0;
    }
    const unsigned long long fb = __ballot(fin);
    if (all_rows) finish_sequence(flag, lane, K, b, n_acc, bits);
    if (lane == 0 && n_finite) {
        const unsigned long long inv = ~fb;
        const int n = inv ? __builtin_ctzll(inv) : 64;
        n_finite[b] = n < K ? n : K;
    }
}

__global__ __launch_bounds__(256) void k_fill_f32(float* out, int64_t n, float v) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) out[i] = v;
}

}  // namespace
}  // namespace asd

using namespace asd;

namespace {
// asd_verify_accept_top_p (top_k = 0) and asd_verify_accept_top_k; a top_k that bounds nothing (<= 0 or >= V) is the former's
// call (the same bits).  min_p in (0, 1] (asd_verify_accept_min_p; 0 = none) always takes the select's route.
int verify_truncated(const void* logits, int dtype, int64_t ld_row, const int32_t* tok, const float* lp_draft, const float* u,
                     int B, int K, int V, float inv_temperature, int top_k, float top_p, float* lp_target, uint8_t* accept,
                     int32_t* n_acc, uint64_t* accept_bits, float* t_nucleus_logit, int32_t* n_finite, void* workspace,
                     size_t workspace_bytes, void* stream, float min_p = 0.0f) {
    if (B < 0 || K < 0 || V < 1) return ASD_ERR_INVALID_ARG;
    if (B == 0 || K == 0) return ASD_OK;
    if (K > ASD_MAX_DRAFT_LEN) return ASD_ERR_UNSUPPORTED;
    const RowGeom g = row_geom(V, dtype);
    if (g.esz == 0) return ASD_ERR_UNSUPPORTED;
    if (!logits || !tok || !lp_draft || !u || !lp_target || !accept || !n_acc || ld_row < V) return ASD_ERR_INVALID_ARG;
    if (!valid_inv_temperature(inv_temperature) || top_p != top_p) return ASD_ERR_INVALID_ARG;
    const int64_t R = static_cast<int64_t>(B) * K;
    if (R > INT32_MAX) return ASD_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Truncation tr = truncation(top_k, top_p, V, dtype);
    if (!tr.nucleus && tr.top_k == 0 && !(min_p > 0.0f)) {
        // no truncation: asd_verify_accept_ex itself (the same bits), then x* = -inf and the leading finite run
        asd_verify_options opt{};
        opt.inv_temperature = inv_temperature;
        opt.nontemporal = -1;
        const int rc = asd_verify_accept_ex(logits, dtype, ld_row, tok, lp_draft, u, B, K, V, lp_target, accept, n_acc,
                                            accept_bits, workspace, workspace_bytes, &opt, stream);
        if (rc != ASD_OK) return rc;
        if (t_nucleus_logit)
            hipLaunchKernelGGL(k_fill_f32, dim3(static_cast<unsigned>((R + 255) / 256)), dim3(256), 0, st, t_nucleus_logit, R, -INFINITY);
        if (n_finite) hipLaunchKernelGGL(k_nucleus_finish, dim3(static_cast<unsigned>(B)), dim3(64), 0, st, accept, lp_target, K, 0,
                                         n_acc, accept_bits, n_finite);
        return launch_status();
    }
    // the nucleus select streams whole 16-byte vectors of 16-byte aligned rows (as asd_draft_sample)
    if (!g.whole || !rows_aligned(logits, ld_row, g.esz)) return ASD_ERR_ALIGNMENT;
    if (g.n_tiles > kDrMaxTiles) return ASD_ERR_UNSUPPORTED;
    VnParams p{};
    p.logits = logits; p.ld = ld_row; p.tok = tok; p.lp_d = lp_draft; p.u = u;
    p.B = B; p.K = K; p.V = V;
    p.nvec = g.nvec; p.n_tiles = g.n_tiles;
    p.c2 = log2_scale(inv_temperature);
    p.top_p = top_p;
    p.levels = tr.levels;
    p.top_k = tr.top_k;
    p.mp_delta = min_p > 0.0f ? min_p_delta(min_p, inv_temperature) : 0.0f;
    p.lp_t = lp_target; p.accept = accept; p.n_acc = n_acc; p.bits = accept_bits;
    p.thr = t_nucleus_logit; p.n_finite = n_finite;
    const dim3 grid(static_cast<unsigned>(R)), block(kDrThreads);
    dispatch_dtype(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (min_p > 0.0f) {
            if (tr.top_k > 0) hipLaunchKernelGGL((k_verify_nucleus<DT, true, true>), grid, block, 0, st, p);
            else hipLaunchKernelGGL((k_verify_nucleus<DT, false, true>), grid, block, 0, st, p);
        } else if (tr.top_k > 0) hipLaunchKernelGGL((k_verify_nucleus<DT, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((k_verify_nucleus<DT, false>), grid, block, 0, st, p);
    });
    hipLaunchKernelGGL(k_nucleus_finish, dim3(static_cast<unsigned>(B)), dim3(64), 0, st, accept, lp_target, K, 1, n_acc,
                       accept_bits, n_finite);
    return launch_status();
}
}  // namespace

ASD_EXPORT int asd_verify_accept_top_p(const void* logits, int dtype, int64_t ld_row, const int32_t* tok,
                                       const float* lp_draft, const float* u, int B, int K, int V, float inv_temperature,
                                       float top_p, float* lp_target, uint8_t* accept, int32_t* n_acc, uint64_t* accept_bits,
                                       float* t_nucleus_logit, int32_t* n_finite, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    return verify_truncated(logits, dtype, ld_row, tok, lp_draft, u, B, K, V, inv_temperature, 0, top_p, lp_target, accept, n_acc,
                            accept_bits, t_nucleus_logit, n_finite, workspace, workspace_bytes, stream);
}

ASD_EXPORT int asd_verify_accept_top_k(const void* logits, int dtype, int64_t ld_row, const int32_t* tok,
                                       const float* lp_draft, const float* u, int B, int K, int V, float inv_temperature,
                                       int top_k, float top_p, float* lp_target, uint8_t* accept, int32_t* n_acc,
                                       uint64_t* accept_bits, float* t_nucleus_logit, int32_t* n_finite, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    return verify_truncated(logits, dtype, ld_row, tok, lp_draft, u, B, K, V, inv_temperature, top_k, top_p, lp_target, accept,
                            n_acc, accept_bits, t_nucleus_logit, n_finite, workspace, workspace_bytes, stream);
}

ASD_EXPORT int asd_verify_accept_min_p(const void* logits, int dtype, int64_t ld_row, const int32_t* tok,
                                       const float* lp_draft, const float* u, int B, int K, int V, float inv_temperature,
                                       int top_k, float top_p, float min_p, float* lp_target, uint8_t* accept, int32_t* n_acc,
                                       uint64_t* accept_bits, float* t_nucleus_logit, int32_t* n_finite, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    if (!valid_min_p(min_p)) return ASD_ERR_INVALID_ARG;
    return verify_truncated(logits, dtype, ld_row, tok, lp_draft, u, B, K, V, inv_temperature, top_k, top_p, lp_target, accept,
                            n_acc, accept_bits, t_nucleus_logit, n_finite, workspace, workspace_bytes, stream,
                            min_p > 0.0f ? min_p : 0.0f);
}

ASD_EXPORT int asd_verify_accept_rows(const void* logits, int dtype, int64_t ld_row, const int32_t* tok, const float* lp_draft,
                                      const float* u, int B, int K, int V, const void* rows, float* lp_target, uint8_t* accept,
                                      int32_t* n_acc, uint64_t* accept_bits, float* t_nucleus_logit, int32_t* n_finite,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace; (void)workspace_bytes;                 // the select's two launches: nothing is handed across workgroups
    if (B < 0 || K < 0 || V < 1) return ASD_ERR_INVALID_ARG;
    if (B == 0 || K == 0) return ASD_OK;
    if (K > ASD_MAX_DRAFT_LEN) return ASD_ERR_UNSUPPORTED;
    const RowGeom g = row_geom(V, dtype);
    if (g.esz == 0) return ASD_ERR_UNSUPPORTED;
    if (!logits || !tok || !lp_draft || !u || !lp_target || !accept || !n_acc || ld_row < V || !rows) return ASD_ERR_INVALID_ARG;
    const int64_t R = static_cast<int64_t>(B) * K;
    if (R > INT32_MAX) return ASD_ERR_UNSUPPORTED;
    if (!g.whole || !rows_aligned(logits, ld_row, g.esz)) return ASD_ERR_ALIGNMENT;
    if (g.n_tiles > kDrMaxTiles) return ASD_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    VnParams p{};
    p.logits = logits; p.ld = ld_row; p.tok = tok; p.lp_d = lp_draft; p.u = u;
    p.B = B; p.K = K; p.V = V;
    p.nvec = g.nvec; p.n_tiles = g.n_tiles;
    p.lp_t = lp_target; p.accept = accept; p.n_acc = n_acc; p.bits = accept_bits;
    p.thr = t_nucleus_logit; p.n_finite = n_finite;
    dispatch_dtype(dtype, [&](auto dt) {
        hipLaunchKernelGGL((k_verify_nucleus_rows<decltype(dt)::value>), dim3(static_cast<unsigned>(R)), dim3(kDrThreads), 0, st, p,
                           static_cast<const SamplingRow*>(rows));
    });
    hipLaunchKernelGGL(k_nucleus_finish, dim3(static_cast<unsigned>(B)), dim3(64), 0, st, accept, lp_target, K, 1, n_acc,
                       accept_bits, n_finite);
    return launch_status();
}
