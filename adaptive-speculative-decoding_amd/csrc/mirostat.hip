// mirostat.hip -- Mirostat v2 (llama.cpp's mirostat_v2) ahead of the samplers, gfx950: a surprise cut against a running target
// mu that is carried per sequence and CHAINED through the K1 rows of a verifying step.  include/asd_hip.h holds the semantics.
//
// logits[b][j][v] lies at b*ld_seq + j*ld_row + v (asd_entropy_cut_rows' addressing; bf16 / f16 / f32; the first element of a
// row aligned to the element size only).  table[b] = {inv_t, tau, eta}; tau == 0: the sequence is off and nothing of it is read.
// With p = softmax(x * inv_t) of row (b, j) as it stands and s_v = -log2 p_v: v is cut (its logit becomes -inf) iff
// s_v > mu_{b,j} and x_v < x_max; with Z the kept mass and t the step's proposal at position j,
// mu_{b,j+1} = mu_{b,j} - eta (s_t + log2 Z - tau).  A proposal that is cut or -inf ends the chain: the rows behind it stay.
//
// Two launches, and the split is the design: everything that does not depend on mu runs on all B*K1 rows at once, and only
// what does sits on the dependent chain.
//   k_mirostat_lse    grid (K1, B), 1024 lanes per row: ONE sweep, the only read that goes to HBM, takes (m2, s) by the
//                     recurrences of lse_device.hpp and the exact maximum of the stored values: a lane meets its vectors in
//                     ascending order, lanes merge by the fixed DPP sequence, waves in wave order out of LDS; never arrival
//                     order.  One record {L.hi, L.lo, x_max, ok} per row goes to the workspace (L = m2 + log2 s, Norm2).
//   k_mirostat_chain  grid (B), 1024 lanes per SEQUENCE, rows j = 0 .. K1-1 in order: one sweep per row (served by L2 / MALL:
//                     the first launch has just read the row) compares log2 p_v = fma(x_v, c2, -L.hi) - L.lo with -mu -- the
//                     key of a token does not depend on which lane holds it --, adds 2^(log2 p_v) of the kept elements in the
//                     same fixed order, and stores a vector only where a bit of it changes.  The proposal's key comes from one
//                     scalar load ahead of the sweep.  The chain lives inside one workgroup: no spin-wait, no hand-off
//                     between workgroups, nothing can wait on a workgroup that is not resident.
//   k_mirostat_commit one thread per sequence, behind the step's commit: mu_b = mu_{b,n_acc} - eta (-lp / ln 2 - tau), and the
//                     mu in force at every committed token into a [B, max_len] buffer.

#include <hip/hip_runtime.h>

#include "top_logprobs_device.hpp"
#include "sample_device.hpp"

namespace asd {
namespace {

constexpr int kMiroThreads = 1024;
constexpr int kMiroWaves = kMiroThreads / 64;
constexpr int kMiroUnroll = 4;                   // 16-byte loads per lane in flight

struct MiroRec {
    float inv_t, tau, eta;
};
static_assert(sizeof(MiroRec) == ASD_MIROSTAT_REC_BYTES, "MiroRec");

// what the first launch leaves per row
struct __attribute__((aligned(16))) MiroRow {
    float l_hi, l_lo;                            // log2 of the normaliser, two floats
    float x_max;                                 // the exact maximum of the stored values
    int32_t ok;                                  // 0: a NaN or +inf element, no finite element, an overflow: the row stays
};
static_assert(sizeof(MiroRow) == ASD_MIROSTAT_ROW_BYTES, "MiroRow");

__device__ __forceinline__ bool miro_on(const MiroRec& r) {
    return r.tau > 0.0f && r.tau < 3.0e38f && r.eta > 0.0f && r.eta < 3.0e38f && r.inv_t > 0.0f && r.inv_t < 3.0e38f;
}

// a row as the sweeps walk it (entropy_cut.hip's walk): `head` scalar elements up to the first 16-byte boundary, nvec vectors,
// `tail` scalar elements
struct MiroWalk {
    char* rowp;
    char* body;
    int head, nvec, tail;
};
template <int DT>
__device__ __forceinline__ MiroWalk miro_walk(void* logits, int64_t ld_seq, int64_t ld_row, int b, int j, int V) {
    using E = Elem<DT>;
    MiroWalk r;
    r.rowp = static_cast<char*>(logits) + (static_cast<int64_t>(b) * ld_seq + static_cast<int64_t>(j) * ld_row) * E::kBytes;
    const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(r.rowp) & 15u);     // (a multiple of the element size)
    r.head = mis ? static_cast<int>((16u - mis) / E::kBytes) : 0;
    if (r.head > V) r.head = V;
    r.nvec = (V - r.head) / E::kPerVec;
    r.tail = V - r.head - r.nvec * E::kPerVec;
    r.body = r.rowp + static_cast<int64_t>(r.head) * E::kBytes;
    return r;
}

// one sweep: wave 0's lanes take the head and the tail, lane t the vectors t, t + 1024, ... in ascending order.
// fone(x) -> true: the element becomes -inf.  fvec(x[]) -> bit i set: element i becomes -inf.
template <int DT, bool kWrite, class FV, class F1>
__device__ __forceinline__ void miro_sweep(const MiroWalk& r, int tid, FV&& fvec, F1&& fone) {
    using E = Elem<DT>;
    constexpr int N = E::kPerVec;
    auto one = [&](int id) {
        const bool cut = fone(E::scalar(r.rowp, id));
        if constexpr (kWrite) {
            if (cut) {
                if constexpr (DT == ASD_DTYPE_F32) reinterpret_cast<uint32_t*>(r.rowp)[id] = E::kNegInfWord;
                else reinterpret_cast<uint16_t*>(r.rowp)[id] = static_cast<uint16_t>(E::kNegInfWord & 0xFFFFu);
            }
        }
    };
    if (tid < r.head) one(tid);
    const uint32_t end = static_cast<uint32_t>(r.nvec) * 16u;                        // launcher: V * element size < 2^31
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(r.body, 0, static_cast<int>(end), 0x00020000);
    for (uint32_t base = static_cast<uint32_t>(tid) * 16u; base < end; base += kMiroUnroll * kMiroThreads * 16u) {
        u32x4 vec[kMiroUnroll];
#pragma unroll
        for (int j = 0; j < kMiroUnroll; ++j) vec[j] = load16<false>(rsrc, base + static_cast<uint32_t>(j) * (kMiroThreads * 16u));
#pragma unroll
        for (int j = 0; j < kMiroUnroll; ++j) {
            const uint32_t off = base + static_cast<uint32_t>(j) * (kMiroThreads * 16u);
            if (off >= end) continue;                                                // (a load past the end returned zeros, unread)
            float x[N];
            unpack<DT>(vec[j], x);
            const uint32_t mask = fvec(x);
            if constexpr (kWrite) {
                if (mask == 0u) continue;
                u32x4 w = vec[j];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if constexpr (N == 8) {
                        if ((mask >> (2 * i)) & 1u) w[i] = (w[i] & 0xFFFF0000u) | (E::kNegInfWord & 0x0000FFFFu);
                        if ((mask >> (2 * i + 1)) & 1u) w[i] = (w[i] & 0x0000FFFFu) | (E::kNegInfWord & 0xFFFF0000u);
                    } else {
                        if ((mask >> i) & 1u) w[i] = E::kNegInfWord;
                    }
                }
                const bool same = w[0] == vec[j][0] && w[1] == vec[j][1] && w[2] == vec[j][2] && w[3] == vec[j][3];
                if (!same) *reinterpret_cast<u32x4*>(r.body + off) = w;              // only the vectors that change
            }
        }
    }
    if (tid < r.tail) one(r.head + r.nvec * N + tid);
}

template <int N>
__device__ __forceinline__ float tree_sum(const float (&e)[N]) {
    if constexpr (N == 8) return ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
    else return (e[0] + e[1]) + (e[2] + e[3]);
}

// ---- launch 1: the row's normaliser and maximum; blockIdx = (j, b)
template <int DT>
__global__ __launch_bounds__(kMiroThreads) void k_mirostat_lse(void* logits, int64_t ld_seq, int64_t ld_row, int K1, int V,
                                                               const MiroRec* __restrict__ table, MiroRow* __restrict__ rows) {
    using E = Elem<DT>;
    constexpr int N = E::kPerVec;
    __shared__ float meet[kMiroWaves][3];                                            // m2, s, x_max of every wave

    const int tid = static_cast<int>(threadIdx.x);
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int j = static_cast<int>(blockIdx.x);
    const int b = static_cast<int>(blockIdx.y);
    const MiroRec rec = table[b];                                                    // (uniform: scalar loads)
    if (!miro_on(rec)) return;                                                       // off: nothing of the row is read
    const float c2 = static_cast<float>(1.4426950408889634074 * static_cast<double>(rec.inv_t));   // log2_scale's own f64 product
    const MiroWalk r = miro_walk<DT>(logits, ld_seq, ld_row, b, j, V);

    float m2 = kSentinel, s = 0.0f, x_max = -INFINITY;
    miro_sweep<DT, false>(
        r, tid,
        [&](const float (&x)[N]) {                                                   // accum8 / accum4's operations, and the maximum
            float vmax;
            if constexpr (N == 8) vmax = fmaxf(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])), fmaxf(fmaxf(x[4], x[5]), fmaxf(x[6], x[7])));
            else vmax = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
            x_max = fmaxf(x_max, vmax);
            const float M = fmaxf(m2, vmax * c2);
            const float scale = fast_exp2(m2 - M);
            float e[N];
#pragma unroll
            for (int i = 0; i < N; ++i) e[i] = fast_exp2(fmaf(x[i], c2, -M));
            s = fmaf(s, scale, tree_sum<N>(e));
            m2 = M;
            return 0u;
        },
        [&](float x) {
            x_max = fmaxf(x_max, x);
            accum_scalar(x, c2, m2, s);
            return false;
        });
    wave_merge(m2, s);
    x_max = wave_max(x_max);
    if (lane == 0) {
        meet[wave][0] = m2;
        meet[wave][1] = s;
        meet[wave][2] = x_max;
    }
    __syncthreads();
    if (tid != 0) return;
    float rm2 = kSentinel, rs = 0.0f;
    x_max = -INFINITY;
#pragma unroll 1
    for (int w = 0; w < kMiroWaves; ++w) {                                           // wave order
        ms_merge(rm2, rs, meet[w][0], meet[w][1]);
        x_max = fmaxf(x_max, meet[w][2]);
    }
    // a NaN or +inf element (NaN sums), no finite element (s == 0), an overflow: the row has no distribution
    const bool ok = rs > 0.0f && rs < INFINITY && rm2 > kSentinel && x_max < INFINITY;
    const Norm2 L = norm2_of(rm2, ok ? rs : 1.0f);
    MiroRow out;
    out.l_hi = L.hi;
    out.l_lo = L.lo;
    out.x_max = x_max;
    out.ok = ok ? 1 : 0;
    rows[static_cast<int64_t>(b) * K1 + j] = out;                                    // (an ordinary 16-byte vector store)
}

// ---- launch 2: the chain of one sequence; blockIdx = b
template <int DT>
__global__ __launch_bounds__(kMiroThreads) void k_mirostat_chain(void* logits, int64_t ld_seq, int64_t ld_row, int K1, int V,
                                                                 const MiroRec* __restrict__ table, const MiroRow* __restrict__ rows,
                                                                 const float* __restrict__ mu_in, const int32_t* __restrict__ tok,
                                                                 int64_t ld_tok, float* __restrict__ mu_path) {
    using E = Elem<DT>;
    constexpr int N = E::kPerVec;
    __shared__ float meet[kMiroWaves];                                               // the kept mass of every wave

    const int tid = static_cast<int>(threadIdx.x);
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int b = static_cast<int>(blockIdx.x);
    const MiroRec rec = table[b];
    if (!miro_on(rec)) return;
    const float c2 = static_cast<float>(1.4426950408889634074 * static_cast<double>(rec.inv_t));
    float* const path = mu_path + static_cast<int64_t>(b) * K1;
    float mu = mu_in[b];                                                             // mu_{b,0}; uniform from here on

#pragma unroll 1
    for (int j = 0; j < K1; ++j) {
        if (tid == 0) path[j] = mu;                                                  // the mu in force at row j
        const MiroRow row = rows[static_cast<int64_t>(b) * K1 + j];
        if (row.ok == 0) continue;                                                   // rule 2: the row stays, mu passes through
        const MiroWalk r = miro_walk<DT>(logits, ld_seq, ld_row, b, j, V);
        const float thr = -mu;                                                       // cut iff log2 p_v < -mu
        const float l_hi = row.l_hi, l_lo = row.l_lo, x_max = row.x_max;
        auto key = [&](float x) { return fmaf(x, c2, -l_hi) - l_lo; };
        // the proposal's own key, from the row as it entered: read by every lane ahead of the barrier that opens the sweep
        bool has_t = false;
        float k_t = 0.0f, x_t = -INFINITY;
        if (j + 1 < K1) {
            const int t = tok[static_cast<int64_t>(b) * ld_tok + j];
            has_t = true;
            if (static_cast<uint32_t>(t) < static_cast<uint32_t>(V)) x_t = E::scalar(r.rowp, t);   // an id outside is never dereferenced
            k_t = key(x_t);
        }
        __syncthreads();                                                             // x_t is read; meet[] of the last row is read

        float z = 0.0f;
        miro_sweep<DT, true>(
            r, tid,
            [&](const float (&x)[N]) {
                uint32_t mask = 0u;
                float e[N];
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    const float k = key(x[i]);
                    const bool cut = k < thr && x[i] < x_max;
                    mask |= (cut ? 1u : 0u) << i;
                    e[i] = cut ? 0.0f : fast_exp2(k);
                }
                z += tree_sum<N>(e);
                return mask;
            },
            [&](float x) {
                const float k = key(x);
                const bool cut = k < thr && x < x_max;
                z += cut ? 0.0f : fast_exp2(k);
                return cut;
            });
        z = wave_sum(z);
        if (lane == 0) meet[wave] = z;
        __syncthreads();
        if (!has_t) break;                                                           // the last row: no proposal, nothing follows
        float Z = 0.0f;
#pragma unroll 1
        for (int w = 0; w < kMiroWaves; ++w) Z += meet[w];                           // wave order
        const bool t_cut = !(x_t > -INFINITY) || (k_t < thr && x_t < x_max);
        if (t_cut || !(Z > 0.0f)) {
            // rule 4: the proposal is rejected with certainty; the rows behind it can never commit and are left untouched
            for (int jj = j + 1 + tid; jj < K1; jj += kMiroThreads) path[jj] = mu;
            return;
        }
        const double s_hat = log2_split(Z) - static_cast<double>(k_t);               // the surprise under the cut distribution
        mu = static_cast<float>(static_cast<double>(mu) - static_cast<double>(rec.eta) * (s_hat - static_cast<double>(rec.tau)));
    }
}

// ---- behind the step's commit: one thread per sequence
__global__ void k_mirostat_commit(const float* __restrict__ mu_path, int K1, const int32_t* __restrict__ n_acc,
                                  const float* __restrict__ lp, const int32_t* __restrict__ seq_len,
                                  const int32_t* __restrict__ n_commit, const MiroRec* __restrict__ table, int B,
                                  float* __restrict__ mu, float* __restrict__ mu_out, int max_len) {
    const int b = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= B) return;
    const MiroRec rec = table[b];
    if (!miro_on(rec)) return;
    int a = n_acc[b];
    a = a < 0 ? 0 : (a > K1 - 1 ? K1 - 1 : a);
    int nc = n_commit[b];
    if (nc <= 0) return;                                                             // a finished sequence keeps its mu
    nc = nc > a + 1 ? a + 1 : nc;
    const float* const path = mu_path + static_cast<int64_t>(b) * K1;
    const int64_t first = static_cast<int64_t>(seq_len[b]) - nc;
    for (int i = 0; i < nc; ++i) {
        const int64_t pos = first + i;
        if (pos >= 0 && pos < max_len) mu_out[static_cast<int64_t>(b) * max_len + pos] = path[i];
    }
    if (nc != a + 1) return;                                                         // ended inside the accepted prefix: mu stays
    const float l = lp[b];
    if (!(l < INFINITY) || !(l > -INFINITY)) return;                                 // no log-prob (NaN, -inf), no move
    mu[b] = static_cast<float>(static_cast<double>(path[a]) -
                               static_cast<double>(rec.eta) * (-static_cast<double>(l) / kLn2d - static_cast<double>(rec.tau)));
}

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT int asd_mirostat_rows(void* logits, int dtype, int B, int K1, int V, int64_t ld_seq, int64_t ld_row,
                                 const asd_mirostat_rec* table, const float* mu, const int32_t* tok, int64_t ld_tok,
                                 float* mu_path, void* workspace, size_t workspace_bytes, void* stream) {
    if (B < 0 || K1 < 0 || V < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0 || K1 == 0 || V == 0) return ASD_OK;
    const int esz = dtype_size(dtype);
    if (esz == 0) return ASD_ERR_UNSUPPORTED;
    if (B > 65535 || K1 > ASD_MAX_DRAFT_LEN + 1) return ASD_ERR_UNSUPPORTED;         // grid (K1, B)
    if (static_cast<int64_t>(V) * esz > INT32_MAX) return ASD_ERR_UNSUPPORTED;       // the sweeps count bytes in 32 bits
    if (!logits || !table || !mu || !mu_path || !workspace) return ASD_ERR_INVALID_ARG;
    if (ld_row < V || ld_seq < static_cast<int64_t>(K1) * ld_row) return ASD_ERR_INVALID_ARG;
    if (K1 > 1 && (!tok || ld_tok < K1 - 1)) return ASD_ERR_INVALID_ARG;
    if (workspace_bytes < static_cast<size_t>(B) * static_cast<size_t>(K1) * ASD_MIROSTAT_ROW_BYTES) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(logits, static_cast<size_t>(esz)) || !aligned_to(table, 4) || !aligned_to(mu, 4) || !aligned_to(mu_path, 4) ||
        (tok && !aligned_to(tok, 4)) || !aligned_to(workspace, 16))
        return ASD_ERR_ALIGNMENT;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const MiroRec* const recs = reinterpret_cast<const MiroRec*>(table);
    MiroRow* const rows = static_cast<MiroRow*>(workspace);
    dispatch_dtype(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        hipLaunchKernelGGL((k_mirostat_lse<DT>), dim3(static_cast<uint32_t>(K1), static_cast<uint32_t>(B)), dim3(kMiroThreads), 0, st,
                           logits, ld_seq, ld_row, K1, V, recs, rows);
        hipLaunchKernelGGL((k_mirostat_chain<DT>), dim3(static_cast<uint32_t>(B)), dim3(kMiroThreads), 0, st, logits, ld_seq, ld_row,
                           K1, V, recs, rows, mu, tok, ld_tok, mu_path);
    });
    return launch_status();
}

ASD_EXPORT int asd_mirostat_commit(const float* mu_path, int B, int K1, const int32_t* n_acc, const float* lp,
                                   const int32_t* seq_len, const int32_t* n_commit, const asd_mirostat_rec* table, float* mu,
                                   float* mu_out, int max_len, void* stream) {
    if (B < 0 || K1 < 1 || max_len < 1) return ASD_ERR_INVALID_ARG;
    if (B == 0) return ASD_OK;
    if (!mu_path || !n_acc || !lp || !seq_len || !n_commit || !table || !mu || !mu_out) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(mu_path, 4) || !aligned_to(n_acc, 4) || !aligned_to(lp, 4) || !aligned_to(seq_len, 4) || !aligned_to(n_commit, 4) ||
        !aligned_to(table, 4) || !aligned_to(mu, 4) || !aligned_to(mu_out, 4))
        return ASD_ERR_ALIGNMENT;
    hipLaunchKernelGGL(k_mirostat_commit, dim3(static_cast<uint32_t>((B + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       mu_path, K1, n_acc, lp, seq_len, n_commit, reinterpret_cast<const MiroRec*>(table), B, mu, mu_out, max_len);
    return launch_status();
}
