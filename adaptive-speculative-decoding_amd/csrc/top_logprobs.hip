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

#include <hip/hip_runtime.h>

#define ASD_DPP_ASM_REDUCTIONS 1   // (this file is built with -ffp-contract=off, like greedy.hip)
#include "lse_device.hpp"

namespace asd {
namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kUnroll = 4;                     // 16-byte loads per lane and batch; two batches in flight
constexpr int kTop = ASD_MAX_TOP_LOGPROBS;
constexpr int kNoIndex = 0x7fffffff;
constexpr int kTicketStride = 16;              // u32 units: one 64-byte line per ticket
constexpr uint32_t kBatchBytes = static_cast<uint32_t>(kUnroll) * kThreads * 16u;
static_assert(kTop == 8, "the lists, the wave bound and the LDS layout are written for 8 entries");
static_assert(ASD_MAX_SPLITS <= 64, "one lane of the finisher's wave 0 per slice");

// 8 (value, id) pairs, value descending then id ascending; an empty slot is (-inf, kNoIndex).  Indexed by constants only.
struct Top {
    float v[kTop];
    int i[kTop];
};
struct __attribute__((aligned(16))) SlicePartial {
    float m2, s;
    float v[kTop];
    int i[kTop];
    int pad[2];
};
static_assert(sizeof(SlicePartial) == 80, "SlicePartial");

struct TopParams {
    const void* logits;
    int64_t ld_seq, ld_row;
    int K1, V, S, N;
    float c2;
    const float* inv_t;       // k_top_logprobs<DT, true> (asd_top_logprobs_rows): [B] per-sequence 1 / T; c2 unused
    int32_t* top_id;
    float* top_lp;
    uint32_t* row_tickets;
    SlicePartial* partials;
};

__device__ __forceinline__ void top_clear(Top& t) {
#pragma unroll
    for (int j = 0; j < kTop; ++j) { t.v[j] = -INFINITY; t.i[j] = kNoIndex; }
}

// x > t.v[7], and id is above every id of the list: x takes the last slot and rises while it is strictly greater
__device__ __forceinline__ void top_insert(Top& t, float x, int id) {
    t.v[kTop - 1] = x;
    t.i[kTop - 1] = id;
#pragma unroll
    for (int j = kTop - 1; j > 0; --j) {
        const bool up = t.v[j] > t.v[j - 1];
        const float hv = up ? t.v[j] : t.v[j - 1], lv = up ? t.v[j - 1] : t.v[j];
        const int hi = up ? t.i[j] : t.i[j - 1], li = up ? t.i[j - 1] : t.i[j];
        t.v[j - 1] = hv; t.v[j] = lv;
        t.i[j - 1] = hi; t.i[j] = li;
    }
}

// wave_max's DPP sequence on v_min_i32: a lane whose source is out of range keeps its value, the total lands in lane 63
__device__ __forceinline__ int wave_min_i32(int v) {
    asm("s_nop 1\n\t"
        "v_min_i32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_min_i32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_min_i32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_min_i32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_min_i32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_min_i32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "s_nop 0"
        : "+v"(v));
    return __builtin_amdgcn_readlane(v, 63);
}

// A lower bound of the wave's 8th best value from the lanes' heads: after row_shr 1, 2, 4 lane i holds the maximum of lanes
// i-7..i of its row of 16, so lanes 7, 15, ..., 63 hold the maxima of the eight 8-lane groups -- eight distinct elements.
// (heads are never NaN: a list only takes what compared `>`.)
__device__ __forceinline__ float wave_bound(float head) {
    asm("s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 0"
        : "+v"(head));
    const int h = __float_as_int(head);
    float b = __int_as_float(__builtin_amdgcn_readlane(h, 7));
#pragma unroll
    for (int g = 1; g < 8; ++g) b = fminf(b, __int_as_float(__builtin_amdgcn_readlane(h, 8 * g + 7)));
    return b;
}

// the lists of all 64 lanes -> the wave's 8 best, uniform in every lane; `t` is consumed.  ids are unique across the lanes, so
// exactly one lane pops per round (or every lane "pops" an empty list once nothing is left: harmless).
__device__ __forceinline__ void wave_top(Top& t, Top& out) {
#pragma unroll
    for (int r = 0; r < kTop; ++r) {
        const float wv = wave_max(t.v[0]);
        const int wi = wave_min_i32(t.v[0] == wv ? t.i[0] : kNoIndex);
        out.v[r] = wv;
        out.i[r] = wi;
        const bool pop = t.v[0] == wv && t.i[0] == wi;
#pragma unroll
        for (int j = 0; j + 1 < kTop; ++j) {
            t.v[j] = pop ? t.v[j + 1] : t.v[j];
            t.i[j] = pop ? t.i[j + 1] : t.i[j];
        }
        t.v[kTop - 1] = pop ? -INFINITY : t.v[kTop - 1];
        t.i[kTop - 1] = pop ? kNoIndex : t.i[kTop - 1];
    }
}

// one element (the scalar head and tail of a row)
__device__ __forceinline__ void accum_one(float x, int id, float c2, float& m2, float& s, Top& t) {
    if (x > t.v[kTop - 1]) top_insert(t, x, id);
    accum_scalar(x, c2, m2, s);
}

// one 16-byte vector whose first element has vocabulary id `id0`: greedy.hip's accum_arg with the list in place of the arg-max
// (fmaxf, not the bare v_max of lse_device.hpp, for the signalling-NaN reason given there; a NaN compares false and is skipped)
template <int N>
__device__ __forceinline__ void accum_top(const float (&x)[N], int id0, float c2, float& m2, float& s, Top& t, float bound) {
    float vmax;
    if constexpr (N == 8) vmax = fmaxf(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])), fmaxf(fmaxf(x[4], x[5]), fmaxf(x[6], x[7])));
    else vmax = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
    if (vmax > t.v[kTop - 1] && vmax >= bound) {
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (x[i] > t.v[kTop - 1] && x[i] >= bound) top_insert(t, x[i], id0 + i);
    }
    const float M = fmaxf(m2, vmax * c2);
    const float scale = fast_exp2(m2 - M);
    float e[N];
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = fast_exp2(fmaf(x[i], c2, -M));
    float sum;
    if constexpr (N == 8) sum = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
    else sum = (e[0] + e[1]) + (e[2] + e[3]);
    s = fmaf(s, scale, sum);
    m2 = M;
}

template <int DT>
__device__ __forceinline__ void accum_vec(const u32x4& v, int id0, float c2, float& m2, float& s, Top& t, float bound) {
    if constexpr (DT == ASD_DTYPE_BF16) {
        float x[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[2 * i] = __uint_as_float(v[i] << 16);
            x[2 * i + 1] = __uint_as_float(v[i] & 0xFFFF0000u);
        }
        accum_top<8>(x, id0, c2, m2, s, t, bound);
    } else if constexpr (DT == ASD_DTYPE_F16) {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        float x[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t w = v[i];
            const h2 h = __builtin_bit_cast(h2, w);
            x[2 * i] = static_cast<float>(h[0]);
            x[2 * i + 1] = static_cast<float>(h[1]);
        }
        accum_top<8>(x, id0, c2, m2, s, t, bound);
    } else {
        float x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = __uint_as_float(v[i]);
        accum_top<4>(x, id0, c2, m2, s, t, bound);
    }
}

// greedy.hip's row_logprob: lp = ln2 * (x c2 - (m2 + log2 s))
__device__ __forceinline__ float row_logprob(float x, float c2, double l2) {
    return static_cast<float>(kLn2d * (static_cast<double>(x) * static_cast<double>(c2) - l2));
}

// the (m2, s) pairs held by lanes 0 .. n-1 of this wave, combined in lane order from the neutral pair: uniform in every lane
__device__ __forceinline__ void merge_in_lane_order(float m2, float s, int n, float& rm2, float& rs) {
    rm2 = kSentinel;
    rs = 0.0f;
    for (int l = 0; l < n; ++l)
        ms_merge(rm2, rs, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m2), l)),
                 __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), l)));
}

// kRows (asd_top_logprobs_rows): the scale of sequence b is formed from inv_t[b] by log2_scale's own f64 product
template <int DT, bool kRows = false>
__global__ __launch_bounds__(kThreads) void k_top_logprobs(const TopParams p) {
    using E = Elem<DT>;
    __shared__ float meet_v[kWaves][kTop];
    __shared__ int meet_i[kWaves][kTop];
    __shared__ float meet_ms[kWaves][2];
    __shared__ int meet_last;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int S = p.S;
    const int K1 = p.K1;
    const int row = static_cast<int>(blockIdx.x);
    const int split = static_cast<int>(blockIdx.y);
    const int b = static_cast<int>(static_cast<uint32_t>(row) / static_cast<uint32_t>(K1));
    float c2 = p.c2;
    if constexpr (kRows)
        c2 = __int_as_float(__builtin_amdgcn_readfirstlane(
            __float_as_int(static_cast<float>(1.4426950408889634074 * static_cast<double>(p.inv_t[b])))));
    const int k = row - b * K1;

    const char* rowp = static_cast<const char*>(p.logits) + (static_cast<int64_t>(b) * p.ld_seq + static_cast<int64_t>(k) * p.ld_row) * E::kBytes;
    const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(rowp) & 15u);   // (a multiple of the element size: launcher)
    int head = mis ? static_cast<int>((16u - mis) / E::kBytes) : 0;
    if (head > p.V) head = p.V;
    const int nvec = (p.V - head) / E::kPerVec;
    const int tail = p.V - head - nvec * E::kPerVec;
    const char* body = rowp + static_cast<int64_t>(head) * E::kBytes;
    const int v0 = static_cast<int>(static_cast<uint64_t>(nvec) * static_cast<uint32_t>(split) / static_cast<uint32_t>(S));
    const int v1 = static_cast<int>(static_cast<uint64_t>(nvec) * static_cast<uint32_t>(split + 1) / static_cast<uint32_t>(S));

    float m2 = kSentinel, s = 0.0f;
    Top t;
    top_clear(t);
    if (wave == 0 && split == 0 && lane < head) accum_one(E::scalar(rowp, lane), lane, c2, m2, s, t);

    // ---- the stream: greedy.hip's (16-byte buffer loads through a descriptor that ends with the slice; the next batch is issued
    // before the current one is consumed); the wave's bound is refreshed behind every batch
    const uint32_t end = v1 > v0 ? static_cast<uint32_t>(v1 - v0) * 16u : 0u;       // launcher: V * element size < 2^31
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(body) + static_cast<int64_t>(v0) * 16, 0, static_cast<int>(end), 0x00020000);
    const uint32_t lane_off = static_cast<uint32_t>(tid) * 16u;
    const int id_first = head + v0 * E::kPerVec;
    float bound = -INFINITY;
    u32x4 cur[kUnroll], nxt[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) cur[j] = load16<true>(rsrc, lane_off + static_cast<uint32_t>(j) * (kThreads * 16u));
    for (uint32_t base = 0; base < end; base += kBatchBytes) {
#pragma unroll
        for (int j = 0; j < kUnroll; ++j)
            nxt[j] = load16<true>(rsrc, base + kBatchBytes + lane_off + static_cast<uint32_t>(j) * (kThreads * 16u));
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) {
            const uint32_t off = base + lane_off + static_cast<uint32_t>(j) * (kThreads * 16u);
            if (off < end) accum_vec<DT>(cur[j], id_first + static_cast<int>(off >> 4) * E::kPerVec, c2, m2, s, t, bound);
        }
        bound = wave_bound(t.v[0]);
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) cur[j] = nxt[j];
    }
    if (wave == 0 && split == S - 1 && lane < tail) {
        const int id = head + nvec * E::kPerVec + lane;
        accum_one(E::scalar(rowp, id), id, c2, m2, s, t);
    }

    // ---- lanes -> wave, waves -> workgroup (lane w of wave 0 takes wave w's list and pair out of LDS)
    Top w;
    wave_top(t, w);
    wave_merge(m2, s);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < kTop; ++j) { meet_v[wave][j] = w.v[j]; meet_i[wave][j] = w.i[j]; }
        meet_ms[wave][0] = m2;
        meet_ms[wave][1] = s;
    }
    __syncthreads();
    float rm2 = kSentinel, rs = 0.0f;
    if (wave == 0) {
        top_clear(t);
        m2 = kSentinel; s = 0.0f;
        if (lane < kWaves) {
#pragma unroll
            for (int j = 0; j < kTop; ++j) { t.v[j] = meet_v[lane][j]; t.i[j] = meet_i[lane][j]; }
            m2 = meet_ms[lane][0];
            s = meet_ms[lane][1];
        }
        wave_top(t, w);
        merge_in_lane_order(m2, s, kWaves, rm2, rs);
    }

    if (S > 1) {
        // ---- publish the slice; the workgroup that draws the row's last ticket combines all of them
        SlicePartial* const mine = p.partials + static_cast<int64_t>(row) * S;
        if (tid == 0) {
            SlicePartial q;
            q.m2 = rm2; q.s = rs;
#pragma unroll
            for (int j = 0; j < kTop; ++j) { q.v[j] = w.v[j]; q.i[j] = w.i[j]; }
            q.pad[0] = 0; q.pad[1] = 0;
            mine[split] = q;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const uint32_t old = __hip_atomic_fetch_add(p.row_tickets + static_cast<int64_t>(row) * kTicketStride, 1u, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT);
            const bool last = old == static_cast<uint32_t>(S - 1);
            if (last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            meet_last = last ? 1 : 0;
        }
        __syncthreads();
        if (meet_last == 0 || wave != 0) return;
        top_clear(t);
        m2 = kSentinel; s = 0.0f;
        if (lane < S) {                            // lane <-> slice: S <= 64
            const SlicePartial* const q = mine + lane;
#pragma unroll
            for (int j = 0; j < kTop; ++j) { t.v[j] = q->v[j]; t.i[j] = q->i[j]; }
            m2 = q->m2;
            s = q->s;
        }
        wave_top(t, w);
        merge_in_lane_order(m2, s, S, rm2, rs);    // slice order, not arrival order
    } else if (wave != 0) {
        return;
    }

    // ---- the row: wave 0 of the row's finisher holds (rm2, rs) and the 8 best, uniform; lane j writes slot j
    float mv = w.v[0];
    int mi = w.i[0];
#pragma unroll
    for (int j = 1; j < kTop; ++j) {
        mv = lane == j ? w.v[j] : mv;
        mi = lane == j ? w.i[j] : mi;
    }
    if (lane < p.N) {
        const double l2 = static_cast<double>(rm2) + log2_split(rs);
        const bool filled = mi != kNoIndex;
        const int64_t at = static_cast<int64_t>(row) * p.N + lane;
        p.top_id[at] = filled ? mi : -1;
        p.top_lp[at] = filled ? row_logprob(mv, c2, l2) : -INFINITY;
    }
}

// the workspace: the rows' tickets (one 64-byte line each: zeroed before every launch), then `splits` partials per row
struct Layout {
    size_t ticket_bytes, total;
};
inline Layout layout(int B, int K1, int splits) {
    const size_t R = static_cast<size_t>(B) * static_cast<size_t>(K1);
    Layout w{};
    w.ticket_bytes = round_up(R * kTicketStride * sizeof(uint32_t), 256);
    w.total = w.ticket_bytes + round_up(R * static_cast<size_t>(splits) * sizeof(SlicePartial), 256);
    return w;
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
