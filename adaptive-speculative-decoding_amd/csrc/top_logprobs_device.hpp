// top_logprobs_device.hpp -- the device parts of the row-streaming top-N pass, shared by top_logprobs.hip (the table alone),
// prompt_logprobs.hip (the table, plus the log-prob and the rank of one given token per row) and token_stats.hip (the table, the
// rank of the step's committed token and the row's entropy): the per-lane list, wave_bound, wave_top, the merges, the ticket
// hand-off and the workspace layout.  top_logprobs.hip's header describes them.  One row body,
// top_logprobs_row<DT, kRows, kMode>; what a mode adds stands under `if constexpr`, so kTopOnly is the pass as it was.
#pragma once

#include <hip/hip_runtime.h>

#define ASD_DPP_ASM_REDUCTIONS 1   // (both files are built with -ffp-contract=off, like greedy.hip)
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
    int count;                // kScore* / kStats: the slice's share of the target's rank; 0 otherwise
    int pad;                  // kStats: the bits of the slice's entropy sum u (below); 0 otherwise
};
static_assert(sizeof(SlicePartial) == 80, "SlicePartial");

// what the row body does beside the lse: the table alone (asd_top_logprobs), the table and one scored token per row, or the
// scored token alone (asd_prompt_logprobs with N >= 1 / N == 0: no list is kept)
// kStats / kStatsOnly (asd_token_stats with N >= 1 / N == 0): the rank of the row's committed token and the third running sum of
// the entropy, beside the table / beside the arg-max alone (slot 0 of a list of one: the same element, so the same bits)
constexpr int kTopOnly = 0, kScoreTop = 1, kScoreOnly = 2, kStats = 3, kStatsOnly = 4;
constexpr bool keeps_list(int mode) { return mode == kTopOnly || mode == kScoreTop || mode == kStats; }
constexpr bool keeps_stats(int mode) { return mode == kStats || mode == kStatsOnly; }

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
// asd_prompt_logprobs: K1 is T
struct PromptParams : TopParams {
    const int32_t* target;
    int64_t ld_target;
    const int32_t* first;     // [B] or nullptr
    float* lp;
    int32_t* rank;
};
// asd_token_stats: row j of sequence b is live while j <= a = clamp(n_acc[b], 0, K1 - 1) and scores tok[b, j] (j < a) or drawn[b]
struct StatsParams : TopParams {
    const int32_t* tok;       // [B, K1 - 1] or nullptr (K1 == 1)
    int64_t ld_tok;
    const int32_t* n_acc;     // [B]
    const int32_t* drawn;     // [B]
    int32_t* stat_id;         // [B, K1, 2]: rank, arg-max id
    float* stat_val;          // [B, K1, 2]: entropy (nats), log-prob of the arg-max
};

// the scored token of a row: its id and its stored value (both uniform: scalar registers), and the count of the elements that
// stand ahead of it in the table's order (value descending, then id ascending): `w` for the 16-byte vectors, counted per WAVE
// on the scalar unit, `n` for the scalar head and tail, per lane.  A NaN xg counts nothing; so does a NaN element.
struct Score {
    int g;
    float xg;
    int n;
    int w;
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

// the same sequence on v_add_u32: the total lands in lane 63
__device__ __forceinline__ int wave_sum_i32(int v) {
    asm("s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
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

// ---- kStats: the entropy's running sum.  Beside (m2, s) a partial carries u = sum_v e_v (x_v c2 - m2) with e_v = 2^(x_v c2 - m2),
// the terms of s weighted by their own exponents, so that H = -sum p ln p = ln2 (log2 s - u / s) at any m2.  The weights are
// differences from the running maximum (<= 0, and small where the mass is), which keeps the sum well conditioned when biases of
// +-100 have moved the logits; moving a partial from m2 to M >= m2 is u' = 2^(m2 - M) (u + (m2 - M) s).  An element without
// mass (e == 0: a -inf logit, or one that underflows) adds nothing: 0 * -inf never reaches the sum.  A NaN element makes s and
// u NaN.  The neutral partial is (kSentinel, 0, 0): kSentinel is finite, so (m2 - M) * 0 is 0.
__device__ __forceinline__ float rebase_u(float u, float s, float m2, float M, float scale) { return scale * fmaf(m2 - M, s, u); }
__device__ __forceinline__ void ms_merge_u(float& m2, float& s, float& u, float m2b, float sb, float ub) {
    const float M = fmaxf(m2, m2b);
    const float ea = fast_exp2(m2 - M);
    const float eb = fast_exp2(m2b - M);
    u = rebase_u(u, s, m2, M, ea) + rebase_u(ub, sb, m2b, M, eb);
    s = fmaf(s, ea, sb * eb);                      // (ms_merge's operations: the pair keeps its bits)
    m2 = M;
}
// wave_merge with the third sum: the same DPP order for u as for s
__device__ __forceinline__ void wave_merge_u(float& m2, float& s, float& u) {
    const float M = wave_max(m2);
    const float f = fast_exp2(m2 - M);
    u = wave_sum(rebase_u(u, s, m2, M, f));
    s = wave_sum(s * f);
    m2 = M;
}
// H in nats of a finished row: NaN when s == 0 (no finite logit) or when a NaN went in
__device__ __forceinline__ float row_entropy_u(float s, float u) {
    return static_cast<float>(kLn2d * (log2_split(s) - static_cast<double>(u) / static_cast<double>(s)));
}

// kStatsOnly: the lane's best element in slot 0.  A lane meets its ids in ascending order, so `>` keeps the lowest id of a tie;
// NaN and -inf never compare greater than the empty slot's -inf and are never taken, as in the list.
__device__ __forceinline__ void best_take(Top& t, float x, int id) {
    const bool up = x > t.v[0];
    t.v[0] = up ? x : t.v[0];
    t.i[0] = up ? id : t.i[0];
}
// the lanes' slot 0 -> the wave's, uniform in every lane: wave_top's first round; the other slots of `out` are empty
__device__ __forceinline__ void wave_best(const Top& t, Top& out) {
    top_clear(out);
    const float wv = wave_max(t.v[0]);
    out.v[0] = wv;
    out.i[0] = wave_min_i32(t.v[0] == wv ? t.i[0] : kNoIndex);
}
template <int kMode>
__device__ __forceinline__ void wave_reduce_top(Top& t, Top& out) {
    if constexpr (keeps_list(kMode)) wave_top(t, out);
    else if constexpr (kMode == kStatsOnly) wave_best(t, out);
    else top_clear(out);
}

// one element (the scalar head and tail of a row)
template <int kMode>
__device__ __forceinline__ void accum_one(float x, int id, float c2, float& m2, float& s, float& u, Top& t, Score& sc) {
    if constexpr (keeps_list(kMode)) {
        if (x > t.v[kTop - 1]) top_insert(t, x, id);
    }
    if constexpr (kMode == kStatsOnly) best_take(t, x, id);
    if constexpr (kMode != kTopOnly) sc.n += (x > sc.xg || (x == sc.xg && id < sc.g)) ? 1 : 0;
    if constexpr (keeps_stats(kMode)) {               // accum_scalar's operations on (m2, s), and the weighted term
        const float M = max2(m2, x * c2);
        const float scale = fast_exp2(m2 - M);
        const float d = fmaf(x, c2, -M);
        const float e = fast_exp2(d);
        u = fmaf(e, e > 0.0f ? d : 0.0f, rebase_u(u, s, m2, M, scale));
        s = fmaf(s, scale, e);
        m2 = M;
    } else {
        accum_scalar(x, c2, m2, s);
    }
}

// one 16-byte vector whose first element has vocabulary id `id0`: greedy.hip's accum_arg with the list in place of the arg-max
// (fmaxf, not the bare v_max of lse_device.hpp, for the signalling-NaN reason given there; a NaN compares false and is skipped)
//
// The count of a scored token (kScore*: called by EVERY lane of the wave, `live` false past the slice's end).  The wave's 64
// vectors hold 64 N consecutive ids from lane 0's id0 on.  A wave wholly below the token's id counts `>=`, one wholly above it
// `>`: one v_cmp into a scalar register pair per element, whose set bits the scalar unit counts and adds (s_bcnt1, s_add) -- no
// per-lane add, no VCC round trip.  The one wave-batch of the row that holds the token takes the order element by element.
template <int N, int kMode>
__device__ __forceinline__ void accum_top(const float (&x)[N], int id0, float c2, float& m2, float& s, float& u, Top& t,
                                          float bound, Score& sc, bool live) {
    if constexpr (kMode != kTopOnly) {
        const float xg = live ? sc.xg : __int_as_float(0x7fc00000);                // a dead lane counts nothing
        const int lo = __builtin_amdgcn_readfirstlane(id0);
        int w = 0;
        if (sc.g >= lo + 64 * N) {
#pragma unroll
            for (int i = 0; i < N; ++i) w += __builtin_popcountll(__builtin_amdgcn_ballot_w64(x[i] >= xg));
        } else if (sc.g < lo) {
#pragma unroll
            for (int i = 0; i < N; ++i) w += __builtin_popcountll(__builtin_amdgcn_ballot_w64(x[i] > xg));
        } else {
#pragma unroll
            for (int i = 0; i < N; ++i)
                w += __builtin_popcountll(__builtin_amdgcn_ballot_w64(x[i] > xg || (x[i] == xg && id0 + i < sc.g)));
        }
        sc.w += w;
        if (!live) return;
    }
    float vmax;
    if constexpr (N == 8) vmax = fmaxf(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])), fmaxf(fmaxf(x[4], x[5]), fmaxf(x[6], x[7])));
    else vmax = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
    if constexpr (keeps_list(kMode)) {
        if (vmax > t.v[kTop - 1] && vmax >= bound) {
#pragma unroll
            for (int i = 0; i < N; ++i)
                if (x[i] > t.v[kTop - 1] && x[i] >= bound) top_insert(t, x[i], id0 + i);
        }
    }
    if constexpr (kMode == kStatsOnly) {
        if (vmax > t.v[0]) {
#pragma unroll
            for (int i = 0; i < N; ++i) best_take(t, x[i], id0 + i);
        }
    }
    const float M = fmaxf(m2, vmax * c2);
    const float scale = fast_exp2(m2 - M);
    float e[N];
    if constexpr (keeps_stats(kMode)) {
        float w = 0.0f;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const float d = fmaf(x[i], c2, -M);
            e[i] = fast_exp2(d);
            w = fmaf(e[i], e[i] > 0.0f ? d : 0.0f, w);
        }
        u = rebase_u(u, s, m2, M, scale) + w;
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) e[i] = fast_exp2(fmaf(x[i], c2, -M));
    }
    float sum;
    if constexpr (N == 8) sum = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
    else sum = (e[0] + e[1]) + (e[2] + e[3]);
    s = fmaf(s, scale, sum);
    m2 = M;
}

template <int DT, int kMode>
__device__ __forceinline__ void accum_vec(const u32x4& v, int id0, float c2, float& m2, float& s, float& u, Top& t, float bound,
                                          Score& sc, bool live) {
    if constexpr (DT == ASD_DTYPE_BF16) {
        float x[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[2 * i] = __uint_as_float(v[i] << 16);
            x[2 * i + 1] = __uint_as_float(v[i] & 0xFFFF0000u);
        }
        accum_top<8, kMode>(x, id0, c2, m2, s, u, t, bound, sc, live);
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
        accum_top<8, kMode>(x, id0, c2, m2, s, u, t, bound, sc, live);
    } else {
        float x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = __uint_as_float(v[i]);
        accum_top<4, kMode>(x, id0, c2, m2, s, u, t, bound, sc, live);
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
__device__ __forceinline__ void merge_in_lane_order_u(float m2, float s, float u, int n, float& rm2, float& rs, float& ru) {
    rm2 = kSentinel;
    rs = 0.0f;
    ru = 0.0f;
    for (int l = 0; l < n; ++l)
        ms_merge_u(rm2, rs, ru, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m2), l)),
                   __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), l)),
                   __int_as_float(__builtin_amdgcn_readlane(__float_as_int(u), l)));
}

// The body of one workgroup: slice blockIdx.y of row blockIdx.x.  P is TopParams (kTopOnly), PromptParams (kScore*) or
// StatsParams (kStats).
// kRows (asd_top_logprobs_rows): the scale of sequence b is formed from inv_t[b] by log2_scale's own f64 product
template <int DT, bool kRows, int kMode, class P>
__device__ __forceinline__ void top_logprobs_row(const P& p) {
    using E = Elem<DT>;
    __shared__ float meet_v[kWaves][kTop];
    __shared__ int meet_i[kWaves][kTop];
    __shared__ float meet_ms[kWaves][2];
    __shared__ float meet_u[kWaves];               // (kStats)
    __shared__ int meet_count[kWaves];
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
    Score sc{0, 0.0f, 0, 0};
    bool scored = false;                           // g is inside [0, V) and x[g] is no NaN: the row has a log-prob and a rank
    if constexpr (keeps_stats(kMode)) {
        int a = p.n_acc[b];
        a = a < 0 ? 0 : (a > K1 - 1 ? K1 - 1 : a);
        if (k > a) {                                      // a row that is never committed (workgroup-uniform): neutral outputs, no pass
            if (split == 0) {
                if (tid == 0) {
                    p.stat_id[2 * static_cast<int64_t>(row)] = 0;
                    p.stat_id[2 * static_cast<int64_t>(row) + 1] = -1;
                    p.stat_val[2 * static_cast<int64_t>(row)] = 0.0f;
                    p.stat_val[2 * static_cast<int64_t>(row) + 1] = 0.0f;
                }
                if (tid < p.N) {
                    const int64_t at = static_cast<int64_t>(row) * p.N + tid;
                    p.top_id[at] = -1;
                    p.top_lp[at] = -INFINITY;
                }
            }
            return;
        }
        sc.g = __builtin_amdgcn_readfirstlane(k < a ? p.tok[static_cast<int64_t>(b) * p.ld_tok + k] : p.drawn[b]);
        const bool inside = static_cast<uint32_t>(sc.g) < static_cast<uint32_t>(p.V);     // an id outside is never dereferenced
        sc.xg = __int_as_float(__builtin_amdgcn_readfirstlane(
            __float_as_int(inside ? E::scalar(rowp, sc.g) : __int_as_float(0x7fc00000))));
        scored = sc.xg == sc.xg;
    } else if constexpr (kMode != kTopOnly) {
        if (p.first != nullptr && k < p.first[b]) {       // a skipped row (workgroup-uniform): neutral outputs, no pass
            if (split == 0) {
                if (tid == 0) { p.lp[row] = 0.0f; p.rank[row] = 0; }
                if (tid < p.N) {
                    const int64_t at = static_cast<int64_t>(row) * p.N + tid;
                    p.top_id[at] = -1;
                    p.top_lp[at] = -INFINITY;
                }
            }
            return;
        }
        sc.g = __builtin_amdgcn_readfirstlane(p.target[static_cast<int64_t>(b) * p.ld_target + k]);
        const bool inside = static_cast<uint32_t>(sc.g) < static_cast<uint32_t>(p.V);     // an id outside is never dereferenced
        sc.xg = __int_as_float(__builtin_amdgcn_readfirstlane(
            __float_as_int(inside ? E::scalar(rowp, sc.g) : __int_as_float(0x7fc00000))));
        scored = sc.xg == sc.xg;
    }
    const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(rowp) & 15u);   // (a multiple of the element size: launcher)
    int head = mis ? static_cast<int>((16u - mis) / E::kBytes) : 0;
    if (head > p.V) head = p.V;
    const int nvec = (p.V - head) / E::kPerVec;
    const int tail = p.V - head - nvec * E::kPerVec;
    const char* body = rowp + static_cast<int64_t>(head) * E::kBytes;
    const int v0 = static_cast<int>(static_cast<uint64_t>(nvec) * static_cast<uint32_t>(split) / static_cast<uint32_t>(S));
    const int v1 = static_cast<int>(static_cast<uint64_t>(nvec) * static_cast<uint32_t>(split + 1) / static_cast<uint32_t>(S));

    float m2 = kSentinel, s = 0.0f, u = 0.0f;      // (u: kStats)
    Top t;
    top_clear(t);
    if (wave == 0 && split == 0 && lane < head) accum_one<kMode>(E::scalar(rowp, lane), lane, c2, m2, s, u, t, sc);

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
            const int id0 = id_first + static_cast<int>(off >> 4) * E::kPerVec;
            if constexpr (kMode == kTopOnly) {
                if (off < end) accum_vec<DT, kMode>(cur[j], id0, c2, m2, s, u, t, bound, sc, true);
            } else {
                accum_vec<DT, kMode>(cur[j], id0, c2, m2, s, u, t, bound, sc, off < end);     // (the count is taken by the whole wave)
            }
        }
        if constexpr (keeps_list(kMode)) bound = wave_bound(t.v[0]);
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) cur[j] = nxt[j];
    }
    if (wave == 0 && split == S - 1 && lane < tail) {
        const int id = head + nvec * E::kPerVec + lane;
        accum_one<kMode>(E::scalar(rowp, id), id, c2, m2, s, u, t, sc);
    }

    // ---- lanes -> wave, waves -> workgroup (lane w of wave 0 takes wave w's list and pair out of LDS)
    Top w;
    wave_reduce_top<kMode>(t, w);
    if constexpr (keeps_stats(kMode)) wave_merge_u(m2, s, u);
    else wave_merge(m2, s);
    int count = 0;                                 // kScore*: uniform in wave 0 from here on
    if constexpr (kMode != kTopOnly) count = wave_sum_i32(sc.n) + sc.w;
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < kTop; ++j) { meet_v[wave][j] = w.v[j]; meet_i[wave][j] = w.i[j]; }
        meet_ms[wave][0] = m2;
        meet_ms[wave][1] = s;
        if constexpr (kMode != kTopOnly) meet_count[wave] = count;
        if constexpr (keeps_stats(kMode)) meet_u[wave] = u;
    }
    __syncthreads();
    float rm2 = kSentinel, rs = 0.0f, ru = 0.0f;
    if (wave == 0) {
        if constexpr (kMode != kTopOnly) count = wave_sum_i32(lane < kWaves ? meet_count[lane] : 0);
        top_clear(t);
        m2 = kSentinel; s = 0.0f; u = 0.0f;
        if (lane < kWaves) {
#pragma unroll
            for (int j = 0; j < kTop; ++j) { t.v[j] = meet_v[lane][j]; t.i[j] = meet_i[lane][j]; }
            m2 = meet_ms[lane][0];
            s = meet_ms[lane][1];
            if constexpr (keeps_stats(kMode)) u = meet_u[lane];
        }
        if constexpr (kMode != kScoreOnly) wave_reduce_top<kMode>(t, w);
        if constexpr (keeps_stats(kMode)) merge_in_lane_order_u(m2, s, u, kWaves, rm2, rs, ru);
        else merge_in_lane_order(m2, s, kWaves, rm2, rs);
    }

    if (S > 1) {
        // ---- publish the slice; the workgroup that draws the row's last ticket combines all of them
        SlicePartial* const mine = p.partials + static_cast<int64_t>(row) * S;
        if (tid == 0) {
            SlicePartial q;
            q.m2 = rm2; q.s = rs;
#pragma unroll
            for (int j = 0; j < kTop; ++j) { q.v[j] = w.v[j]; q.i[j] = w.i[j]; }
            q.count = count; q.pad = 0;
            if constexpr (keeps_stats(kMode)) q.pad = __float_as_int(ru);
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
        m2 = kSentinel; s = 0.0f; u = 0.0f;
        if (lane < S) {                            // lane <-> slice: S <= 64
            const SlicePartial* const q = mine + lane;
#pragma unroll
            for (int j = 0; j < kTop; ++j) { t.v[j] = q->v[j]; t.i[j] = q->i[j]; }
            m2 = q->m2;
            s = q->s;
            if constexpr (kMode != kTopOnly) count = q->count;
            if constexpr (keeps_stats(kMode)) u = __int_as_float(q->pad);
        } else {
            count = 0;
        }
        if constexpr (kMode != kScoreOnly) wave_reduce_top<kMode>(t, w);
        if constexpr (keeps_stats(kMode)) merge_in_lane_order_u(m2, s, u, S, rm2, rs, ru);
        else merge_in_lane_order(m2, s, S, rm2, rs);    // slice order, not arrival order
        if constexpr (kMode != kTopOnly) count = wave_sum_i32(count);
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
    if constexpr (keeps_stats(kMode)) {
        if (lane == 0) {                           // slot 0 again (the table may have N == 0), the rank and the entropy
            const double l2 = static_cast<double>(rm2) + log2_split(rs);
            const bool filled = mi != kNoIndex;
            p.stat_id[2 * static_cast<int64_t>(row)] = scored ? 1 + count : 0;
            p.stat_id[2 * static_cast<int64_t>(row) + 1] = filled ? mi : -1;
            p.stat_val[2 * static_cast<int64_t>(row)] = row_entropy_u(rs, ru);
            p.stat_val[2 * static_cast<int64_t>(row) + 1] = filled ? row_logprob(mv, c2, l2) : -INFINITY;
        }
    } else if constexpr (kMode != kTopOnly) {
        if (lane == 0) {                           // a slot's own operations on x[g]: the bits of a slot that holds g
            const double l2 = static_cast<double>(rm2) + log2_split(rs);
            p.lp[row] = scored ? row_logprob(sc.xg, c2, l2) : __int_as_float(0x7fc00000);
            p.rank[row] = scored ? 1 + count : 0;
        }
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
