// watermark.hip -- the green-list text watermark of Kirchenbauer et al. 2023 ("A Watermark for Large Language Models"; HF
// generate's WatermarkingConfig: greenlist_ratio, bias, hashing_key, context_width) ahead of the samplers, and the counting
// half of its detector, gfx950 / wave64.  HF draws the green list from torch.randperm under a seeded generator, which no kernel
// can restate; the predicate here is this library's own, keyed by Philox4x32-10 (philox.hip's generator).
//
// THE PREDICATE.  A sequence has a 64-bit key (k_lo, k_hi), a context width h in 1..3 and a threshold thr in 1..65535.  At a
// position with history H let a = H[-1], b = H[-2] (h >= 2, else 0xFFFFFFFF), c = H[-3] (h == 3, else 0xFFFFFFFF).  Token v is
// GREEN iff halfword v & 7 of philox4x32_10(counter = (v >> 3, a, b, c), key = (k_lo, k_hi)) is < thr; halfword i is word
// i >> 1, bits 0..15 for even i and 16..31 for odd i.  One call serves eight consecutive token ids.
//
// asd_watermark_rows: logits[b][j][v] lies at b*ld_seq + j*ld_row + v (asd_dry_rows' addressing and history arguments; bf16 /
// f16 / f32; the base aligned to the element size only).  Record b = {key_lo, key_hi, delta, thr | h << 16}.  Every FINITE
// green element becomes round_dtype(fl32(x) + delta): nearest even, a result that leaves the dtype's range becomes its largest
// finite value.  -inf, +inf, NaN, the other elements and the padding behind V keep their bits; 16 bytes are stored only where
// a bit of them changes.  thr == 0: the row is off and is not read; h outside 1..3, a delta that is not finite and positive:
// damaged data, the row is skipped; a history shorter than h: nothing is written.
//
// GEOMETRY.  The pass has no reduction: no LDS, no barrier, no atomics, nothing shared between workgroups.  The work item is
// the UNIT of eight elements: one 16-byte vector in 16 bits, two ADJACENT vectors in f32 -- what one Philox call serves.  A row
// is a head of up to 7 scalar elements in front of the first 16-byte boundary, nunit units and a tail of up to 7 elements.  A
// workgroup is 256 lanes and owns a contiguous range of a row's units, a multiple of 256 long; lane t takes the units t,
// t + 256, ... of it, four at a time: the 4 (f32: 8) loads of a step are issued ahead of its first Philox call, so the integer
// work runs under the memory latency.  The launcher cuts every row into `splits` ranges, splits = floor(8 * CUs / (B * K1))
// clamped into [1, ceil(nunit / 256)]: B * K1 = 1 at V = 152064 is 75 workgroups with one unit per lane, B * K1 = 288 is 7 per
// row, 2016 in all, which is what the CUs hold at once (8 workgroups of 256 lanes each at <= 64 registers).  The record and the
// up to three context tokens are uniform in a workgroup: scalar loads, once.  Split 0's wave 0 takes the head and its wave 1
// the tail, one Philox call per element.
// ALIGNMENT.  Where every row's body starts at a token id that is a multiple of 8 -- a 16-byte aligned base with ld_seq and
// ld_row multiples of 16 bytes; the launcher decides -- a unit IS one Philox group: one call per unit, and in 16 bits the
// halfwords are compared in place, word i of the call against word i of the vector.  Otherwise a unit straddles two groups:
// the kernel makes TWO calls per unit, forms the two 8-bit green masks and shifts the 16 bits right by the row's offset.  A
// realignment through a neighbour lane would halve that; misaligned logits are the exception, so the plain form was chosen.
// The two forms give the same bits for the same row.
// ARITHMETIC.  A Philox round is two 32 x 32 -> 64 products; the key schedule and, in round 1, M1 * b are uniform.  Ten rounds
// are 19 per-lane products (v_mad_u64_u32 or a v_mul_lo / v_mul_hi pair: the compiler's choice) and 20 xors, per eight
// elements; the edit is one f32 add, one min against the dtype's largest finite value (which is the clamp) and the rounding (bf16: gfx950's
// v_cvt_pk_bf16_f32, two elements per issue; f16: v_cvt_f16_f32).
//
// asd_watermark_score: out[b] = {n_scored, n_green} over the positions i of tokens[b] in [max(row_from, row_start + h),
// seq_len) -- one wave per sequence, lanes over positions, one Philox call per position for the group that holds tokens[b][i],
// the lanes' counts merged by the DPP sequence of top_logprobs_device.hpp.  No workspace.

#include <hip/hip_runtime.h>

#include <float.h>

#include "top_logprobs_device.hpp"

namespace asd {
namespace {

constexpr int kWmThreads = 256;
constexpr int kWmUnroll = 4;                     // units of a lane whose loads are in flight together
constexpr int kWmGroupsPerCu = 8;                // 256-lane workgroups a CU holds at <= 64 registers
constexpr int kScoreThreads = 64;
constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;
constexpr uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
constexpr uint32_t kNoToken = 0xFFFFFFFFu;       // the filler of a context narrower than 3: no token id is negative

struct WmRec {
    uint32_t key_lo, key_hi;
    float delta;
    uint32_t thr_h;                              // thr | h << 16
};
static_assert(sizeof(WmRec) == ASD_WATERMARK_REC_BYTES, "WmRec");

// what a workgroup knows about its row: uniform, in scalar registers
struct WmCtx {
    uint32_t a, b, c, k0, k1, thr;
    float delta;
};

// philox.hip's rounds on (g, a, b, c): w[0..3] hold the halfwords of token ids 8g .. 8g + 7
__device__ __forceinline__ void wm_philox(uint32_t g, const WmCtx& x, uint32_t (&w)[4]) {
    uint32_t c0 = g, c1 = x.a, c2 = x.b, c3 = x.c, k0 = x.k0, k1 = x.k1;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = static_cast<uint64_t>(kM0) * c0, p1 = static_cast<uint64_t>(kM1) * c2;
        const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0, n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
        c1 = static_cast<uint32_t>(p1);
        c3 = static_cast<uint32_t>(p0);
        c0 = n0;
        c2 = n2;
        k0 += kW0;
        k1 += kW1;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// bit i: token 8g + i is green
__device__ __forceinline__ uint32_t wm_mask8(const uint32_t (&w)[4], uint32_t thr) {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        m |= ((w[i] & 0xFFFFu) < thr ? 1u : 0u) << (2 * i);
        m |= ((w[i] >> 16) < thr ? 1u : 0u) << (2 * i + 1);
    }
    return m;
}

// the green bits of the eight token ids t0 .. t0 + 7; s = t0 & 7 is the row's offset (uniform)
__device__ __forceinline__ uint32_t wm_unit_mask(uint32_t t0, uint32_t s, const WmCtx& x) {
    uint32_t w[4];
    wm_philox(t0 >> 3, x, w);
    uint32_t m = wm_mask8(w, x.thr);
    if (s != 0) {                                // the unit straddles two groups: the second call
        wm_philox((t0 >> 3) + 1u, x, w);
        m = (m | (wm_mask8(w, x.thr) << 8)) >> s;
    }
    return m;
}

__device__ __forceinline__ bool wm_green_one(uint32_t v, const WmCtx& x) {
    uint32_t w[4];
    wm_philox(v >> 3, x, w);
    const uint32_t q = (v >> 1) & 3u;
    const uint32_t word = q == 0 ? w[0] : (q == 1 ? w[1] : (q == 2 ? w[2] : w[3]));
    return ((v & 1u) ? word >> 16 : word & 0xFFFFu) < x.thr;
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

template <int DT>
constexpr float kWmMax = FLT_MAX;                // the dtype's largest finite value
template <>
constexpr float kWmMax<ASD_DTYPE_BF16> = 3.3895313892515355e+38f;
template <>
constexpr float kWmMax<ASD_DTYPE_F16> = 65504.0f;

// Two results, each finite or +inf, -> one word of two 16-bit elements: to nearest even, a result beyond the range -> the
// largest finite value.  The minimum in front IS that clamp: what lies above the largest finite value rounds to it or to inf.
// bf16 by gfx950's v_cvt_pk_bf16_f32, f16 by v_cvt_f16_f32: nearest even both (the mode register's default).
template <int DT>
__device__ __forceinline__ uint32_t wm_round2(float y0, float y1) {
    const f32x2 y = {__builtin_fminf(y0, kWmMax<DT>), __builtin_fminf(y1, kWmMax<DT>)};
    if constexpr (DT == ASD_DTYPE_BF16) return __builtin_bit_cast(uint32_t, __builtin_convertvector(y, bf16x2));
    else return __builtin_bit_cast(uint32_t, __builtin_convertvector(y, f16x2));
}

// one word of two 16-bit elements -> its new bits; g0 / g1: the elements are green.  x finite and delta > 0: x + delta is
// finite or +inf, never NaN
template <int DT>
__device__ __forceinline__ uint32_t wm_edit2(uint32_t old, bool g0, bool g1, float delta) {
    using E = Elem<DT>;
    const float x0 = E::from_raw(old & 0xFFFFu), x1 = E::from_raw(old >> 16);
    const uint32_t now = wm_round2<DT>(x0 + delta, x1 + delta);
    const uint32_t take = (g0 && fabsf(x0) < INFINITY ? 0x0000FFFFu : 0u) | (g1 && fabsf(x1) < INFINITY ? 0xFFFF0000u : 0u);
    return (old & ~take) | (now & take);
}

__device__ __forceinline__ uint32_t wm_edit1(uint32_t old, bool green, float delta) {       // one f32 element
    const float x = __uint_as_float(old);
    return green && fabsf(x) < INFINITY ? __float_as_uint(__builtin_fminf(x + delta, FLT_MAX)) : old;
}

template <int DT>
__device__ __forceinline__ void wm_one(char* rowp, int id, const WmCtx& x) {
    using E = Elem<DT>;
    const uint32_t old = E::raw(rowp, id);
    const bool green = wm_green_one(static_cast<uint32_t>(id), x);
    if constexpr (DT == ASD_DTYPE_F32) {
        const uint32_t now = wm_edit1(old, green, x.delta);
        if (now != old) reinterpret_cast<uint32_t*>(rowp)[id] = now;
    } else {
        const uint32_t now = wm_edit2<DT>(old, green, false, x.delta);
        if (now != old) reinterpret_cast<uint16_t*>(rowp)[id] = static_cast<uint16_t>(now);
    }
}

// a unit in 16 bits: one vector, token ids t0 .. t0 + 7
template <int DT, bool kAligned>
__device__ __forceinline__ void wm_unit16(char* at, const u32x4& v, uint32_t t0, uint32_t s, const WmCtx& x) {
    bool g[8];
    if constexpr (kAligned) {                    // the unit is the group: the call's halfwords against thr, word by word
        uint32_t w[4];
        wm_philox(t0 >> 3, x, w);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            g[2 * i] = (w[i] & 0xFFFFu) < x.thr;
            g[2 * i + 1] = (w[i] >> 16) < x.thr;
        }
    } else {
        const uint32_t m = wm_unit_mask(t0, s, x);
#pragma unroll
        for (int i = 0; i < 8; ++i) g[i] = (m >> i) & 1u;
    }
    u32x4 out;
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = wm_edit2<DT>(v[i], g[2 * i], g[2 * i + 1], x.delta);
    const bool same = out[0] == v[0] && out[1] == v[1] && out[2] == v[2] && out[3] == v[3];
    if (!same) *reinterpret_cast<u32x4*>(at) = out;
}

// a unit in f32: two adjacent vectors, token ids t0 .. t0 + 7, each stored where a bit of it changes
__device__ __forceinline__ void wm_unit32(char* at, const u32x4& v0, const u32x4& v1, uint32_t t0, uint32_t s, const WmCtx& x) {
    const uint32_t m = wm_unit_mask(t0, s, x);
    u32x4 o0, o1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        o0[i] = wm_edit1(v0[i], (m >> i) & 1u, x.delta);
        o1[i] = wm_edit1(v1[i], (m >> (4 + i)) & 1u, x.delta);
    }
    if (!(o0[0] == v0[0] && o0[1] == v0[1] && o0[2] == v0[2] && o0[3] == v0[3])) *reinterpret_cast<u32x4*>(at) = o0;
    if (!(o1[0] == v1[0] && o1[1] == v1[1] && o1[2] == v1[2] && o1[3] == v1[3])) *reinterpret_cast<u32x4*>(at + 16) = o1;
}

template <int DT, bool kAligned>
__global__ __launch_bounds__(kWmThreads) void k_watermark_rows(void* logits, int64_t ld_seq, int64_t ld_row, int K1, int V, int splits,
                                                               const WmRec* __restrict__ recs,
                                                               const int32_t* __restrict__ row_start,
                                                               const int32_t* __restrict__ tokens, int64_t ld_tokens,
                                                               const int32_t* __restrict__ seq_len, int start, int max_len,
                                                               const int32_t* __restrict__ step_tok, int64_t ld_tok, int n_prev) {
    using E = Elem<DT>;
    constexpr bool kWide = DT == ASD_DTYPE_F32;
    constexpr uint32_t kUnitBytes = 8u * E::kBytes;
    const int tid = static_cast<int>(threadIdx.x);
    const uint32_t row = blockIdx.x / static_cast<uint32_t>(splits);
    const uint32_t split = blockIdx.x - row * static_cast<uint32_t>(splits);
    const int b = static_cast<int>(row / static_cast<uint32_t>(K1));
    const int j = static_cast<int>(row) - b * K1;

    // ---- the record and the context: uniform, fetched once per workgroup
    WmCtx x;
    x.thr = recs[b].thr_h & 0xFFFFu;
    const int h = static_cast<int>(recs[b].thr_h >> 16);
    if (x.thr == 0 || h < 1 || h > 3) return;                // off; damaged
    x.delta = recs[b].delta;
    if (!(x.delta > 0.0f && x.delta < INFINITY)) return;     // damaged (NaN included)
    x.k0 = recs[b].key_lo;
    x.k1 = recs[b].key_hi;
    int L = seq_len[b];
    L = L < start ? start : (L > max_len ? max_len : L);     // start <= max_len <= ld_tokens: the launcher's checks
    int first = start;
    if (row_start) {
        first = row_start[b];
        first = first < 0 ? 0 : (first > start ? start : first);
    }
    const int n_com = L - first;                             // real prompt ids and committed tokens: one run of `tokens`
    const int n_see = step_tok ? n_prev + j : 0;             // n_prev + K1 - 1 <= n_tok <= ld_tok: the launcher's
    const int len = n_com + n_see;                           // <= max_len + n_tok <= INT32_MAX: the launcher's
    if (len < h) return;
    const int32_t* const committed = tokens + static_cast<int64_t>(b) * ld_tokens + first;
    const int64_t proposed = static_cast<int64_t>(b) * ld_tok - n_com;
    auto hist = [&](int p) -> uint32_t {                     // H[p], 0 <= len - 3 <= p < len
        return static_cast<uint32_t>(p < n_com ? committed[p] : step_tok[proposed + p]);
    };
    x.a = hist(len - 1);
    x.b = h >= 2 ? hist(len - 2) : kNoToken;
    x.c = h == 3 ? hist(len - 3) : kNoToken;

    // ---- the row: head, units, tail
    char* const rowp = static_cast<char*>(logits) + (static_cast<int64_t>(b) * ld_seq + static_cast<int64_t>(j) * ld_row) * E::kBytes;
    int head = 0;
    if constexpr (!kAligned) {
        const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(rowp) & 15u);   // (a multiple of the element size)
        head = mis ? static_cast<int>((16u - mis) / E::kBytes) : 0;
        if (head > V) head = V;
    }
    const uint32_t nunit = static_cast<uint32_t>(V - head) >> 3;
    const int tail = V - head - static_cast<int>(nunit << 3);
    char* const body = rowp + static_cast<int64_t>(head) * E::kBytes;
    const uint32_t s = static_cast<uint32_t>(head) & 7u;     // the body's first token id modulo 8

    if (split == 0) {                                        // the scalar elements: wave 0 the head, wave 1 the tail
        if (tid < head) wm_one<DT>(rowp, tid, x);
        else if (tid >= 64 && tid < 64 + tail) wm_one<DT>(rowp, head + static_cast<int>(nunit << 3) + tid - 64, x);
    }

    // ---- this workgroup's range of units [lo, hi): a multiple of 256 long; V * element size < 2^31: the launcher's
    const uint32_t nsplit = static_cast<uint32_t>(splits);
    const uint32_t per = ((nunit + nsplit - 1u) / nsplit + kWmThreads - 1u) / kWmThreads * kWmThreads;
    const uint32_t lo = split * per;
    const uint32_t hi = lo + per < nunit ? lo + per : nunit;
    if (lo >= hi) return;
    // (a lane whose offset is >= hi units gets zeros and makes no memory access)
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(body, 0, static_cast<int>(hi * kUnitBytes), 0x00020000);
    for (uint32_t q0 = lo + static_cast<uint32_t>(tid); q0 < hi; q0 += kWmUnroll * kWmThreads) {
        u32x4 v[kWmUnroll][kWide ? 2 : 1];
#pragma unroll
        for (int i = 0; i < kWmUnroll; ++i) {                // every load of the step ahead of its first Philox call
            const uint32_t off = (q0 + static_cast<uint32_t>(i) * kWmThreads) * kUnitBytes;
            v[i][0] = load16<false>(rsrc, off);
            if constexpr (kWide) v[i][1] = load16<false>(rsrc, off + 16u);
        }
#pragma unroll
        for (int i = 0; i < kWmUnroll; ++i) {
            const uint32_t q = q0 + static_cast<uint32_t>(i) * kWmThreads;
            if (q >= hi) break;
            const uint32_t t0 = static_cast<uint32_t>(head) + (q << 3);
            if constexpr (kWide) wm_unit32(body + q * kUnitBytes, v[i][0], v[i][1], t0, s, x);
            else wm_unit16<DT, kAligned>(body + q * kUnitBytes, v[i][0], t0, s, x);
        }
    }
}

__global__ __launch_bounds__(kScoreThreads) void k_watermark_score(const int32_t* __restrict__ tokens, int64_t ld_tokens,
                                                                   const int32_t* __restrict__ row_start,
                                                                   const int32_t* __restrict__ row_from,
                                                                   const int32_t* __restrict__ seq_len, int max_len,
                                                                   const WmRec* __restrict__ recs, int32_t* __restrict__ out) {
    const int lane = static_cast<int>(threadIdx.x);
    const int b = static_cast<int>(blockIdx.x);
    WmCtx x;
    x.thr = recs[b].thr_h & 0xFFFFu;
    const int h = static_cast<int>(recs[b].thr_h >> 16);
    x.k0 = recs[b].key_lo;
    x.k1 = recs[b].key_hi;
    x.delta = 0.0f;
    int n = 0, green = 0;
    if (x.thr != 0 && h >= 1 && h <= 3) {                    // (uniform) else off or damaged: {0, 0}
        int L = seq_len[b];
        L = L < 0 ? 0 : (L > max_len ? max_len : L);         // max_len <= ld_tokens: the launcher's check
        int first = row_start ? row_start[b] : 0;
        first = first < 0 ? 0 : (first > L ? L : first);
        int from = row_from[b];
        from = from < first ? first : (from > L ? L : from);
        const int lo = from > first + h ? from : first + h;  // the first position with h tokens at or behind row_start in front
        n = L > lo ? L - lo : 0;
        const int32_t* const t = tokens + static_cast<int64_t>(b) * ld_tokens;
        for (int i = lo + lane; i < L; i += kScoreThreads) {
            x.a = static_cast<uint32_t>(t[i - 1]);
            x.b = h >= 2 ? static_cast<uint32_t>(t[i - 2]) : kNoToken;
            x.c = h == 3 ? static_cast<uint32_t>(t[i - 3]) : kNoToken;
            green += wm_green_one(static_cast<uint32_t>(t[i]), x) ? 1 : 0;
        }
        green = wave_sum_i32(green);
    }
    if (lane == 0) {
        out[2 * b] = n;
        out[2 * b + 1] = green;
    }
}

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT int asd_watermark_rows(void* logits, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V,
                                  const asd_watermark_rec* recs, const int32_t* row_start, const int32_t* tokens, int64_t ld_tokens,
                                  const int32_t* seq_len, int start, int max_len, const int32_t* step_tok, int64_t ld_tok, int n_tok,
                                  int n_prev, void* stream) {
    if (B < 0 || K1 < 0 || V < 0 || n_tok < 0 || n_prev < 0 || start < 0 || max_len < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0 || K1 == 0 || V == 0) return ASD_OK;
    const int esz = dtype_size(dtype);
    if (esz == 0) return ASD_ERR_UNSUPPORTED;
    if (n_tok > ASD_MAX_DRAFT_LEN) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(B) * K1 > INT32_MAX) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(max_len) + n_tok > INT32_MAX) return ASD_ERR_UNSUPPORTED;          // the history's length is an int32
    if (static_cast<int64_t>(V) * esz > INT32_MAX) return ASD_ERR_UNSUPPORTED;                  // the body counts bytes in 32 bits
    if (!logits || !recs || !tokens || !seq_len) return ASD_ERR_INVALID_ARG;
    if (ld_row < V || ld_seq < static_cast<int64_t>(K1) * ld_row || ld_tokens < max_len || start > max_len) return ASD_ERR_INVALID_ARG;
    if (!step_tok && n_prev != 0) return ASD_ERR_INVALID_ARG;
    if (step_tok && (static_cast<int64_t>(n_prev) + K1 - 1 > n_tok || ld_tok < n_tok)) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(logits, static_cast<size_t>(esz)) || !aligned_to(recs, 4) || !aligned_to(row_start, 4) || !aligned_to(tokens, 4) ||
        !aligned_to(seq_len, 4) || !aligned_to(step_tok, 4))
        return ASD_ERR_ALIGNMENT;
    // the grid from B * K1 and V: what the CUs hold at once, a row cut into at most ceil(nunit / 256) ranges
    const int64_t rows = static_cast<int64_t>(B) * K1;
    const int64_t most = (V / 8 + kWmThreads - 1) / kWmThreads;
    int64_t splits = static_cast<int64_t>(current_device_cus()) * kWmGroupsPerCu / rows;
    splits = splits > most ? most : splits;
    splits = splits < 1 ? 1 : splits;                                                           // rows * splits < 2^32
    const bool aligned = rows_aligned(logits, ld_row, esz) && (ld_seq * esz) % 16 == 0;         // every row starts a Philox group
    const dim3 grid(static_cast<uint32_t>(rows * splits));
    dispatch_dtype(dtype, [&](auto dt) {
        dispatch_bool(aligned, [&](auto al) {
            hipLaunchKernelGGL((k_watermark_rows<decltype(dt)::value, decltype(al)::value>), grid, dim3(kWmThreads), 0,
                               static_cast<hipStream_t>(stream), logits, ld_seq, ld_row, K1, V, static_cast<int>(splits),
                               reinterpret_cast<const WmRec*>(recs), row_start, tokens, ld_tokens, seq_len, start, max_len, step_tok,
                               ld_tok, n_prev);
        });
    });
    return launch_status();
}

ASD_EXPORT int asd_watermark_score(const int32_t* tokens, int64_t ld_tokens, const int32_t* row_start, const int32_t* row_from,
                                   const int32_t* seq_len, int B, int max_len, const asd_watermark_rec* recs, int32_t* out,
                                   void* stream) {
    if (B < 0 || max_len < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0) return ASD_OK;
    if (!tokens || !row_from || !seq_len || !recs || !out || ld_tokens < max_len) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(tokens, 4) || !aligned_to(row_start, 4) || !aligned_to(row_from, 4) || !aligned_to(seq_len, 4) ||
        !aligned_to(recs, 4) || !aligned_to(out, 4))
        return ASD_ERR_ALIGNMENT;
    hipLaunchKernelGGL(k_watermark_score, dim3(static_cast<uint32_t>(B)), dim3(kScoreThreads), 0, static_cast<hipStream_t>(stream),
                       tokens, ld_tokens, row_start, row_from, seq_len, max_len, reinterpret_cast<const WmRec*>(recs), out);
    return launch_status();
}
