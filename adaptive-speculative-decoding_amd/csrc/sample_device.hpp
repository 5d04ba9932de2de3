// sample_device.hpp -- device helpers shared by the sampling kernels (residual_sample.hip: the commit draw;
// draft_sample.hip: the draft tier's proposal): element unpacking, nucleus-masked accumulation, two-float row
// normalisers, the per-vector probability weights, order-preserving float keys and fixed-point masses.
#pragma once

#include "lse_device.hpp"

namespace asd {

template <int DT>
__device__ __forceinline__ void unpack(const u32x4& v, float (&x)[Elem<DT>::kPerVec]);
template <>
__device__ __forceinline__ void unpack<ASD_DTYPE_BF16>(const u32x4& v, float (&x)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        x[2 * i] = __uint_as_float(v[i] << 16);
        x[2 * i + 1] = __uint_as_float(v[i] & 0xFFFF0000u);
    }
}
template <>
__device__ __forceinline__ void unpack<ASD_DTYPE_F16>(const u32x4& v, float (&x)[8]) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t w = v[i];
        const h2 h = __builtin_bit_cast(h2, w);
        x[2 * i] = static_cast<float>(h[0]);
        x[2 * i + 1] = static_cast<float>(h[1]);
    }
}
template <>
__device__ __forceinline__ void unpack<ASD_DTYPE_F32>(const u32x4& v, float (&x)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = __uint_as_float(v[i]);
}

// (m2, s) of the elements >= thr only (the nucleus of a top-p draft row); thr = -inf is the plain accumulate
template <int DT>
__device__ __forceinline__ void accum_nucleus(const u32x4& v, float thr, float c2, float& m2, float& s) {
    using E = Elem<DT>;
    if (thr == -INFINITY) {
        E::accum(v, c2, m2, s);
        return;
    }
    float x[E::kPerVec];
    unpack<DT>(v, x);
#pragma unroll
    for (int i = 0; i < E::kPerVec; ++i) x[i] = x[i] >= thr ? x[i] : -INFINITY;
    if constexpr (E::kPerVec == 8) accum8(x, c2, m2, s);
    else accum4(x, c2, m2, s);
}

// A row's normaliser L = m2 + log2(s) as TWO floats (hi + lo = the f64 value to ~1e-14).  With L rounded to one float every
// probability of the row carries the same relative error (|L| * 6e-8 * ln 2, ~4e-6 at |L| ~ 100), which is harmless for p_t or
// p_d alone but not for their DIFFERENCE on a token that holds nearly all the mass of both rows: max(0, p_t - p_d) then has
// that absolute error against a true value of maybe 1e-3.  The exponent is formed as fma(x, c2, -hi) - lo: the fma result is
// exact to its own (small) magnitude, so the residual keeps ~1e-7 relative accuracy on near-deterministic rows too.
struct Norm2 { float hi, lo; };
__device__ __forceinline__ Norm2 norm2_of(float m2, float s) {
    const double L = static_cast<double>(m2) + log2_split(s);
    Norm2 n;
    n.hi = static_cast<float>(L);
    n.lo = static_cast<float>(L - static_cast<double>(n.hi));
    return n;
}
// weights of one 16-byte vector: w_i = max(0, p_t - p_d), and p_t itself; returns the lane's sums
template <int DT>
__device__ __forceinline__ void vector_weights(const u32x4& vt, const u32x4& vd, bool has_d, float c2, Norm2 Lt, Norm2 Ld,
                                               float tthr, float dthr,
                                               float (&w)[Elem<DT>::kPerVec], float (&pt)[Elem<DT>::kPerVec]) {
    constexpr int N = Elem<DT>::kPerVec;
    float xt[N], xd[N];
    unpack<DT>(vt, xt);
    unpack<DT>(vd, xd);             // (by value, not through an optional pointer: that form went through scratch memory)
#pragma unroll
    for (int i = 0; i < N; ++i) {
        // outside a row's nucleus the probability is exactly 0 (Lt / Ld are then the nucleus normalisers)
        pt[i] = xt[i] >= tthr ? fast_exp2(fmaf(xt[i], c2, -Lt.hi) - Lt.lo) : 0.0f;
        const float pd = (has_d && xd[i] >= dthr) ? fast_exp2(fmaf(xd[i], c2, -Ld.hi) - Ld.lo) : 0.0f;
        w[i] = fmaxf(pt[i] - pd, 0.0f);
    }
}

constexpr int kDsDigits = 4096;                 // histogram slots (12-bit digit)
constexpr float kDsFix = 1099511627776.0f;      // 2^40
constexpr int kDrThreads = 1024;
constexpr int kDrWaves = kDrThreads / 64;
constexpr int kDrMaxTiles = 2048;               // 64-vector tiles per row the LDS mass array holds (V <= 1 M bf16 elements)
constexpr int kDrSeg = 1536;                    // candidate tokens one wave can list in LDS (16 waves x 6 KB)

__device__ __forceinline__ uint32_t order_key(float x) {
    x += 0.0f;                                            // -0 -> +0: equal values share one key
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_floor_value(uint32_t key) {   // smallest float whose key is >= `key`
    const uint32_t u = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
    return __uint_as_float(u);
}
// floor(pr * 2^40) for 0 <= pr <~ 1 without the generic (software) f32 -> u64 conversion: two f32 -> u32 conversions
__device__ __forceinline__ unsigned long long mass_fixed40(float pr) {
    const float y = pr * 1048576.0f;                       // * 2^20
    const uint32_t hi = static_cast<uint32_t>(y);
    const uint32_t lo = static_cast<uint32_t>((y - static_cast<float>(hi)) * 1048576.0f);
    return (static_cast<unsigned long long>(hi) << 20) | lo;
}
// inclusive prefix sum over the 64 lanes (the DPP sequence of wave_sum: row_shr 1,2,4,8, row_bcast 15 / 31)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_move_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false); }
__device__ __forceinline__ int wave_incl_scan_i32(int v) {
    v += dpp_move_i32<0x111, 0xf>(v);
    v += dpp_move_i32<0x112, 0xf>(v);
    v += dpp_move_i32<0x114, 0xf>(v);
    v += dpp_move_i32<0x118, 0xf>(v);
    v += dpp_move_i32<0x142, 0xa>(v);
    v += dpp_move_i32<0x143, 0xc>(v);
    return v;
}
__device__ __forceinline__ unsigned long long wave_incl_scan_u64(unsigned long long v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}


// ---- pieces shared by both kernels -----------------------------------------------------------------------------------
// The CANONICAL pair of one 64-vector tile: (M, s) with  sum over the tile of 2^(x c2) = s 2^M.  Every lane reduces its own
// vector against its own maximum, the wave combines max-first (DPP): the value depends on the tile's bytes only, not on
// which wave of which workgroup computes it.  A ragged last tile is padded with -inf vectors (no mass).
template <int DT>
__device__ __forceinline__ void tile_pair(const u32x4& vec, float c2, float& M, float& sw, float thr = -INFINITY) {
    constexpr int N = Elem<DT>::kPerVec;
    float x[N];
    unpack<DT>(vec, x);
    if (thr != -INFINITY) {                                // a nucleus-truncated row: elements below the threshold carry no mass
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = x[i] >= thr ? x[i] : -INFINITY;
    }
    float vmax = x[0];
#pragma unroll
    for (int i = 1; i < N; ++i) vmax = fmaxf(vmax, x[i]);
    const float ml = fmaxf(vmax * c2, kSentinel);          // a lane of -inf logits: finite sentinel, every term 0
    float sl = 0.0f;
#pragma unroll
    for (int i = 0; i < N; ++i) sl += fast_exp2(fmaf(x[i], c2, -ml));
    M = wave_max(ml);
    sw = wave_sum(sl * fast_exp2(ml - M));
}
// (m2, s) of the row from its tile pairs in a FIXED order (wave w folds tiles w, w + 16, ... one per lane, then the lanes,
// then the 16 waves): the same bits whichever kernel / geometry produced the pairs.  All 1024 threads call it.
__device__ __forceinline__ void fold_tile_pairs(const float* tm, const float* ts, int n_tiles, float (*red)[2], int wave, int lane,
                                                float& m2, float& s) {
    float wm = kSentinel, ws = 0.0f;
    for (int tile = wave + kDrWaves * lane; tile < n_tiles; tile += kDrWaves * 64) ms_merge(wm, ws, tm[tile], ts[tile]);
    wave_merge(wm, ws);
    if (lane == 0) { red[wave][0] = wm; red[wave][1] = ws; }
    __syncthreads();
    m2 = red[0][0];
    s = red[0][1];
#pragma unroll
    for (int w = 1; w < kDrWaves; ++w) ms_merge(m2, s, red[w][0], red[w][1]);
}
__device__ __forceinline__ double wave_incl_scan_f64(double v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

// ---- the nucleus select of ONE row inside ONE 1024-lane workgroup: phases 1-3 of k_draft_row (draft_sample.hip), shared
// with k_verify_nucleus (verify_nucleus.hip) and the bonus-row threshold of asd_residual_sample_top_p (residual_sample.hip).
// One body for all three is what makes x* and L_N -- and so log q(tok) / lp_t -- the same bits in every one of them.
struct NucleusLds {
    unsigned long long hist[kDsDigits];
    float tile_mass[kDrMaxTiles];
    float red[kDrWaves][2];
    unsigned long long wave_tot[kDrWaves];
    unsigned long long sel_above, sel_incl;
    int sel_digit;
    uint32_t cand[kDrWaves][kDrSeg];       // per wave: ids of the tokens above the mass floor, tile by tile
    uint32_t tile_span[kDrMaxTiles];       // (first candidate << 16) | candidates of the tile, in its wave's list
    int overflow;
};

// fn(v, vector) for thread t's vectors v = t, t + 1024, ... (after the first sweep the row is L2-resident).  The trip count is
// the same for all lanes of a wave -- a ragged last tile is padded with -inf vectors, which carry no mass anywhere -- so the wave
// reductions inside `fn` always run with every lane active.  Four of a thread's vectors are loaded before the first is consumed:
// with one load in flight per thread a sweep is 19 dependent L2 round trips.  (Holding the row in registers instead, 19 x 16 B
// per lane, was tried: it spills at the 128-VGPR budget of a 1024-lane workgroup and was slower.)
template <int DT, class Fn>
__device__ __forceinline__ void row_sweep(const u32x4* row, int nvec, int t, Fn&& fn) {
    using E = Elem<DT>;
    constexpr int kAhead = 4;
    const int lane = t & 63;
    const u32x4 neg = {E::kNegInfWord, E::kNegInfWord, E::kNegInfWord, E::kNegInfWord};
    for (int v0 = t - lane; v0 < nvec; v0 += kAhead * kDrThreads) {
        u32x4 q[kAhead];
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            const int v = v0 + j * kDrThreads + lane;
            q[j] = v < nvec ? row[v] : neg;
        }
#pragma unroll
        for (int j = 0; j < kAhead; ++j)
            if (v0 + j * kDrThreads < nvec) fn(v0 + j * kDrThreads + lane, q[j]);     // wave-uniform guard
    }
}
// fn(slot, x) for this wave's candidates cand[slot], slot in [0, count): 64 per step, four steps' logits gathered (L2 hits)
// before the first is used; lanes past the end see slot = -1, x = -inf
template <int DT, class Fn>
__device__ __forceinline__ void cand_sweep(const u32x4* row, const uint32_t* cand, int count, int lane, Fn&& fn) {
    using E = Elem<DT>;
    constexpr int kAhead = 4;
    for (int e0 = 0; e0 < count; e0 += kAhead * 64) {
        float x[kAhead];
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            const int e = e0 + j * 64 + lane;
            x[j] = E::scalar(row, e < count ? cand[e] : 0u);
        }
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            const int e = e0 + j * 64 + lane;
            if (e0 + j * 64 < count) fn(e < count ? e : -1, e < count ? x[j] : -INFINITY);
        }
    }
}

// ---- top-k: x_k, the k-th largest logit of the row counting multiplicity (HF TopKLogitsWarper keeps { v : x_v >= x_k }, every
// tie at x_k included), or -inf when fewer than k values are > -inf.  A radix select by COUNT on order_key(x) with the digit
// schedule of the mass select (12 + 12 bits for 16-bit logits, 12 + 12 + 8 for f32): per level every token of the selected
// prefix adds 1 to the slot of its digit, the slots are scanned from the top for the digit where above < k <= above + count.
// Integer counts: the result depends on the row's bytes only, not on the geometry.  The counts live in the first 16 KB of
// sh.hist (the mass select rewrites it afterwards); sel_digit / sel_above / wave_tot are the mass select's words.  The first
// level's sweep is the only HBM read of the row; the later levels compare every token against the prefix (L2 hits) and count
// only the tokens of the selected digit.  All 1024 threads call it.
template <int DT>
__device__ __forceinline__ float topk_row_threshold(const u32x4* row, int nvec, int top_k, NucleusLds& sh, int t) {
    using E = Elem<DT>;
    constexpr int N = E::kPerVec;
    constexpr int kLevels = DT == ASD_DTYPE_F32 ? 3 : 2;
    const int lane = t & 63, wave = t >> 6;
    uint32_t* const cnt = reinterpret_cast<uint32_t*>(sh.hist);
    const uint32_t k = static_cast<uint32_t>(top_k);
    const int shifts[3] = {20, 8, 0}, widths[3] = {12, 12, 8};
    uint32_t prefix = 0u, above = 0u;
    bool found = true;
    for (int lv = 0; lv < kLevels; ++lv) {
        const int shift = shifts[lv], digits = 1 << widths[lv], hi_shift = shifts[lv] + widths[lv];
        for (int i = t; i < digits; i += kDrThreads) cnt[i] = 0u;
        if (t == 0) sh.sel_digit = -1;
        __syncthreads();
        row_sweep<DT>(row, nvec, t, [&](int, const u32x4& vec) {
            float x[N];
            unpack<DT>(vec, x);
#pragma unroll
            for (int i = 0; i < N; ++i) {
                if (!(x[i] > -INFINITY)) continue;             // -inf (and the padding of a ragged tile) is never counted
                const uint32_t key = order_key(x[i]);
                if (hi_shift >= 32 || (key >> hi_shift) == (prefix >> hi_shift)) atomicAdd(&cnt[(key >> shift) & (digits - 1)], 1u);
            }
        });
        __syncthreads();
        // thread t owns the t-th chunk of digits counted from the TOP
        const int per = digits >= kDrThreads ? digits / kDrThreads : 1;
        const int hi = digits - t * per, lo = hi - per;
        int mine = 0;
        if (lo >= 0)
            for (int j = lo; j < hi; ++j) mine += static_cast<int>(cnt[j]);
        const int incl = wave_incl_scan_i32(mine);
        if (lane == 63) sh.wave_tot[wave] = static_cast<unsigned long long>(incl);
        __syncthreads();
        uint32_t base = 0u;
#pragma unroll
        for (int w = 0; w < kDrWaves; ++w)
            if (w < wave) base += static_cast<uint32_t>(sh.wave_tot[w]);
        const uint32_t before = above + base + static_cast<uint32_t>(incl - mine);
        if (lo >= 0 && mine > 0 && before < k && k <= before + static_cast<uint32_t>(mine)) {   // exactly one thread
            uint32_t acc = before;
            int pick = lo;
            for (int j = hi - 1; j >= lo; --j) {
                const uint32_t m = cnt[j];
                if (m > 0u && acc + m >= k) { pick = j; break; }
                acc += m;
            }
            sh.sel_digit = pick;
            sh.sel_above = acc;
        }
        __syncthreads();
        const int dg = sh.sel_digit;
        if (dg >= 0) {
            prefix |= static_cast<uint32_t>(dg) << shift;
            above = static_cast<uint32_t>(sh.sel_above);
        }
        __syncthreads();                                  // sel_* and the counts are rewritten by the next level
        if (dg < 0) { found = false; break; }             // (block-uniform) fewer than k counted values
    }
    if (!found) return -INFINITY;
    // 16-bit logits: the low 8 key bits are constant (zeros for x >= 0, ones for x < 0), as in the mass select
    if (kLevels == 2 && !(prefix & 0x80000000u)) prefix |= 0xffu;
    return key_floor_value(prefix);
}

struct NucleusSel {
    float thr;        // x*: the nucleus is { v : x_v >= thr } (-inf: no truncation, an empty select or a row without mass)
    double L64;       // log2 of the normaliser of the distribution drawn from / scored against (L_N with truncation)
    bool listed;      // the candidates of the row are in sh.cand: later phases walk the lists, not the row
    int wcnt;         // candidates in this wave's list (wave-uniform)
    bool pairs;       // kMinP, x_mp won: sh.tile_span / sh.tile_mass hold the tile pairs of { x >= thr } (as with levels == 0)
};

//   1. (m2, s) of the row                                   -> L, the softmax normaliser            (sweep, exp per element)
//   2. top-p only (levels > 0): tokens below the mass floor (1 - top_p) / V cannot be inside the nucleus; a compare-only sweep
//      lists the rest (the CANDIDATES) in LDS, per wave, tile by tile, in a fixed order             (sweep, compares)
//   3. radix select on probability MASS over the candidates (2^-40 fixed point, integer adds: reproducible) -> x*, L_N
// (draft_sample.hip explains each phase.)  Leaves the tile pairs' sums in sh.tile_mass / their maxima in sh.tile_span when
// levels == 0, the candidate spans in sh.tile_span otherwise.  All 1024 threads call it; `stamp(slot)` marks phase boundaries.
// kTopK (HF's TopKLogitsWarper before its TopPLogitsWarper): phase 0 finds x_k (topk_row_threshold) and every later phase works
// on the top-k set K = { x >= x_k } only -- the tile pairs are taken with thr = x_k (-> L_K), the candidate floor is
// max(x_floor, x_k) and the mass target is top_p of K's mass -- so thr = max(x_k, x*_K) and L64 = the normaliser over
// { x >= thr }; with levels == 0 (top-p off) thr = x_k, L64 = L_K.  kTopK = false is the form without phase 0 (x_lo is the
// constant -inf, every use of it folds away).
// kMinP (HF's MinPLogitsWarper behind the two, include/asd_hip.h "Min-p"): sweep 1 also takes the EXACT maximum x_max of the raw
// logits (a float max per lane, the lanes, the 16 waves: no rounding, no dependence on the order), and behind the select
// x_mp = x_max + mp_delta (mp_delta = T ln(min_p) <= 0, the launcher's) is compared with thr_kp = max(x_k, x*_K).  Where x_mp
// is larger it is the threshold, and one more sweep (L2 hits) takes the tile pairs of { x >= x_mp } and folds them into its
// normaliser -- the pairs stay in sh.tile_span / sh.tile_mass as with levels == 0 (`pairs`), the candidate lists are dropped.
// With levels == 0 and no top-k there is no select at all: the row costs sweep 1, that sweep and the draw.  kMinP = false
// compiles none of it.
template <int DT, bool kTopK = false, bool kMinP = false, class Stamp>
__device__ __forceinline__ NucleusSel nucleus_row_select(const u32x4* row, int V, int nvec, int n_tiles, float c2, float top_p,
                                                         int levels, NucleusLds& sh, int t, Stamp&& stamp, int top_k = 0,
                                                         float mp_delta = 0.0f) {
    using E = Elem<DT>;
    constexpr int N = E::kPerVec;
    const int lane = t & 63, wave = t >> 6;
    auto any_at_least = [&](const float (&x)[N], float bound) -> bool {
        bool any = false;
#pragma unroll
        for (int i = 0; i < N; ++i) any = any || (x[i] >= bound);
        return __ballot(any) != 0ull;
    };
    float m2, s;
    float x_lo = -INFINITY;                                   // x_k of a top-k row (kTopK only)
    if constexpr (kTopK) x_lo = topk_row_threshold<DT>(row, nvec, top_k, sh, t);
    stamp(0);
    // Sweep 1 (the only pass that reads HBM) leaves every tile's CANONICAL (max, sum) pair in LDS and folds the pairs in the
    // fixed order of fold_tile_pairs: L has the same bits as in k_draft_group, whatever the batch (round 2 ran a per-lane
    // online softmax here when top-p was on: 5 us less for the sweep, but a value only this geometry could reproduce).
    // Without truncation the tile masses then follow from L without a second exp-per-element sweep of the row.
    float x_max = -INFINITY;                                  // kMinP only: this lane's, then the row's, largest raw logit
    row_sweep<DT>(row, nvec, t, [&](int v, const u32x4& vec) {
        float M, sw;
        if constexpr (kTopK) tile_pair<DT>(vec, c2, M, sw, x_lo);      // the top-k set's pairs -> L_K
        else tile_pair<DT>(vec, c2, M, sw);
        if (lane == 0) {                                      // nothing is carried from tile to tile: the four tiles of a
            sh.tile_span[v >> 6] = __float_as_uint(M);        // row_sweep step reduce side by side
            sh.tile_mass[v >> 6] = sw;
        }
        if constexpr (kMinP) {
            float x[N];
            unpack<DT>(vec, x);
#pragma unroll
            for (int i = 0; i < N; ++i) x_max = fmaxf(x_max, x[i]);
        }
    });
    __syncthreads();
    fold_tile_pairs(reinterpret_cast<const float*>(sh.tile_span), sh.tile_mass, n_tiles, sh.red, wave, lane, m2, s);
    if constexpr (kMinP) {
        // the 16 waves' maxima through sh.wave_tot (idle here: phase 0 is over, the mass select writes it behind two barriers)
        x_max = wave_max(x_max);
        if (lane == 0) sh.wave_tot[wave] = __float_as_uint(x_max);
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kDrWaves; ++w) x_max = fmaxf(x_max, __uint_as_float(static_cast<uint32_t>(sh.wave_tot[w])));
    }
    stamp(1);
    NucleusSel r;
    r.pairs = false;
    r.L64 = static_cast<double>(m2) + log2_split(s);
    r.thr = -INFINITY;
    r.listed = false;
    r.wcnt = 0;
    int& wcnt = r.wcnt;
    if (levels > 0 && s > 0.0f) {
        const float L = static_cast<float>(r.L64);
        const float p_floor = fmaxf((1.0f - top_p) / static_cast<float>(V), 1.0f / kDsFix);
        float x_floor = (L + __builtin_amdgcn_logf(p_floor)) / c2;            // p >= p_floor  <=>  x >= x_floor
        if constexpr (kTopK) x_floor = fmaxf(x_floor, x_lo);                    // only K's tokens are candidates
        // ---- candidates.  Tokens below p_floor = (1 - top_p) / V carry < 1 - top_p together, so the threshold lies above
        // all of them.  One compare-only sweep lists the others (per-lane counts, DPP prefix sum, lane-major inside a tile: a
        // fixed order) in the LDS segment of the wave that owns their tile; the histogram levels, the nucleus normaliser and
        // the tile masses then cost a few candidates per lane instead of a sweep of divergent per-element work.  A row too
        // flat for the lists (some wave holds more than kDrSeg candidates) keeps the sweeps.
        if (t == 0) sh.overflow = 0;
        __syncthreads();
        bool over = false;
        row_sweep<DT>(row, nvec, t, [&](int v, const u32x4& vec) {
            float x[N];
            unpack<DT>(vec, x);
            uint32_t keep = 0u;                           // bit i: element i of this lane's vector is a candidate
#pragma unroll
            for (int i = 0; i < N; ++i) keep |= (x[i] >= x_floor ? 1u : 0u) << i;
            const int first = wcnt;
            if (__ballot(keep != 0u) != 0ull) {
                const int cnt = __builtin_popcount(keep);
                const int incl = wave_incl_scan_i32(cnt);
                const int n = __builtin_amdgcn_readlane(incl, 63);
                if (wcnt + n <= kDrSeg) {
                    int at = wcnt + incl - cnt;           // lane-major inside the tile: a fixed order
                    while (keep != 0u) {                  // as many rounds as the fullest lane has candidates (1-3, not N)
                        sh.cand[wave][at++] = static_cast<uint32_t>(v * N + __builtin_ctz(keep));
                        keep &= keep - 1u;
                    }
                    wcnt += n;
                } else {
                    over = true;
                }
            }
            if (lane == 0) sh.tile_span[v >> 6] = (static_cast<uint32_t>(first) << 16) | static_cast<uint32_t>(wcnt - first);
        });
        if (over && lane == 0) sh.overflow = 1;
        __syncthreads();
        r.listed = sh.overflow == 0;
        stamp(12);

        unsigned long long above = 0ull, target = 0ull;
        uint32_t prefix = 0u;
        bool empty = false;
        const int shifts[3] = {20, 8, 0}, widths[3] = {12, 12, 8};
        for (int lv = 0; lv < levels; ++lv) {
            const int shift = shifts[lv], digits = 1 << widths[lv], hi_shift = shifts[lv] + widths[lv];
            for (int i = t; i < digits; i += kDrThreads) sh.hist[i] = 0ull;
            if (t == 0) sh.sel_digit = -1;
            __syncthreads();
            stamp(2 + 2 * lv);
            // every candidate adds its probability, 2^-40 fixed point, to the slot of its digit
            auto add_mass = [&](int, float x) {
                if (!(x >= x_floor)) return;
                const uint32_t key = order_key(x);
                const bool mine = hi_shift >= 32 || (key >> hi_shift) == (prefix >> hi_shift);
                if (mine) atomicAdd(&sh.hist[(key >> shift) & (digits - 1)], mass_fixed40(fast_exp2(fmaf(x, c2, -L))));
            };
            if (r.listed) {
                cand_sweep<DT>(row, sh.cand[wave], wcnt, lane, add_mass);
            } else {
                row_sweep<DT>(row, nvec, t, [&](int, const u32x4& vec) {
                    float x[N];
                    unpack<DT>(vec, x);
                    if (!any_at_least(x, x_floor)) return;
#pragma unroll
                    for (int i = 0; i < N; ++i) add_mass(0, x[i]);
                });
            }
            __syncthreads();
            stamp(3 + 2 * lv);
            // thread t owns the t-th chunk of digits counted from the TOP
            const int per = digits >= kDrThreads ? digits / kDrThreads : 1;
            const int hi = digits - t * per, lo = hi - per;
            unsigned long long mine = 0ull;
            if (lo >= 0)
                for (int j = lo; j < hi; ++j) mine += sh.hist[j];
            const unsigned long long incl = wave_incl_scan_u64(mine, lane);
            if (lane == 63) sh.wave_tot[wave] = incl;
            __syncthreads();
            unsigned long long base = 0ull, total = 0ull;
#pragma unroll
            for (int w = 0; w < kDrWaves; ++w) {
                if (w < wave) base += sh.wave_tot[w];
                total += sh.wave_tot[w];
            }
            if (lv == 0) {   // the probabilities sum to 1 = 2^40 fixed point (the histogram only holds the tokens above p_floor)
                target = static_cast<unsigned long long>(static_cast<double>(top_p) * static_cast<double>(kDsFix));
                if (target > total) target = total;      // fixed-point truncation: never ask for more than is there
                if (target == 0ull) target = 1ull;
                empty = total == 0ull;
            }
            const unsigned long long before = above + base + incl - mine;
            if (lo >= 0 && mine > 0ull && before < target && target <= before + mine) {   // exactly one thread
                unsigned long long acc = before;
                int pick = lo;
                for (int j = hi - 1; j >= lo; --j) {
                    const unsigned long long m = sh.hist[j];
                    if (m > 0ull && acc + m >= target) { pick = j; break; }
                    acc += m;
                }
                sh.sel_digit = pick;
                sh.sel_above = acc;
                sh.sel_incl = acc + sh.hist[pick];
            }
            __syncthreads();
            const int dg = sh.sel_digit;
            if (dg < 0) empty = true;
            else {
                prefix |= static_cast<uint32_t>(dg) << shift;
                above = sh.sel_above;
            }
            __syncthreads();                              // sel_* and hist are rewritten by the next level
        }
        // 16-bit logits: the low 8 key bits were never examined because they are constant -- zeros for x >= 0, ones for
        // x < 0 (the key of a negative float is its complement) -- so the threshold is the logit value itself
        if (levels == 2 && !(prefix & 0x80000000u)) prefix |= 0xffu;
        r.thr = empty ? -INFINITY : key_floor_value(prefix);
        // The nucleus normaliser needs no pass of its own: the last level's scan has summed the masses of exactly the tokens
        // >= thr (2^-40 fixed point relative to L, an integer sum: reproducible, |error| < candidates * 2^-40).
        if (!empty) r.L64 = static_cast<double>(L) + log2_split(static_cast<float>(sh.sel_incl)) - 40.0;
        stamp(8);
    }
    if constexpr (kTopK) r.thr = fmaxf(r.thr, x_lo);          // x*_K >= x_k whenever the mass select found one
    if constexpr (kMinP) {
        const float x_mp = x_max + mp_delta;                  // p_v >= min_p p_max  <=>  x_v >= x_max + T ln(min_p)
        if (x_mp > r.thr) {                                   // (block-uniform; never for a row of -inf)
            __syncthreads();                                  // the select's readers of tile_span / tile_mass are done
            row_sweep<DT>(row, nvec, t, [&](int v, const u32x4& vec) {
                float M, sw;
                tile_pair<DT>(vec, c2, M, sw, x_mp);
                if (lane == 0) {
                    sh.tile_span[v >> 6] = __float_as_uint(M);
                    sh.tile_mass[v >> 6] = sw;
                }
            });
            __syncthreads();
            fold_tile_pairs(reinterpret_cast<const float*>(sh.tile_span), sh.tile_mass, n_tiles, sh.red, wave, lane, m2, s);
            r.L64 = static_cast<double>(m2) + log2_split(s);
            r.thr = x_mp;
            r.listed = false;
            r.pairs = true;
        }
    }
    return r;
}

// rows[b] of the packed sampling table (common.hpp, SamplingRow) as workgroup-uniform values: b is uniform, and every field goes
// through readfirstlane so that the mode branches and the select's parameters live in scalar registers as a kernel argument would
__device__ __forceinline__ SamplingRow load_sampling_row(const SamplingRow* rows, int b) {
    const SamplingRow q = rows[b];
    SamplingRow r{};
    r.c2 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(q.c2)));
    r.top_p = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(q.top_p)));
    r.levels = __builtin_amdgcn_readfirstlane(q.levels);
    r.top_k = __builtin_amdgcn_readfirstlane(q.top_k);
    r.mp_delta = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(q.mp_delta)));
    r.clamp = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(q.clamp)));
    return r;
}

// ---- cross-workgroup mailboxes of the group kernels (k_draft_group, k_residual_group): single writer, single reader,
// self-tagging words (non-zero = published), handed back empty by the reader
constexpr int kDgMaxGroups = 32;          // workgroups per row
constexpr int kDgMaxLevels = 3;           // histogram rounds (f32 keys: 12 + 12 + 8 bits)
constexpr int kDgMsgs = 1 + kDgMaxLevels; // mailbox messages per partner: (m2, s), then one decision per round
constexpr int kDgSlots = 256;             // rows * groups the histogram exchange area is sized for (one workgroup per CU)
constexpr int kDgSpinLimit = 1 << 19;    // polls (~1 us each) of a word whose store is in flight before the row is given up
constexpr unsigned long long kDgValid = 1ull << 63;

// bounded wait for a mailbox word (non-zero = published).  `lost` (LDS) is raised by the first wait that runs out and makes
// every later wait of the workgroup return at once: a row whose partner never shows up costs ONE timeout, not one per word.
// `status`: the workspace's sticky status word (its first 32 bits; include/asd_hip.h, asd_workspace_status) -- the wait that runs
// out or-s ASD_WS_LOST_HANDOFF into it, so that the host learns of the loss at its next synchronisation: the poisoned outputs
// (tok = -1, lp = NaN) say WHICH row, the status word says THAT the workspace is no longer all-zero (the late word will never be
// handed back empty) and must be re-initialised before its next use.
__device__ __forceinline__ unsigned long long dg_poll(unsigned long long* slot, volatile int* lost, uint32_t* status) {
    unsigned long long v = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int spins = 0; v == 0ull && spins < kDgSpinLimit && !*lost; ++spins) {
        __builtin_amdgcn_s_sleep(1);
        v = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (v == 0ull) {
        if (!*lost && status) __hip_atomic_fetch_or(status, static_cast<uint32_t>(ASD_WS_LOST_HANDOFF), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *lost = 1;
    }
    return v;
}
constexpr size_t kWorkspaceHeaderBytes = 256;   // every hand-off workspace begins with this block: u32 status word at +0, rest reserved
__device__ __forceinline__ void dg_put(unsigned long long* slot, unsigned long long v) {
    __hip_atomic_store(slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}


}  // namespace asd
