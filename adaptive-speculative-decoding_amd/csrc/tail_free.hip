// tail_free.hip -- tail-free sampling (`tfs` of text-generation-webui, koboldcpp, KoboldAI and Aphrodite; `tfs_z` of older
// llama.cpp), gfx950: the one truncation that needs a row IN SORTED ORDER.  One in-place pass on the logits behind the relative
// cut and ahead of the entropy cuts; the row sort and the scan over the sorted row are this file's.
//
// logits[b][j][v] lies at b*ld_seq + j*ld_row + v (asd_relative_cut_rows' addressing; bf16 / f16 / f32; the first element of a
// row aligned to the element size only).  All K1 rows of sequence b use the record table[b] = {inv_t, z}; fin is the set of
// finite elements, n = |fin|; a -inf element carries no mass, stays -inf and enters no statistic.  With the finite elements
// sorted by value, descending, and w_(i) = exp(inv_t * (x_(i) - x_max)) in f64:
//   d1_i = w_(i) - w_(i+1) (i < n-1),  d2_i = |d1_i - d1_(i+1)| (i < n-2),  S = sum d2_i,  c_i = d2_0 + ... + d2_i;
//   i* = the first i with c_i > z * S (the product in f64 from the f32 z);  x_cut = the stored value at sorted position i*;
//   v is cut iff x_v < x_cut: every tie at x_cut stays, the arg-max is never cut.
// z == 1: off, the row is not read.  z outside (0, 1] or an inv_t that is not a positive finite number: damaged device data, the
// row is skipped.  n < 3, S == 0, a NaN or +inf element: the row is left as it is.  A cut element becomes -inf of the dtype;
// nothing else is written (a vector is stored only where a bit of it changes).
//
// GEOMETRY.  One workgroup of 1024 lanes (16 waves) per (b, j), four phases; the row is never held in registers, phases 2 and 4
// re-read it from L2.
//   1  STATISTICS and the first histogram, one sweep of the row in relative_cut.hip's walk (lane t owns the 16-byte vectors t,
//      t + 1024, ... of the aligned body through a buffer resource, wave 0 the up to 7 scalar elements in front of and behind
//      it): all on the stored BITS -- n, whether a NaN or +inf element exists, and the per-wave counts of the keys' lowest
//      digit.  The key of a finite element is its bits under  k = sign ? bits : bits ^ 0x7FFF(FFFF): ascending keys are
//      descending values, 16 bits for bf16 / f16 and 32 for f32.
//   2  KEYS-ONLY LSD RADIX SORT, 8-bit digits: two passes for the 16-bit dtypes, four for f32, between the row's two key
//      buffers in the workspace (row -> A -> B [-> A -> B]: the sorted keys always end in B).  Per pass: per-wave 256-bin
//      histograms in LDS (ds_add), ONE exclusive scan over the 4096 (digit, wave) counts (four per lane, a wave scan, the wave
//      totals through LDS), and a stable scatter: a wave takes 64 keys at a time, the lanes that hold the same digit find each
//      other by eight ballots over the digit's bits, the lowest of them takes the group's base with one returning ds_add and
//      hands it on by a read-lane, a lane's place is base + its rank among the group's lower lanes.  The first pass takes its
//      keys from the row in phase 1's walk (its order is fixed, and a first LSD pass needs no stability); in the later passes
//      wave w owns the contiguous slice [w * ceil(n / 16), ...) of the source buffer and walks it in order, lanes in lane order:
//      that is what stability across passes rests on.  No payload ids: the rule needs values only.
//   3  SCAN over the sorted keys.  Lane t owns the d2_i of i in [t * C, (t + 1) * C), C = ceil(n / 1024), reads its keys and two
//      more, turns them back into values, takes w by the f64 exp (one per key) and adds its d2 in ascending i in f64.  The
//      1024 chunk sums: an inclusive scan inside each wave (lane l adds the partial of lane l - 1, l - 2, l - 4, ... l - 32, in
//      that order), the sixteen wave totals in wave order through LDS, which gives S and every lane's exclusive prefix P_t =
//      (waves before) + (lanes before).  The first lane with P_t + s_t > z * S walks its chunk again -- the same additions, so
//      its last partial is s_t bit for bit -- and the first i with P_t + (d2 of the chunk up to i) > z * S is i*.
//   4  CUT sweep: relative_cut.hip's stores, x_v < x_cut on the stored values.
// ORDER of the f64 additions: lane chunk (ascending i), wave (the scan above), workgroup (wave order): a row's result depends
// on its bytes and its record only, not on what the workspace held.
// WORKSPACE: per row two key buffers of V keys, each rounded up to 256 bytes; asd_tail_free_workspace_bytes.

#include <hip/hip_runtime.h>

#include "top_logprobs_device.hpp"
#include "sample_device.hpp"

namespace asd {
namespace {

constexpr int kTfThreads = 1024;
constexpr int kTfWaves = kTfThreads / 64;
constexpr int kTfBins = 256;                     // 8-bit digits
constexpr int kTfUnroll = 4;                     // the cut sweep: 16-byte loads per lane in flight
constexpr uint32_t kTfStride = kTfThreads * 16u; // bytes between two vectors of one lane

struct TfRec {
    float inv_t, z;
};
static_assert(sizeof(TfRec) == ASD_TAIL_FREE_REC_BYTES, "TfRec");

struct TfLds {
    uint32_t hist[kTfBins * kTfWaves];           // [digit][wave]: counts, then the scatter's running bases
    uint32_t wtot[kTfWaves];                     // the scan's wave totals
    int cnt[kTfWaves], bad[kTfWaves];
    double dsum[kTfWaves];
    int first[kTfWaves];
    uint32_t cut_key;
};

template <int DT>
struct TfKey {                                   // bf16 / f16
    using type = uint16_t;
    static constexpr uint32_t kMag = 0x7FFFu, kSign = 0x8000u;
    static constexpr uint32_t kExp = DT == ASD_DTYPE_BF16 ? 0x7F80u : 0x7C00u;
    static constexpr int kPasses = 2;
    static __device__ __forceinline__ float value(uint32_t bits) {
        if constexpr (DT == ASD_DTYPE_BF16) return __uint_as_float(bits << 16);
        else return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(bits)));
    }
};
template <>
struct TfKey<ASD_DTYPE_F32> {
    using type = uint32_t;
    static constexpr uint32_t kMag = 0x7FFFFFFFu, kSign = 0x80000000u, kExp = 0x7F800000u;
    static constexpr int kPasses = 4;
    static __device__ __forceinline__ float value(uint32_t bits) { return __uint_as_float(bits); }
};

// stored bits <-> key: an involution (the sign bit is kept); ascending keys are descending values
template <int DT>
__device__ __forceinline__ uint32_t tf_flip(uint32_t u) {
    return (u & TfKey<DT>::kSign) ? u : (u ^ TfKey<DT>::kMag);
}

// a row as the sweeps walk it: `head` scalar elements up to the first 16-byte boundary, nvec vectors, `tail` scalar elements
struct TfRow {
    char* rowp;
    char* body;
    int head, nvec, tail;
};

template <int DT>
__device__ __forceinline__ uint32_t tf_bits_at(const char* rowp, int id) {
    if constexpr (DT == ASD_DTYPE_F32) return reinterpret_cast<const uint32_t*>(rowp)[id];
    else return reinterpret_cast<const uint16_t*>(rowp)[id];
}

// Phase 1's walk, which the first scatter repeats: every WAVE calls el(bits, valid) the same number of times (el holds
// ballots), a lane's elements in ascending order.  valid: the slot holds an element of the row.
template <int DT, class F>
__device__ __forceinline__ void tf_walk(const TfRow& r, int tid, F&& el) {
    constexpr int N = Elem<DT>::kPerVec;
    const int wave = tid >> 6;
    if (wave == 0 && r.head > 0) {                                                   // (wave-uniform)
        const bool in = tid < r.head;
        el(in ? tf_bits_at<DT>(r.rowp, tid) : 0u, in);
    }
    const uint32_t end = static_cast<uint32_t>(r.nvec) * 16u;                        // launcher: V * element size < 2^31
    // (a lane whose offset is >= end gets zeros and makes no memory access)
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(r.body, 0, static_cast<int>(end), 0x00020000);
    const uint32_t wave_off = static_cast<uint32_t>(wave) * 64u * 16u;
    for (uint32_t base = 0u; base + wave_off < end; base += kTfStride) {             // (the bound is the wave's lane 0's)
        const uint32_t off = base + static_cast<uint32_t>(tid) * 16u;
        const u32x4 v = load16<false>(rsrc, off);
        const bool in = off < end;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if constexpr (N == 8) el((i & 1) ? v[i >> 1] >> 16 : v[i >> 1] & 0xFFFFu, in);
            else el(v[i], in);
        }
    }
    if (wave == 0 && r.tail > 0) {
        const bool in = tid < r.tail;
        el(in ? tf_bits_at<DT>(r.rowp, r.head + r.nvec * N + tid) : 0u, in);
    }
}

// inclusive prefix sums over the 64 lanes, lane l adding the partials of l - 1, l - 2, l - 4, ..., l - 32 in that order
__device__ __forceinline__ uint32_t tf_wave_scan_u32(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}
__device__ __forceinline__ double tf_wave_scan_f64(double v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// counts[digit][wave] -> their exclusive prefix sums in (digit, wave) order, in place.  Lane t owns the four entries 4t .. 4t+3.
__device__ __forceinline__ void tf_scan_hist(TfLds& sh, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    __syncthreads();                                                                 // every count is in
    uint32_t c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = sh.hist[tid * 4 + i];
    const uint32_t mine = (c[0] + c[1]) + (c[2] + c[3]);
    const uint32_t incl = tf_wave_scan_u32(mine, lane);
    if (lane == 63) sh.wtot[wave] = incl;
    __syncthreads();
    uint32_t before = 0u;
#pragma unroll 1
    for (int w = 0; w < wave; ++w) before += sh.wtot[w];
    uint32_t run = before + incl - mine;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        sh.hist[tid * 4 + i] = run;
        run += c[i];
    }
    __syncthreads();                                                                 // the bases are in (and wtot may be reused)
}

// One round of the stable scatter: the wave's lanes with `valid` each hold one key; equal digits go to consecutive places in
// lane order, behind every key the wave scattered to that digit before.  Called by whole waves.
template <class K>
__device__ __forceinline__ void tf_scatter_round(TfLds& sh, K* dst, uint32_t key, int shift, bool valid, int lane, int wave) {
    const uint32_t digit = (key >> shift) & 0xFFu;
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
        const uint64_t set = __ballot((digit >> bit) & 1u);
        peers &= ((digit >> bit) & 1u) ? set : ~set;
    }
    if (!valid) peers = 0ull;
    const uint64_t below = peers & ((1ull << lane) - 1ull);
    const int leader = peers ? __builtin_ctzll(peers) : lane;
    uint32_t base = 0u;
    if (valid && below == 0ull) base = atomicAdd(&sh.hist[digit * kTfWaves + wave], static_cast<uint32_t>(__popcll(peers)));
    base = __shfl(base, leader);
    if (valid) dst[base + static_cast<uint32_t>(__popcll(below))] = static_cast<K>(key);
}

template <int DT>
__device__ __forceinline__ void tf_store_one(char* rowp, int id) {
    using E = Elem<DT>;
    if constexpr (DT == ASD_DTYPE_F32) reinterpret_cast<uint32_t*>(rowp)[id] = E::kNegInfWord;
    else reinterpret_cast<uint16_t*>(rowp)[id] = static_cast<uint16_t>(E::kNegInfWord & 0xFFFFu);
}

// bit i of mask: element i of `vec` becomes -inf; stored (16 bytes, to `dst`) only where a bit of the vector changes
template <int DT>
__device__ __forceinline__ void tf_store_vec(char* dst, const u32x4& vec, uint32_t mask) {
    using E = Elem<DT>;
    if (mask == 0u) return;
    u32x4 w = vec;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (E::kPerVec == 8) {
            if ((mask >> (2 * i)) & 1u) w[i] = (w[i] & 0xFFFF0000u) | (E::kNegInfWord & 0x0000FFFFu);
            if ((mask >> (2 * i + 1)) & 1u) w[i] = (w[i] & 0x0000FFFFu) | (E::kNegInfWord & 0xFFFF0000u);
        } else {
            if ((mask >> i) & 1u) w[i] = E::kNegInfWord;
        }
    }
    const bool same = w[0] == vec[0] && w[1] == vec[1] && w[2] == vec[2] && w[3] == vec[3];
    if (!same) *reinterpret_cast<u32x4*>(dst) = w;
}

template <int DT>
__global__ __launch_bounds__(kTfThreads) void k_tail_free_rows(void* logits, int64_t ld_seq, int64_t ld_row, int K1, int V,
                                                               const TfRec* __restrict__ table, char* workspace,
                                                               uint64_t buf_bytes) {
    using E = Elem<DT>;
    using KT = TfKey<DT>;
    using K = typename KT::type;
    constexpr int N = E::kPerVec;
    __shared__ TfLds sh;

    const int tid = static_cast<int>(threadIdx.x);
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int row = static_cast<int>(blockIdx.x);
    const int b = static_cast<int>(static_cast<uint32_t>(row) / static_cast<uint32_t>(K1));
    const int j = row - b * K1;
    const float z = table[b].z;                                                      // (uniform: scalar loads)
    const float inv_t = table[b].inv_t;
    if (!(z > 0.0f && z < 1.0f)) return;                                             // 1: off; anything else: damaged, skipped
    if (!(inv_t > 0.0f && inv_t < 3.0e38f)) return;

    TfRow r;
    r.rowp = static_cast<char*>(logits) + (static_cast<int64_t>(b) * ld_seq + static_cast<int64_t>(j) * ld_row) * E::kBytes;
    const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(r.rowp) & 15u);     // (a multiple of the element size)
    r.head = mis ? static_cast<int>((16u - mis) / E::kBytes) : 0;
    if (r.head > V) r.head = V;
    r.nvec = (V - r.head) / N;
    r.tail = V - r.head - r.nvec * N;
    r.body = r.rowp + static_cast<int64_t>(r.head) * E::kBytes;
    K* buf_a = reinterpret_cast<K*>(workspace + static_cast<uint64_t>(row) * 2u * buf_bytes);
    K* buf_b = reinterpret_cast<K*>(workspace + (static_cast<uint64_t>(row) * 2u + 1u) * buf_bytes);

    // ---- phase 1: n, the NaN / +inf flag and the histogram of the keys' lowest digit, on the stored bits
#pragma unroll
    for (int i = 0; i < 4; ++i) sh.hist[tid * 4 + i] = 0u;
    __syncthreads();
    int cnt = 0, bad = 0;
    tf_walk<DT>(r, tid, [&](uint32_t u, bool in) {
        const bool fin = in && (u & KT::kExp) != KT::kExp;
        bad |= (in && !fin && u != (E::kNegInfWord & (KT::kMag | KT::kSign))) ? 1 : 0;        // not finite and not -inf
        cnt += fin ? 1 : 0;
        if (fin) atomicAdd(&sh.hist[(tf_flip<DT>(u) & 0xFFu) * kTfWaves + wave], 1u);
    });
    cnt = wave_sum_i32(cnt);
    bad = wave_sum_i32(bad);
    if (lane == 0) {
        sh.cnt[wave] = cnt;
        sh.bad[wave] = bad;
    }
    __syncthreads();
    int n = 0;
    bad = 0;
#pragma unroll 1
    for (int w = 0; w < kTfWaves; ++w) {
        n += sh.cnt[w];
        bad += sh.bad[w];
    }
    if (bad != 0 || n < 3) return;                                                   // the row stays (block-uniform)

    // ---- phase 2, pass 0: row -> A in phase 1's walk
    tf_scan_hist(sh, tid);
    tf_walk<DT>(r, tid, [&](uint32_t u, bool in) {
        const bool fin = in && (u & KT::kExp) != KT::kExp;
        tf_scatter_round<K>(sh, buf_a, tf_flip<DT>(u), 0, fin, lane, wave);
    });
    // ---- the later passes: wave w owns [w * slice, ...) of the source and walks it in order
    const int slice = (n + kTfWaves - 1) / kTfWaves;
    const int s_lo = wave * slice < n ? wave * slice : n;
    const int s_hi = s_lo + slice < n ? s_lo + slice : n;
    K* src = buf_a;
    K* dst = buf_b;
#pragma unroll 1
    for (int pass = 1; pass < KT::kPasses; ++pass) {
        const int shift = 8 * pass;
        __syncthreads();                                                             // the last scatter is done: its keys are visible
#pragma unroll
        for (int i = 0; i < 4; ++i) sh.hist[tid * 4 + i] = 0u;
        __syncthreads();
        for (int i = s_lo + lane; i < s_hi; i += 64)
            atomicAdd(&sh.hist[((static_cast<uint32_t>(src[i]) >> shift) & 0xFFu) * kTfWaves + wave], 1u);
        tf_scan_hist(sh, tid);
        for (int base = s_lo; base < s_hi; base += 64) {                             // (wave-uniform bounds)
            const int i = base + lane;
            const bool in = i < s_hi;
            tf_scatter_round<K>(sh, dst, in ? static_cast<uint32_t>(src[i]) : 0u, shift, in, lane, wave);
        }
        K* t = src;
        src = dst;
        dst = t;
    }
    __syncthreads();                                                                 // the sorted keys are in `src` (buffer B)
    const K* keys = src;

    // ---- phase 3: the scan.  Lane t owns d2_i for i in [lo, hi), hi <= n - 2
    const double x_max = static_cast<double>(KT::value(tf_flip<DT>(keys[0])));
    const double it = static_cast<double>(inv_t);
    auto weight = [&](int i) { return exp(it * (static_cast<double>(KT::value(tf_flip<DT>(keys[i]))) - x_max)); };
    const int chunk = (n + kTfThreads - 1) / kTfThreads;
    const int lo = tid * chunk < n - 2 ? tid * chunk : n - 2;
    const int hi = lo + chunk < n - 2 ? lo + chunk : n - 2;
    double mine = 0.0;
    if (lo < hi) {
        double w0 = weight(lo), w1 = weight(lo + 1);
#pragma unroll 1
        for (int i = lo; i < hi; ++i) {
            const double w2 = weight(i + 2);
            mine += fabs((w0 - w1) - (w1 - w2));
            w0 = w1;
            w1 = w2;
        }
    }
    const double incl = tf_wave_scan_f64(mine, lane);
    double excl = __shfl_up(incl, 1);
    if (lane == 0) excl = 0.0;
    if (lane == 63) sh.dsum[wave] = incl;
    __syncthreads();
    double S = 0.0, before = 0.0;
#pragma unroll 1
    for (int w = 0; w < kTfWaves; ++w) {
        if (w == wave) before = S;
        S += sh.dsum[w];
    }
    if (!(S > 0.0)) return;                                                          // a flat row (block-uniform)
    const double thr = static_cast<double>(z) * S;
    const double P = before + excl;
    // the first lane whose inclusive sum passes the threshold (the last lane's is S > thr: there is one)
    int first = (P + mine > thr) ? tid : kTfThreads;
    first = wave_min_i32(first);
    if (lane == 0) sh.first[wave] = first;
    __syncthreads();
    first = kTfThreads;
#pragma unroll 1
    for (int w = 0; w < kTfWaves; ++w) first = sh.first[w] < first ? sh.first[w] : first;
    if (tid == first) {                                                              // the same additions: the last partial is `mine`
        double run = 0.0, w0 = weight(lo), w1 = weight(lo + 1);
        int at = hi - 1;
#pragma unroll 1
        for (int i = lo; i < hi; ++i) {
            const double w2 = weight(i + 2);
            run += fabs((w0 - w1) - (w1 - w2));
            if (P + run > thr) {
                at = i;
                break;
            }
            w0 = w1;
            w1 = w2;
        }
        sh.cut_key = static_cast<uint32_t>(keys[at]);
    }
    __syncthreads();
    const float x_cut = KT::value(tf_flip<DT>(sh.cut_key));

    // ---- phase 4: the cut, on stored values
    auto cut = [&](float x) { return x < x_cut && x > -INFINITY; };
    if (tid < r.head && cut(E::scalar(r.rowp, tid))) tf_store_one<DT>(r.rowp, tid);
    const uint32_t end = static_cast<uint32_t>(r.nvec) * 16u;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(r.body, 0, static_cast<int>(end), 0x00020000);
    for (uint32_t base = static_cast<uint32_t>(tid) * 16u; base < end; base += kTfUnroll * kTfStride) {
        u32x4 vec[kTfUnroll];
#pragma unroll
        for (int q = 0; q < kTfUnroll; ++q) vec[q] = load16<false>(rsrc, base + static_cast<uint32_t>(q) * kTfStride);
#pragma unroll
        for (int q = 0; q < kTfUnroll; ++q) {
            const uint32_t off = base + static_cast<uint32_t>(q) * kTfStride;
            if (off < end) {
                float x[N];
                unpack<DT>(vec[q], x);
                uint32_t mask = 0u;
#pragma unroll
                for (int i = 0; i < N; ++i) mask |= (cut(x[i]) ? 1u : 0u) << i;
                tf_store_vec<DT>(r.body + off, vec[q], mask);
            }
        }
    }
    if (tid < r.tail) {
        const int id = r.head + r.nvec * N + tid;
        if (cut(E::scalar(r.rowp, id))) tf_store_one<DT>(r.rowp, id);
    }
}

// one key buffer of a row: V keys, rounded up to 256 bytes
inline uint64_t tf_buf_bytes(int V, int esz) { return (static_cast<uint64_t>(V) * static_cast<uint64_t>(esz) + 255u) & ~uint64_t{255}; }

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT size_t asd_tail_free_workspace_bytes(int B, int K1, int V, int dtype) {
    const int esz = dtype_size(dtype);
    if (B <= 0 || K1 <= 0 || V <= 0 || esz == 0) return 256;
    return static_cast<size_t>(static_cast<uint64_t>(B) * static_cast<uint64_t>(K1) * 2u * tf_buf_bytes(V, esz));
}

ASD_EXPORT int asd_tail_free_rows(void* logits, int dtype, int B, int K1, int V, int64_t ld_seq, int64_t ld_row,
                                  const asd_tail_free_rec* table, void* workspace, size_t workspace_bytes, void* stream) {
    if (B < 0 || K1 < 0 || V < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0 || K1 == 0 || V == 0) return ASD_OK;
    const int esz = dtype_size(dtype);
    if (esz == 0) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(B) * K1 > INT32_MAX) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(V) * esz > INT32_MAX) return ASD_ERR_UNSUPPORTED;       // the sweeps count bytes in 32 bits
    if (!logits || !table || !workspace) return ASD_ERR_INVALID_ARG;
    if (ld_row < V || ld_seq < static_cast<int64_t>(K1) * ld_row) return ASD_ERR_INVALID_ARG;
    if (workspace_bytes < asd_tail_free_workspace_bytes(B, K1, V, dtype)) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(logits, static_cast<size_t>(esz)) || !aligned_to(table, 4) || !aligned_to(workspace, 256)) return ASD_ERR_ALIGNMENT;
    const dim3 grid(static_cast<uint32_t>(static_cast<int64_t>(B) * K1));
    dispatch_dtype(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        hipLaunchKernelGGL((k_tail_free_rows<DT>), grid, dim3(kTfThreads), 0, static_cast<hipStream_t>(stream), logits, ld_seq,
                           ld_row, K1, V, reinterpret_cast<const TfRec*>(table), static_cast<char*>(workspace),
                           tf_buf_bytes(V, esz));
    });
    return launch_status();
}
