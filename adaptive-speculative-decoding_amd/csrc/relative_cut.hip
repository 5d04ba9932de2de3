// relative_cut.hip -- the truncations that cut a row relative to its own statistics (llama.cpp's top_n_sigma and xtc_*,
// koboldcpp's top_a), gfx950.  One in-place pass on the logits behind DRY and ahead of the entropy cuts.
//
// logits[b][j][v] lies at b*ld_seq + j*ld_row + v (asd_entropy_cut_rows' addressing; bf16 / f16 / f32; the first element of a
// row aligned to the element size only).  All K1 rows of sequence b use the record table[b] = {inv_t, mode, a, b}; fin is the
// set of finite elements, a -inf element carries no mass and enters no statistic:
//   mode 1 (top-n-sigma, a = n):  mu = mean over fin, sigma = sqrt(sum_fin (x_v - mu)^2 / |fin|); v is cut iff
//           x_v < fl(x_max - n * sigma).  inv_t is not used.
//   mode 2 (top-a, a = a):        p = softmax(x * inv_t); v is cut iff p_v < a * p_max^2 and x_v < x_max
//   mode 3 (XTC, a = t, b = q):   with the coin c = coins[b][j]: c >= q: nothing.  A = {v : p_v >= t}; |A| < 2: nothing.
//           x_lo = the smallest stored value in A; v is cut iff v in A and x_v > x_lo (every tie at x_lo stays)
//   mode 0: off, the row is not read.  Any other mode, n outside (0, inf), a / t / q outside (0, 1], an inv_t that is not a
//           positive finite number, a NULL coin tensor under mode 3: damaged device data, the row is skipped.
// A cut element becomes -inf of the dtype; nothing else is written (a vector is stored only where a bit of it changes).  A row
// with a NaN or +inf element, or without a finite element, is left as it is.
//
// GEOMETRY.  One workgroup of 1024 lanes per (b, j); lane t owns the 16-byte vectors t, t + 1024, ... of the row's aligned
// body, wave 0's lanes the up to 7 scalar elements in front of and behind it.  Every mode sweeps the row two or three times
// (statistics, a second statistic that needs the first, the cut), so the row is read from HBM ONCE: the RESIDENT kernel
// (rows of at most 19 * 1024 vectors: V <= 155655 in 16 bits, 77827 in f32) loads a lane's vectors into 19 x 4 registers in
// the packed form they have in memory -- all loads in flight at once -- and every later sweep unpacks them from there; the
// cut sweep stores a changed vector from the same registers.  Longer rows take the STREAMING kernel, which walks the row four
// vectors per lane at a time and re-reads it from L2 in the later sweeps.  The launcher chooses by V.
// ORDER.  A lane meets its elements in ascending order (head, its vectors, tail), the lanes of a wave merge by the fixed DPP
// sequence of lse_device.hpp, the sixteen waves in wave order out of LDS: a row's result depends on its bytes, its record
// and its coin only.
// ARITHMETIC.  top-n-sigma: two passes, the mean first (f32 sums in the order above, the count of finite elements an
// integer, mu = float(sum / count) in f64), then sum (x - mu)^2; sigma and the threshold in f64, rounded once to f32 and
// compared with the stored values.  top-a / XTC: (m2, s) by the recurrences of lse_device.hpp and the exact maximum, L = m2 +
// log2 s in two floats, log2 p_v = fma(x_v, c2, -L.hi) - L.lo with c2 = float(log2(e) * inv_t); top-a compares it with
// float(log2 a + 2 (x_max c2 - L)), XTC's membership with float(log2 t).  XTC's count is an integer, its minimum and the
// x_v > x_lo test are exact compares on stored values.

#include <hip/hip_runtime.h>

#include "top_logprobs_device.hpp"
#include "sample_device.hpp"

namespace asd {
namespace {

constexpr int kRcThreads = 1024;
constexpr int kRcWaves = kRcThreads / 64;
constexpr int kRcResVec = 19;                    // 16-byte vectors a lane keeps: 76 dwords
constexpr int kRcUnroll = 4;                     // the streaming kernel: 16-byte loads per lane in flight
constexpr uint32_t kRcStride = kRcThreads * 16u; // bytes between two vectors of one lane

struct RelRec {
    float inv_t;
    int32_t mode;
    float a, b;
};
static_assert(sizeof(RelRec) == ASD_RELATIVE_CUT_REC_BYTES, "RelRec");

// every array is written once per row, by lane 0 of each wave: no reuse, one barrier per reduction
struct RcLds {
    float f0[kRcWaves], f1[kRcWaves], f2[kRcWaves], f3[kRcWaves];
    int i0[kRcWaves], i1[kRcWaves];
};

// a row as the sweeps walk it: `head` scalar elements up to the first 16-byte boundary, nvec vectors, `tail` scalar elements
struct RcRow {
    char* rowp;
    char* body;
    int head, nvec, tail;
};

constexpr int kStream = 0, kFill = 1, kHeld = 2; // a sweep reads memory, reads memory into `res`, or reads `res`

template <int DT>
__device__ __forceinline__ void rc_store_one(char* rowp, int id) {
    using E = Elem<DT>;
    if constexpr (DT == ASD_DTYPE_F32) reinterpret_cast<uint32_t*>(rowp)[id] = E::kNegInfWord;
    else reinterpret_cast<uint16_t*>(rowp)[id] = static_cast<uint16_t>(E::kNegInfWord & 0xFFFFu);
}

// bit i of mask: element i of `vec` becomes -inf; stored (16 bytes, to `dst`) only where a bit of the vector changes
template <int DT>
__device__ __forceinline__ void rc_store_vec(char* dst, const u32x4& vec, uint32_t mask) {
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

// one sweep.  fone(x) -> true: the element becomes -inf.  fvec(x[]) -> bit i set: element i becomes -inf.
template <int DT, int kPath, bool kWrite, class FV, class F1>
__device__ __forceinline__ void rc_sweep(const RcRow& r, int tid, u32x4 (&res)[kRcResVec], FV&& fvec, F1&& fone) {
    using E = Elem<DT>;
    constexpr int N = E::kPerVec;
    auto one = [&](int id) {
        const bool cut = fone(E::scalar(r.rowp, id));
        if constexpr (kWrite) {
            if (cut) rc_store_one<DT>(r.rowp, id);
        }
    };
    if (tid < r.head) one(tid);
    const uint32_t end = static_cast<uint32_t>(r.nvec) * 16u;                        // launcher: V * element size < 2^31
    // (a lane whose offset is >= end gets zeros and makes no memory access)
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(r.body, 0, static_cast<int>(end), 0x00020000);
    auto vec_at = [&](const u32x4& v, uint32_t off) {
        float x[N];
        unpack<DT>(v, x);
        const uint32_t mask = fvec(x);
        if constexpr (kWrite) rc_store_vec<DT>(r.body + off, v, mask);
    };
    if constexpr (kPath == kStream) {
        for (uint32_t base = static_cast<uint32_t>(tid) * 16u; base < end; base += kRcUnroll * kRcStride) {
            u32x4 vec[kRcUnroll];
#pragma unroll
            for (int j = 0; j < kRcUnroll; ++j) vec[j] = load16<false>(rsrc, base + static_cast<uint32_t>(j) * kRcStride);
#pragma unroll
            for (int j = 0; j < kRcUnroll; ++j) {
                const uint32_t off = base + static_cast<uint32_t>(j) * kRcStride;
                if (off < end) vec_at(vec[j], off);
            }
        }
    } else {
        if constexpr (kPath == kFill) {
#pragma unroll
            for (int j = 0; j < kRcResVec; ++j)                                      // the row's one trip to HBM, all in flight
                res[j] = load16<false>(rsrc, static_cast<uint32_t>(tid) * 16u + static_cast<uint32_t>(j) * kRcStride);
        }
#pragma unroll
        for (int j = 0; j < kRcResVec; ++j) {
            const uint32_t off = static_cast<uint32_t>(tid) * 16u + static_cast<uint32_t>(j) * kRcStride;
            if (off < end) vec_at(res[j], off);
        }
    }
    if (tid < r.tail) one(r.head + r.nvec * N + tid);
}

template <int N>
__device__ __forceinline__ float rc_tree_sum(const float (&y)[N]) {
    if constexpr (N == 8) return ((y[0] + y[1]) + (y[2] + y[3])) + ((y[4] + y[5]) + (y[6] + y[7]));
    else return (y[0] + y[1]) + (y[2] + y[3]);
}
template <int N>
__device__ __forceinline__ float rc_tree_max(const float (&x)[N]) {
    if constexpr (N == 8) return fmaxf(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])), fmaxf(fmaxf(x[4], x[5]), fmaxf(x[6], x[7])));
    else return fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
}
__device__ __forceinline__ bool rc_finite(float x) { return fabsf(x) < INFINITY; }   // (false for NaN)

template <int DT, bool kResident>
__global__ __launch_bounds__(kRcThreads) void k_relative_cut_rows(void* logits, int64_t ld_seq, int64_t ld_row, int K1, int V,
                                                                  const RelRec* __restrict__ table,
                                                                  const float* __restrict__ coins, int64_t ld_coin) {
    using E = Elem<DT>;
    constexpr int N = E::kPerVec;
    constexpr int kFirst = kResident ? kFill : kStream, kLater = kResident ? kHeld : kStream;
    __shared__ RcLds sh;

    const int tid = static_cast<int>(threadIdx.x);
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int row = static_cast<int>(blockIdx.x);
    const int b = static_cast<int>(static_cast<uint32_t>(row) / static_cast<uint32_t>(K1));
    const int j = row - b * K1;
    const int mode = table[b].mode;                                                  // (uniform: scalar loads)
    if (mode < ASD_RELCUT_TOP_N_SIGMA || mode > ASD_RELCUT_XTC) return;              // 0: off; anything else: damaged, skipped
    const float inv_t = table[b].inv_t;
    const float va = table[b].a;
    if (!(inv_t > 0.0f && inv_t < 3.0e38f)) return;
    if (mode == ASD_RELCUT_TOP_N_SIGMA ? !(va > 0.0f && va < INFINITY) : !(va > 0.0f && va <= 1.0f)) return;
    if (mode == ASD_RELCUT_XTC) {                                                    // the coin: ahead of the row's first load
        const float q = table[b].b;
        if (!(q > 0.0f && q <= 1.0f) || coins == nullptr) return;
        const float c = coins[static_cast<int64_t>(b) * ld_coin + j];
        if (!(c < q)) return;                                                        // c == q is "no"; so is a NaN
    }

    RcRow r;
    r.rowp = static_cast<char*>(logits) + (static_cast<int64_t>(b) * ld_seq + static_cast<int64_t>(j) * ld_row) * E::kBytes;
    const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(r.rowp) & 15u);     // (a multiple of the element size)
    r.head = mis ? static_cast<int>((16u - mis) / E::kBytes) : 0;
    if (r.head > V) r.head = V;
    r.nvec = (V - r.head) / N;                                                       // resident: <= V / N <= kRcResVec * 1024
    r.tail = V - r.head - r.nvec * N;
    r.body = r.rowp + static_cast<int64_t>(r.head) * E::kBytes;
    u32x4 res[kRcResVec];                                                            // (the streaming kernel never touches it)

    if (mode == ASD_RELCUT_TOP_N_SIGMA) {
        // ---- sweep 1: the sum and the count over fin, the maximum, and whether a NaN or +inf element exists
        float sum = 0.0f, x_max = -INFINITY;
        int cnt = 0, bad = 0;
        auto take = [&](float x) {
            const bool fin = rc_finite(x);
            bad |= !(x < INFINITY) ? 1 : 0;                                          // NaN or +inf
            cnt += fin ? 1 : 0;
            return fin ? x : 0.0f;
        };
        rc_sweep<DT, kFirst, false>(
            r, tid, res,
            [&](const float (&x)[N]) {
                float y[N];
#pragma unroll
                for (int i = 0; i < N; ++i) y[i] = take(x[i]);
                x_max = fmaxf(x_max, rc_tree_max<N>(x));
                sum += rc_tree_sum<N>(y);
                return 0u;
            },
            [&](float x) {
                sum += take(x);
                x_max = fmaxf(x_max, x);
                return false;
            });
        sum = wave_sum(sum);
        x_max = wave_max(x_max);
        cnt = wave_sum_i32(cnt);
        bad = wave_sum_i32(bad);
        if (lane == 0) {
            sh.f0[wave] = sum;
            sh.f1[wave] = x_max;
            sh.i0[wave] = cnt;
            sh.i1[wave] = bad;
        }
        __syncthreads();
        sum = 0.0f;
        x_max = -INFINITY;
        cnt = bad = 0;
#pragma unroll 1
        for (int w = 0; w < kRcWaves; ++w) {
            sum += sh.f0[w];
            x_max = fmaxf(x_max, sh.f1[w]);
            cnt += sh.i0[w];
            bad += sh.i1[w];
        }
        if (bad != 0 || cnt == 0) return;                                            // no distribution: the row stays (uniform)
        const float mu = static_cast<float>(static_cast<double>(sum) / static_cast<double>(cnt));
        // ---- sweep 2: sum over fin of (x - mu)^2
        float sq = 0.0f;
        auto dev2 = [&](float x) {
            const float d = rc_finite(x) ? x - mu : 0.0f;
            return d * d;
        };
        rc_sweep<DT, kLater, false>(
            r, tid, res,
            [&](const float (&x)[N]) {
                float y[N];
#pragma unroll
                for (int i = 0; i < N; ++i) y[i] = dev2(x[i]);
                sq += rc_tree_sum<N>(y);
                return 0u;
            },
            [&](float x) {
                sq += dev2(x);
                return false;
            });
        sq = wave_sum(sq);
        if (lane == 0) sh.f2[wave] = sq;
        __syncthreads();
        sq = 0.0f;
#pragma unroll 1
        for (int w = 0; w < kRcWaves; ++w) sq += sh.f2[w];
        const double sigma = sqrt(static_cast<double>(sq) / static_cast<double>(cnt));
        const float thr = static_cast<float>(static_cast<double>(x_max) - static_cast<double>(va) * sigma);   // one rounding
        if (!(thr == thr)) return;                                                   // (an overflowed sum: inf - inf)
        // ---- sweep 3: the cut, on stored values
        auto cut = [&](float x) { return x < thr && x > -INFINITY; };
        rc_sweep<DT, kLater, true>(
            r, tid, res,
            [&](const float (&x)[N]) {
                uint32_t mask = 0u;
#pragma unroll
                for (int i = 0; i < N; ++i) mask |= (cut(x[i]) ? 1u : 0u) << i;
                return mask;
            },
            [&](float x) { return cut(x); });
        return;
    }

    // ---- top-a and XTC, sweep 1: (m2, s) and the exact maximum
    const float c2 = static_cast<float>(1.4426950408889634074 * static_cast<double>(inv_t));   // log2_scale's own f64 product
    float m2 = kSentinel, s = 0.0f, x_max = -INFINITY;
    rc_sweep<DT, kFirst, false>(
        r, tid, res,
        [&](const float (&x)[N]) {
            x_max = fmaxf(x_max, rc_tree_max<N>(x));
            if constexpr (N == 8) accum8(x, c2, m2, s);
            else accum4(x, c2, m2, s);
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
        sh.f0[wave] = m2;
        sh.f1[wave] = s;
        sh.f2[wave] = x_max;
    }
    __syncthreads();
    float rm2 = kSentinel, rs = 0.0f;
    x_max = -INFINITY;
#pragma unroll 1
    for (int w = 0; w < kRcWaves; ++w) {
        ms_merge(rm2, rs, sh.f0[w], sh.f1[w]);
        x_max = fmaxf(x_max, sh.f2[w]);
    }
    // a NaN or +inf element (NaN sums), no finite element (s == 0), an overflow: the row has no distribution and stays
    if (!(rs > 0.0f) || !(rs < INFINITY) || !(rm2 > kSentinel)) return;              // (block-uniform)
    const double Ld = static_cast<double>(rm2) + log2_split(rs);                     // log2 of the normaliser
    Norm2 L;
    L.hi = static_cast<float>(Ld);
    L.lo = static_cast<float>(Ld - static_cast<double>(L.hi));
    auto log2p = [&](float x) { return fmaf(x, c2, -L.hi) - L.lo; };

    if (mode == ASD_RELCUT_TOP_A) {
        // ---- cut iff log2 p_v < log2 a + 2 log2 p_max and x_v < x_max
        const double lpm = static_cast<double>(x_max) * static_cast<double>(c2) - Ld;
        const float thr = static_cast<float>(log2_split(va) + 2.0 * lpm);
        auto cut = [&](float x) { return log2p(x) < thr && x < x_max && x > -INFINITY; };
        rc_sweep<DT, kLater, true>(
            r, tid, res,
            [&](const float (&x)[N]) {
                uint32_t mask = 0u;
#pragma unroll
                for (int i = 0; i < N; ++i) mask |= (cut(x[i]) ? 1u : 0u) << i;
                return mask;
            },
            [&](float x) { return cut(x); });
        return;
    }

    // ---- XTC, sweep 2: |A| and the smallest stored value of A = {v : log2 p_v >= log2 t}
    const float thr = static_cast<float>(log2_split(va));
    int cnt = 0;
    float lo = INFINITY;
    auto member = [&](float x) { return log2p(x) >= thr; };                          // (false for -inf: log2 p = -inf)
    auto take = [&](float x) {
        const bool in = member(x);
        cnt += in ? 1 : 0;
        lo = in ? fminf(lo, x) : lo;
    };
    rc_sweep<DT, kLater, false>(
        r, tid, res,
        [&](const float (&x)[N]) {
#pragma unroll
            for (int i = 0; i < N; ++i) take(x[i]);
            return 0u;
        },
        [&](float x) {
            take(x);
            return false;
        });
    cnt = wave_sum_i32(cnt);
    lo = -wave_max(-lo);                                                             // the minimum: exact
    if (lane == 0) {
        sh.i0[wave] = cnt;
        sh.f3[wave] = lo;
    }
    __syncthreads();
    cnt = 0;
    lo = INFINITY;
#pragma unroll 1
    for (int w = 0; w < kRcWaves; ++w) {
        cnt += sh.i0[w];
        lo = fminf(lo, sh.f3[w]);
    }
    if (cnt < 2) return;                                                             // nothing to exclude (uniform)
    // ---- sweep 3: every member above the least likely one goes
    const float x_lo = lo;
    auto cut = [&](float x) { return x > x_lo && member(x); };
    rc_sweep<DT, kLater, true>(
        r, tid, res,
        [&](const float (&x)[N]) {
            uint32_t mask = 0u;
#pragma unroll
            for (int i = 0; i < N; ++i) mask |= (cut(x[i]) ? 1u : 0u) << i;
            return mask;
        },
        [&](float x) { return cut(x); });
}

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT int asd_relative_cut_rows(void* logits, int dtype, int B, int K1, int V, int64_t ld_seq, int64_t ld_row,
                                     const asd_relative_cut_rec* table, const float* coins, int64_t ld_coin, void* stream) {
    if (B < 0 || K1 < 0 || V < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0 || K1 == 0 || V == 0) return ASD_OK;
    const int esz = dtype_size(dtype);
    if (esz == 0) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(B) * K1 > INT32_MAX) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(V) * esz > INT32_MAX) return ASD_ERR_UNSUPPORTED;       // the sweeps count bytes in 32 bits
    if (!logits || !table) return ASD_ERR_INVALID_ARG;
    if (ld_row < V || ld_seq < static_cast<int64_t>(K1) * ld_row) return ASD_ERR_INVALID_ARG;
    if (coins && ld_coin < K1) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(logits, static_cast<size_t>(esz)) || !aligned_to(table, 4) || !aligned_to(coins, 4)) return ASD_ERR_ALIGNMENT;
    const dim3 grid(static_cast<uint32_t>(static_cast<int64_t>(B) * K1));
    const bool resident = V / (16 / esz) <= kRcResVec * kRcThreads;                  // every row's nvec <= V / N
    dispatch_dtype(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (resident)
            hipLaunchKernelGGL((k_relative_cut_rows<DT, true>), grid, dim3(kRcThreads), 0, static_cast<hipStream_t>(stream),
                               logits, ld_seq, ld_row, K1, V, reinterpret_cast<const RelRec*>(table), coins, ld_coin);
        else
            hipLaunchKernelGGL((k_relative_cut_rows<DT, false>), grid, dim3(kRcThreads), 0, static_cast<hipStream_t>(stream),
                               logits, ld_seq, ld_row, K1, V, reinterpret_cast<const RelRec*>(table), coins, ld_coin);
    });
    return launch_status();
}
