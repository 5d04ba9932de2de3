// logit_shape.hip -- the samplers that RESHAPE a row instead of cutting it (llama.cpp's / koboldcpp's dynamic temperature,
// text-generation-webui's / koboldcpp's / Aphrodite's quadratic "smooth" sampling), gfx950.  One in-place pass on the logits
// behind the cuts and ahead of the temperature: the first pass of this library that writes a whole row back.
//
// logits[b][j][v] lies at b*ld_seq + j*ld_row + v (asd_relative_cut_rows' addressing; bf16 / f16 / f32; the first element of a
// row aligned to the element size only).  All K1 rows of sequence b use the record table[b] = {mode, T, a, b}; fin is the set
// of finite elements and n = |fin|; a -inf element stays -inf and enters no statistic:
//   mode 1 (dynatemp, T = the row's temperature, a = range r, b = exponent e):  p = softmax(x) over fin at temperature 1,
//           H = -sum p ln p, h = clamp(H / ln n, 0, 1), T_dyn = (T - r) + 2 r h^e, g = float(T / T_dyn); every finite element
//           becomes fl(x_v * g).  n < 2: nothing is written.
//   mode 2 (quadratic, a = factor f, b = curve c):  d = fl(x_v - x_max), k = float(f (3 - c) / 2), s = float(f (c - 1) / 2);
//           every finite element becomes fl(fl(x_max - fl(k fl(d d))) + fl(s fl(fl(d d) d))).  T is not used.
//   mode 0: off, the row is not read.  Any other mode, a T / r / e that is not a positive finite number, r >= T, f outside
//           (0, inf), c outside [1, 3]: damaged device data, the row is skipped.
// The f32 result is rounded to the dtype to nearest even and clamped to the dtype's finite range (a finite element never
// becomes +-inf; a NaN of the polynomial's 0 * inf stands for -inf and becomes the lowest finite value).  A vector is stored
// only where a bit of it changes.  A row with a NaN or +inf element, or without a finite element, is left as it is.
//
// GEOMETRY.  relative_cut.hip's: one workgroup of 1024 lanes per (b, j); lane t owns the 16-byte vectors t, t + 1024, ... of
// the row's aligned body, wave 0's lanes the up to 7 scalar elements in front of and behind it.  Two sweeps, statistics and
// the rewrite, so the row is read from HBM ONCE: the RESIDENT kernel (rows of at most 19 * 1024 vectors: V <= 155655 in 16
// bits, 77827 in f32) loads a lane's vectors into 19 x 4 registers in their packed form -- all loads in flight at once -- and
// the write sweep unpacks vector j, transforms it, repacks it into four fresh registers, compares them with the held four and
// stores: 76 held registers, 8 + 8 + 4 temporaries of one vector at a time and the row's constants stay under the 128 a lane
// of a 1024-lane workgroup has (the held four are dead behind their store; the merge of the waves' partials and the f64 work
// for g run in wave 0 alone, between two barriers, so their registers are not live across the write sweep of every wave).  Longer rows take the STREAMING kernel, which
// walks the row four vectors per lane at a time and re-reads it from L2 in the write sweep.  The launcher chooses by V.
// ORDER.  A lane meets its elements in ascending order (head, its vectors, tail), the lanes of a wave merge by the fixed DPP
// sequence of lse_device.hpp, the sixteen waves in wave order out of LDS (by wave 0, which hands the row's one number -- g or
// x_max -- to the others through LDS): a row's result depends on its bytes and its record.
// ARITHMETIC.  dynatemp: (m2, s, u) by the recurrences of top_logprobs_device.hpp with c2 = float(log2 e), the count an
// integer; H / ln n = (log2_split(s) - u / s) / log2_split(float(n)), h^e, T_dyn and g in f64, g rounded once to f32.
// quadratic: the exact maximum; k and s from f64 products, rounded once.

#include <hip/hip_runtime.h>

#include <float.h>

#include "top_logprobs_device.hpp"
#include "sample_device.hpp"

namespace asd {
namespace {

constexpr int kLsThreads = 1024;
constexpr int kLsWaves = kLsThreads / 64;
constexpr int kLsResVec = 19;                    // 16-byte vectors a lane keeps: 76 dwords
constexpr int kLsUnroll = 4;                     // the streaming kernel: 16-byte loads per lane in flight
constexpr uint32_t kLsStride = kLsThreads * 16u; // bytes between two vectors of one lane

struct ShapeRec {
    int32_t mode;
    float T, a, b;
};
static_assert(sizeof(ShapeRec) == ASD_LOGIT_SHAPE_REC_BYTES, "ShapeRec");

// every array is written once per row, by lane 0 of each wave; go / val once by wave 0: two barriers per row
struct LsLds {
    float m2[kLsWaves], s[kLsWaves], u[kLsWaves], x_max[kLsWaves];
    int cnt[kLsWaves], bad[kLsWaves];
    int go;                                      // wave 0's verdict and number for the row, behind the second barrier
    float val;
};

// a row as the sweeps walk it: `head` scalar elements up to the first 16-byte boundary, nvec vectors, `tail` scalar elements
struct LsRow {
    char* rowp;
    char* body;
    int head, nvec, tail;
};

constexpr int kStream = 0, kFill = 1, kHeld = 2; // a sweep reads memory, reads memory into `res`, or reads `res`

// an f32 result -> the dtype's bits (the low 16 for bf16 / f16): nearest even, clamped to the finite range; NaN -> the lowest
template <int DT>
__device__ __forceinline__ uint32_t ls_round(float y) {
    y = y >= -FLT_MAX ? y : -FLT_MAX;                                                // (-inf and NaN)
    y = y <= FLT_MAX ? y : FLT_MAX;
    if constexpr (DT == ASD_DTYPE_F32) {
        return __float_as_uint(y);
    } else if constexpr (DT == ASD_DTYPE_BF16) {
        uint32_t w = __float_as_uint(y);
        w = (w + 0x7FFFu + ((w >> 16) & 1u)) >> 16;
        return (w & 0x7F80u) == 0x7F80u ? (w & 0x8000u) | 0x7F7Fu : w;               // rounded up to inf: the largest finite
    } else {
        const uint32_t w = __builtin_bit_cast(uint16_t, static_cast<_Float16>(y));  // v_cvt_f16_f32: nearest even
        return (w & 0x7C00u) == 0x7C00u ? (w & 0x8000u) | 0x7BFFu : w;
    }
}

// the statistics sweep: fvec(x[]) per vector, fone(x) per head / tail element
template <int DT, int kPath, class FV, class F1>
__device__ __forceinline__ void ls_sweep(const LsRow& r, int tid, u32x4 (&res)[kLsResVec], FV&& fvec, F1&& fone) {
    using E = Elem<DT>;
    constexpr int N = E::kPerVec;
    if (tid < r.head) fone(E::scalar(r.rowp, tid));
    const uint32_t end = static_cast<uint32_t>(r.nvec) * 16u;                        // launcher: V * element size < 2^31
    // (a lane whose offset is >= end gets zeros and makes no memory access)
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(r.body, 0, static_cast<int>(end), 0x00020000);
    auto vec_at = [&](const u32x4& v) {
        float x[N];
        unpack<DT>(v, x);
        fvec(x);
    };
    if constexpr (kPath == kStream) {
        for (uint32_t base = static_cast<uint32_t>(tid) * 16u; base < end; base += kLsUnroll * kLsStride) {
            u32x4 vec[kLsUnroll];
#pragma unroll
            for (int j = 0; j < kLsUnroll; ++j) vec[j] = load16<false>(rsrc, base + static_cast<uint32_t>(j) * kLsStride);
#pragma unroll
            for (int j = 0; j < kLsUnroll; ++j)
                if (base + static_cast<uint32_t>(j) * kLsStride < end) vec_at(vec[j]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < kLsResVec; ++j)                                          // the row's one trip to HBM, all in flight
            res[j] = load16<false>(rsrc, static_cast<uint32_t>(tid) * 16u + static_cast<uint32_t>(j) * kLsStride);
#pragma unroll
        for (int j = 0; j < kLsResVec; ++j)
            if (static_cast<uint32_t>(tid) * 16u + static_cast<uint32_t>(j) * kLsStride < end) vec_at(res[j]);
    }
    if (tid < r.tail) fone(E::scalar(r.rowp, r.head + r.nvec * N + tid));
}

// the write sweep: f(x) -> the element's new f32 value.  Unpack, transform, round, repack; 16 bytes are stored where the
// repacked vector differs from the one read, a head / tail element where its own bits do.  A -inf element keeps its bits.
template <int DT, int kPath, class F>
__device__ __forceinline__ void ls_write(const LsRow& r, int tid, u32x4 (&res)[kLsResVec], F&& f) {
    using E = Elem<DT>;
    constexpr int N = E::kPerVec;
    auto one = [&](int id) {
        const uint32_t old = E::raw(r.rowp, id);
        const float x = E::from_raw(old);
        if (!(x > -INFINITY)) return;
        const uint32_t now = ls_round<DT>(f(x));
        if (now == old) return;
        if constexpr (DT == ASD_DTYPE_F32) reinterpret_cast<uint32_t*>(r.rowp)[id] = now;
        else reinterpret_cast<uint16_t*>(r.rowp)[id] = static_cast<uint16_t>(now);
    };
    auto vec_at = [&](const u32x4& v, uint32_t off) {
        float x[N];
        unpack<DT>(v, x);
        u32x4 w;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (N == 8) {
                const uint32_t lo = x[2 * i] > -INFINITY ? ls_round<DT>(f(x[2 * i])) : (v[i] & 0xFFFFu);
                const uint32_t hi = x[2 * i + 1] > -INFINITY ? ls_round<DT>(f(x[2 * i + 1])) : (v[i] >> 16);
                w[i] = lo | (hi << 16);
            } else {
                w[i] = x[i] > -INFINITY ? ls_round<DT>(f(x[i])) : v[i];
            }
        }
        const bool same = w[0] == v[0] && w[1] == v[1] && w[2] == v[2] && w[3] == v[3];
        if (!same) *reinterpret_cast<u32x4*>(r.body + off) = w;
    };
    if (tid < r.head) one(tid);
    const uint32_t end = static_cast<uint32_t>(r.nvec) * 16u;
    if constexpr (kPath == kStream) {
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(r.body, 0, static_cast<int>(end), 0x00020000);
        for (uint32_t base = static_cast<uint32_t>(tid) * 16u; base < end; base += kLsUnroll * kLsStride) {
            u32x4 vec[kLsUnroll];
#pragma unroll
            for (int j = 0; j < kLsUnroll; ++j) vec[j] = load16<false>(rsrc, base + static_cast<uint32_t>(j) * kLsStride);
#pragma unroll
            for (int j = 0; j < kLsUnroll; ++j) {
                const uint32_t off = base + static_cast<uint32_t>(j) * kLsStride;
                if (off < end) vec_at(vec[j], off);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < kLsResVec; ++j) {
            const uint32_t off = static_cast<uint32_t>(tid) * 16u + static_cast<uint32_t>(j) * kLsStride;
            if (off < end) vec_at(res[j], off);
        }
    }
    if (tid < r.tail) one(r.head + r.nvec * N + tid);
}

template <int N>
__device__ __forceinline__ float ls_tree_max(const float (&x)[N]) {
    if constexpr (N == 8) return fmaxf(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])), fmaxf(fmaxf(x[4], x[5]), fmaxf(x[6], x[7])));
    else return fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
}

// sweep 1's accumulate of one vector: accum_top<N, kStatsOnly>'s operations on (m2, s, u)
template <int N>
__device__ __forceinline__ void ls_accum(const float (&x)[N], float vmax, float c2, float& m2, float& s, float& u) {
    const float M = fmaxf(m2, vmax * c2);
    const float scale = fast_exp2(m2 - M);
    float e[N];
    float w = 0.0f;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float d = fmaf(x[i], c2, -M);
        e[i] = fast_exp2(d);
        w = fmaf(e[i], e[i] > 0.0f ? d : 0.0f, w);
    }
    u = rebase_u(u, s, m2, M, scale) + w;
    float sum;
    if constexpr (N == 8) sum = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
    else sum = (e[0] + e[1]) + (e[2] + e[3]);
    s = fmaf(s, scale, sum);
    m2 = M;
}

template <int DT, bool kResident>
__global__ __launch_bounds__(kLsThreads) void k_logit_shape_rows(void* logits, int64_t ld_seq, int64_t ld_row, int K1, int V,
                                                                 const ShapeRec* __restrict__ table) {
    using E = Elem<DT>;
    constexpr int N = E::kPerVec;
    constexpr int kFirst = kResident ? kFill : kStream, kLater = kResident ? kHeld : kStream;
    __shared__ LsLds sh;

    const int tid = static_cast<int>(threadIdx.x);
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int row = static_cast<int>(blockIdx.x);
    const int b = static_cast<int>(static_cast<uint32_t>(row) / static_cast<uint32_t>(K1));
    const int j = row - b * K1;
    const int mode = table[b].mode;                                                  // (uniform: scalar loads)
    if (mode != ASD_SHAPE_DYNATEMP && mode != ASD_SHAPE_QUADRATIC) return;           // 0: off; anything else: damaged, skipped
    const float T = table[b].T;
    const float va = table[b].a;
    const float vb = table[b].b;
    if (!(va > 0.0f && va < INFINITY)) return;
    if (mode == ASD_SHAPE_DYNATEMP) {
        if (!(T > 0.0f && T < INFINITY) || !(va < T) || !(vb > 0.0f && vb < INFINITY)) return;
    } else if (!(vb >= 1.0f && vb <= 3.0f)) {
        return;
    }

    LsRow r;
    r.rowp = static_cast<char*>(logits) + (static_cast<int64_t>(b) * ld_seq + static_cast<int64_t>(j) * ld_row) * E::kBytes;
    const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(r.rowp) & 15u);     // (a multiple of the element size)
    r.head = mis ? static_cast<int>((16u - mis) / E::kBytes) : 0;
    if (r.head > V) r.head = V;
    r.nvec = (V - r.head) / N;                                                       // resident: <= V / N <= kLsResVec * 1024
    r.tail = V - r.head - r.nvec * N;
    r.body = r.rowp + static_cast<int64_t>(r.head) * E::kBytes;
    u32x4 res[kLsResVec];                                                            // (the streaming kernel never touches it)

    // ---- sweep 1: the count of finite elements, the NaN / +inf flag, the exact maximum; dynatemp: (m2, s, u) at temperature 1
    const bool dyn = mode == ASD_SHAPE_DYNATEMP;                                     // (uniform)
    float m2 = kSentinel, s = 0.0f, u = 0.0f, x_max = -INFINITY;
    int cnt = 0, bad = 0;
    auto take = [&](float x) {
        bad |= !(x < INFINITY) ? 1 : 0;                                              // NaN or +inf
        cnt += fabsf(x) < INFINITY ? 1 : 0;
    };
    ls_sweep<DT, kFirst>(
        r, tid, res,
        [&](const float (&x)[N]) {
#pragma unroll
            for (int i = 0; i < N; ++i) take(x[i]);
            const float vmax = ls_tree_max<N>(x);
            x_max = fmaxf(x_max, vmax);
            if (dyn) ls_accum<N>(x, vmax, kLog2e, m2, s, u);
        },
        [&](float x) {                                                               // accum_one<kStatsOnly>'s operations
            take(x);
            x_max = fmaxf(x_max, x);
            if (dyn) {
                const float M = max2(m2, x * kLog2e);
                const float scale = fast_exp2(m2 - M);
                const float d = fmaf(x, kLog2e, -M);
                const float e = fast_exp2(d);
                u = fmaf(e, e > 0.0f ? d : 0.0f, rebase_u(u, s, m2, M, scale));
                s = fmaf(s, scale, e);
                m2 = M;
            }
        });
    if (dyn) wave_merge_u(m2, s, u);
    x_max = wave_max(x_max);
    cnt = wave_sum_i32(cnt);
    bad = wave_sum_i32(bad);
    if (lane == 0) {
        sh.m2[wave] = m2;
        sh.s[wave] = s;
        sh.u[wave] = u;
        sh.x_max[wave] = x_max;
        sh.cnt[wave] = cnt;
        sh.bad[wave] = bad;
    }
    __syncthreads();
    // ---- wave 0 alone merges the sixteen partials in wave order and forms the row's one number -- g (dynatemp) or x_max
    // (quadratic) -- ONCE; the others wait at a second barrier: no f64 work and no merge registers in fifteen of sixteen waves
    if (wave == 0) {
        float rm2 = kSentinel, rs = 0.0f, ru = 0.0f;
        x_max = -INFINITY;
        cnt = bad = 0;
#pragma unroll 1
        for (int w = 0; w < kLsWaves; ++w) {
            if (dyn) ms_merge_u(rm2, rs, ru, sh.m2[w], sh.s[w], sh.u[w]);
            x_max = fmaxf(x_max, sh.x_max[w]);
            cnt += sh.cnt[w];
            bad += sh.bad[w];
        }
        bool go = bad == 0 && cnt != 0;                                              // else no distribution: the row stays
        float val = x_max;
        if (go && dyn) {
            // n < 2: ln n == 0, nothing to scale by; sums that overflowed f32 (|x| log2 e beyond its range): the row stays
            go = cnt >= 2 && rs > 0.0f && rs < INFINITY && ru == ru;
            // g in f64 from the f32 statistics
            const double H2 = log2_split(rs) - static_cast<double>(ru) / static_cast<double>(rs);    // the entropy in bits
            double h = H2 / log2_split(static_cast<float>(cnt));                     // (the same logarithm: a uniform row gives 1)
            h = h > 0.0 ? (h < 1.0 ? h : 1.0) : 0.0;
            const double t_dyn = (static_cast<double>(T) - static_cast<double>(va)) +
                                 2.0 * static_cast<double>(va) * pow(h, static_cast<double>(vb));
            val = static_cast<float>(static_cast<double>(T) / t_dyn);
            go = go && val > 0.0f && val < INFINITY && val != 1.0f;                  // g == 1: every element keeps its bits
        }
        if (lane == 0) {
            sh.go = go ? 1 : 0;
            sh.val = val;
        }
    }
    __syncthreads();
    if (sh.go == 0) return;                                                          // (block-uniform)
    if (dyn) {
        const float g = sh.val;
        ls_write<DT, kLater>(r, tid, res, [&](float x) { return x * g; });
        return;
    }
    x_max = sh.val;

    // ---- quadratic: x_max - k d^2 + s d^3 around the exact maximum
    const float k = static_cast<float>(static_cast<double>(va) * (3.0 - static_cast<double>(vb)) * 0.5);
    const float sc = static_cast<float>(static_cast<double>(va) * (static_cast<double>(vb) - 1.0) * 0.5);
    ls_write<DT, kLater>(r, tid, res, [&](float x) {
        const float d = x - x_max;
        const float d2 = d * d;
        return (x_max - k * d2) + sc * (d2 * d);
    });
}

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT int asd_logit_shape_rows(void* logits, int dtype, int B, int K1, int V, int64_t ld_seq, int64_t ld_row,
                                    const asd_logit_shape_rec* table, void* stream) {
    if (B < 0 || K1 < 0 || V < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0 || K1 == 0 || V == 0) return ASD_OK;
    const int esz = dtype_size(dtype);
    if (esz == 0) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(B) * K1 > INT32_MAX) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(V) * esz > INT32_MAX) return ASD_ERR_UNSUPPORTED;       // the sweeps count bytes in 32 bits
    if (!logits || !table) return ASD_ERR_INVALID_ARG;
    if (ld_row < V || ld_seq < static_cast<int64_t>(K1) * ld_row) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(logits, static_cast<size_t>(esz)) || !aligned_to(table, 4)) return ASD_ERR_ALIGNMENT;
    const dim3 grid(static_cast<uint32_t>(static_cast<int64_t>(B) * K1));
    const bool resident = V / (16 / esz) <= kLsResVec * kLsThreads;                  // every row's nvec <= V / N
    dispatch_dtype(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (resident)
            hipLaunchKernelGGL((k_logit_shape_rows<DT, true>), grid, dim3(kLsThreads), 0, static_cast<hipStream_t>(stream), logits,
                               ld_seq, ld_row, K1, V, reinterpret_cast<const ShapeRec*>(table));
        else
            hipLaunchKernelGGL((k_logit_shape_rows<DT, false>), grid, dim3(kLsThreads), 0, static_cast<hipStream_t>(stream), logits,
                               ld_seq, ld_row, K1, V, reinterpret_cast<const ShapeRec*>(table));
    });
    return launch_status();
}
