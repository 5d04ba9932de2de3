// entropy_cut.hip -- the entropy-aware truncations ahead of the samplers (HF's TypicalLogitsWarper, EpsilonLogitsWarper and
// EtaLogitsWarper with min_tokens_to_keep = 1), gfx950.  One in-place pass on the logits, like the mask, ban and edit kernels.
//
// logits[b][j][v] lies at b*ld_seq + j*ld_row + v (asd_no_repeat_ngram_rows' addressing; bf16 / f16 / f32; the first element of
// a row aligned to the element size only).  All K1 rows of sequence b use the record table[b] = {inv_t, mode, value}.  With
// p = softmax(x * inv_t) of the row as it stands and H = -sum p ln p:
//   mode 1 (typical_p = value = m): d_v = |-ln p_v - H|; d* = the smallest value with sum{p_v : d_v <= d*} >= m; v is cut iff
//           d_v > d* (every tie at d* is kept; the arg-max may be cut); the mass never reaches m: nothing is cut
//   mode 2 (epsilon_cutoff = value = e): v is cut iff p_v < e and x_v < x_max
//   mode 3 (eta_cutoff = value = e): the same with min(e, sqrt(e) exp(-H)) in place of e
//   mode 0: off, the row is not read.  Any other mode, a value outside (0, 1), an inv_t that is not a positive finite number:
//           damaged device data, the row is skipped.
// A cut element becomes -inf of the dtype; nothing else is written (a vector is stored only where a bit of it changes).  A row
// with a NaN or +inf element, or without a finite element, is left as it is: its sums are NaN, infinite or 0.
//
// One workgroup of 1024 lanes per (b, j).  SWEEP 1 (the only read that goes to HBM) takes (m2, s, u) by the recurrences of
// top_logprobs_device.hpp -- u the entropy's running sum relative to the running maximum -- and the exact maximum x_max of the
// stored values: a lane meets its vectors in ascending order, lanes merge by the fixed DPP sequence, waves in wave order out of
// LDS; never arrival order.  From them L = m2 + log2 s (two floats, Norm2) and H2 = log2 s - u / s (bits).  Everything behind it
// is in the log2 domain with the stream's own c2: log2 p_v = fma(x_v, c2, -L.hi) - L.lo.
// EPSILON / ETA: one more sweep (L2) compares log2 p_v with log2 of the bound.
// TYPICAL: the key of v is k_v = |fma(x_v, c2, -A.hi) - A.lo| with A = L - H2 (so d_v = ln2 k_v), and the select is the mass
// select of sample_device.hpp turned round: ascending on order_key(k_v), 12 + 12 + 8 bits, every level one sweep that adds the
// elements' masses floor(p_v 2^40) to integer counters in LDS (integer adds commute: the counters do not depend on the order
// the lanes arrive in) and one scan that finds the digit where the running mass reaches floor(m 2^40).  A last sweep cuts the
// elements whose key is above the selected one.  The result depends on the row's bytes and its record only.

#include <hip/hip_runtime.h>

#include "top_logprobs_device.hpp"
#include "sample_device.hpp"

namespace asd {
namespace {

constexpr int kCutThreads = 1024;
constexpr int kCutWaves = kCutThreads / 64;
constexpr int kCutUnroll = 4;                    // 16-byte loads per lane in flight

struct CutRec {
    float inv_t;
    int32_t mode;
    float value;
};
static_assert(sizeof(CutRec) == ASD_ENTROPY_CUT_REC_BYTES, "CutRec");

struct CutLds {
    unsigned long long hist[kDsDigits];          // masses per digit, 2^-40 fixed point
    unsigned long long wave_tot[kCutWaves];
    unsigned long long sel_below;
    float meet[kCutWaves][4];                    // m2, s, u, x_max of every wave
    int sel_digit;
};

// a row as the sweeps walk it: `head` scalar elements up to the first 16-byte boundary, nvec vectors, `tail` scalar elements
struct RowWalk {
    char* rowp;
    char* body;
    int head, nvec, tail;
};

// one sweep: wave 0's lanes take the head and the tail, lane t the vectors t, t + 1024, ... in ascending order.
// fone(x, id) -> true: the element becomes -inf.  fvec(x[], id0) -> bit i set: element i becomes -inf.
template <int DT, bool kWrite, class FV, class F1>
__device__ __forceinline__ void cut_sweep(const RowWalk& r, int tid, FV&& fvec, F1&& fone) {
    using E = Elem<DT>;
    constexpr int N = E::kPerVec;
    auto one = [&](int id) {
        const bool cut = fone(E::scalar(r.rowp, id), id);
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
    for (uint32_t base = static_cast<uint32_t>(tid) * 16u; base < end; base += kCutUnroll * kCutThreads * 16u) {
        u32x4 vec[kCutUnroll];
#pragma unroll
        for (int j = 0; j < kCutUnroll; ++j) vec[j] = load16<false>(rsrc, base + static_cast<uint32_t>(j) * (kCutThreads * 16u));
#pragma unroll
        for (int j = 0; j < kCutUnroll; ++j) {
            const uint32_t off = base + static_cast<uint32_t>(j) * (kCutThreads * 16u);
            if (off >= end) continue;
            float x[N];
            unpack<DT>(vec[j], x);
            const uint32_t mask = fvec(x, r.head + static_cast<int>(off >> 4) * N);
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

// sweep 1's accumulate of one vector: accum_top<N, kStatsOnly>'s operations on (m2, s, u), and the exact maximum
template <int N>
__device__ __forceinline__ void cut_accum(const float (&x)[N], float c2, float& m2, float& s, float& u, float& x_max) {
    float vmax;
    if constexpr (N == 8) vmax = fmaxf(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])), fmaxf(fmaxf(x[4], x[5]), fmaxf(x[6], x[7])));
    else vmax = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
    x_max = fmaxf(x_max, vmax);
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

template <int DT>
__global__ __launch_bounds__(kCutThreads) void k_entropy_cut_rows(void* logits, int64_t ld_seq, int64_t ld_row, int K1, int V,
                                                                  const CutRec* __restrict__ table) {
    using E = Elem<DT>;
    constexpr int N = E::kPerVec;
    __shared__ CutLds sh;

    const int tid = static_cast<int>(threadIdx.x);
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int row = static_cast<int>(blockIdx.x);
    const int b = static_cast<int>(static_cast<uint32_t>(row) / static_cast<uint32_t>(K1));
    const int j = row - b * K1;
    const int mode = table[b].mode;                                                  // (uniform: scalar loads)
    if (mode < ASD_CUT_TYPICAL || mode > ASD_CUT_ETA) return;                        // 0: off; anything else: damaged, skipped
    const float inv_t = table[b].inv_t;
    const float value = table[b].value;
    if (!(inv_t > 0.0f && inv_t < 3.0e38f) || !(value > 0.0f && value < 1.0f)) return;
    const float c2 = static_cast<float>(1.4426950408889634074 * static_cast<double>(inv_t));   // log2_scale's own f64 product

    RowWalk r;
    r.rowp = static_cast<char*>(logits) + (static_cast<int64_t>(b) * ld_seq + static_cast<int64_t>(j) * ld_row) * E::kBytes;
    const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(r.rowp) & 15u);     // (a multiple of the element size)
    r.head = mis ? static_cast<int>((16u - mis) / E::kBytes) : 0;
    if (r.head > V) r.head = V;
    r.nvec = (V - r.head) / N;
    r.tail = V - r.head - r.nvec * N;
    r.body = r.rowp + static_cast<int64_t>(r.head) * E::kBytes;

    // ---- sweep 1: (m2, s, u) and x_max; lanes -> wave (DPP), waves -> row (wave order, out of LDS)
    float m2 = kSentinel, s = 0.0f, u = 0.0f, x_max = -INFINITY;
    cut_sweep<DT, false>(
        r, tid,
        [&](const float (&x)[N], int) {
            cut_accum<N>(x, c2, m2, s, u, x_max);
            return 0u;
        },
        [&](float x, int) {                                                          // accum_one<kStatsOnly>'s operations
            x_max = fmaxf(x_max, x);
            const float M = max2(m2, x * c2);
            const float scale = fast_exp2(m2 - M);
            const float d = fmaf(x, c2, -M);
            const float e = fast_exp2(d);
            u = fmaf(e, e > 0.0f ? d : 0.0f, rebase_u(u, s, m2, M, scale));
            s = fmaf(s, scale, e);
            m2 = M;
            return false;
        });
    wave_merge_u(m2, s, u);
    x_max = wave_max(x_max);
    if (lane == 0) {
        sh.meet[wave][0] = m2;
        sh.meet[wave][1] = s;
        sh.meet[wave][2] = u;
        sh.meet[wave][3] = x_max;
    }
    __syncthreads();
    float rm2 = kSentinel, rs = 0.0f, ru = 0.0f;
    x_max = -INFINITY;
#pragma unroll 1
    for (int w = 0; w < kCutWaves; ++w) {                                            // (a loop: sixteen merges in flight cost registers)
        ms_merge_u(rm2, rs, ru, sh.meet[w][0], sh.meet[w][1], sh.meet[w][2]);
        x_max = fmaxf(x_max, sh.meet[w][3]);
    }
    // a NaN or +inf element (NaN sums), no finite element (s == 0), an overflow: the row has no distribution and stays
    if (!(rs > 0.0f) || !(rs < INFINITY) || !(ru == ru) || !(rm2 > kSentinel)) return;           // (block-uniform)
    const double l2s = log2_split(rs);
    const double Ld = static_cast<double>(rm2) + l2s;                                // log2 of the normaliser
    const double H2 = l2s - static_cast<double>(ru) / static_cast<double>(rs);       // the entropy in bits
    Norm2 L;
    L.hi = static_cast<float>(Ld);
    L.lo = static_cast<float>(Ld - static_cast<double>(L.hi));

    if (mode != ASD_CUT_TYPICAL) {
        // ---- epsilon / eta: cut iff log2 p_v < log2 bound and x_v < x_max
        double t2 = log2_split(value);
        if (mode == ASD_CUT_ETA) {
            const double alt = 0.5 * t2 - H2;                                        // log2(sqrt(e) exp(-H))
            t2 = alt < t2 ? alt : t2;
        }
        const float thr = static_cast<float>(t2);
        auto cut = [&](float x) { return (fmaf(x, c2, -L.hi) - L.lo) < thr && x < x_max; };
        cut_sweep<DT, true>(
            r, tid,
            [&](const float (&x)[N], int) {
                uint32_t mask = 0u;
#pragma unroll
                for (int i = 0; i < N; ++i) mask |= (cut(x[i]) ? 1u : 0u) << i;
                return mask;
            },
            [&](float x, int) { return cut(x); });
        return;
    }

    // ---- typical: ascending radix select on order_key(k_v) by mass
    const double Ad = Ld - H2;
    Norm2 A;
    A.hi = static_cast<float>(Ad);
    A.lo = static_cast<float>(Ad - static_cast<double>(A.hi));
    auto key_of = [&](float x) { return order_key(fabsf(fmaf(x, c2, -A.hi) - A.lo)); };
    unsigned long long target = static_cast<unsigned long long>(static_cast<double>(value) * static_cast<double>(kDsFix));
    if (target == 0ull) target = 1ull;
    unsigned long long below = 0ull;
    uint32_t prefix = 0u;
    const int shifts[3] = {20, 8, 0}, widths[3] = {12, 12, 8};
#pragma unroll 1
    for (int lv = 0; lv < 3; ++lv) {
        const int shift = shifts[lv], digits = 1 << widths[lv], hi_shift = shifts[lv] + widths[lv];
        for (int i = tid; i < digits; i += kCutThreads) sh.hist[i] = 0ull;
        if (tid == 0) sh.sel_digit = -1;
        __syncthreads();
        auto add_mass = [&](float x) {
            const uint32_t key = key_of(x);
            const bool mine = hi_shift >= 32 || (key >> hi_shift) == (prefix >> hi_shift);
            if (!mine) return;
            const unsigned long long mass = mass_fixed40(fast_exp2(fmaf(x, c2, -L.hi) - L.lo));
            if (mass > 0ull) atomicAdd(&sh.hist[(key >> shift) & static_cast<uint32_t>(digits - 1)], mass);
        };
        cut_sweep<DT, false>(
            r, tid,
            [&](const float (&x)[N], int) {
#pragma unroll
                for (int i = 0; i < N; ++i) add_mass(x[i]);
                return 0u;
            },
            [&](float x, int) {
                add_mass(x);
                return false;
            });
        __syncthreads();
        // thread t owns the t-th chunk of digits counted from the BOTTOM
        const int per = digits >= kCutThreads ? digits / kCutThreads : 1;
        const int lo = tid * per, hi = lo + per;
        const bool owner = lo < digits;
        unsigned long long mine = 0ull;
        if (owner)
            for (int d = lo; d < hi; ++d) mine += sh.hist[d];
        const unsigned long long incl = wave_incl_scan_u64(mine, lane);
        if (lane == 63) sh.wave_tot[wave] = incl;
        __syncthreads();
        unsigned long long base = 0ull, total = 0ull;
#pragma unroll
        for (int w = 0; w < kCutWaves; ++w) {
            if (w < wave) base += sh.wave_tot[w];
            total += sh.wave_tot[w];
        }
        if (lv == 0 && total < target) return;                                       // the mass never reaches m: all kept (uniform)
        const unsigned long long before = below + base + incl - mine;
        if (owner && mine > 0ull && before < target && target <= before + mine) {    // exactly one thread
            unsigned long long acc = before;
            int pick = hi - 1;
            for (int d = lo; d < hi; ++d) {
                const unsigned long long m = sh.hist[d];
                if (m > 0ull && acc + m >= target) { pick = d; break; }
                acc += m;
            }
            sh.sel_digit = pick;
            sh.sel_below = acc;
        }
        __syncthreads();
        const int dg = sh.sel_digit;
        if (dg < 0) return;                                                          // (cannot happen: the levels add the same integers)
        prefix |= static_cast<uint32_t>(dg) << shift;
        below = sh.sel_below;
        __syncthreads();                                                             // sel_* and hist are rewritten by the next level
    }
    cut_sweep<DT, true>(
        r, tid,
        [&](const float (&x)[N], int) {
            uint32_t mask = 0u;
#pragma unroll
            for (int i = 0; i < N; ++i) mask |= (key_of(x[i]) > prefix ? 1u : 0u) << i;
            return mask;
        },
        [&](float x, int) { return key_of(x) > prefix; });
}

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT int asd_entropy_cut_rows(void* logits, int dtype, int B, int K1, int V, int64_t ld_seq, int64_t ld_row,
                                    const asd_entropy_cut_rec* table, void* stream) {
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
    dispatch_dtype(dtype, [&](auto dt) {
        hipLaunchKernelGGL((k_entropy_cut_rows<decltype(dt)::value>), grid, dim3(kCutThreads), 0, static_cast<hipStream_t>(stream),
                           logits, ld_seq, ld_row, K1, V, reinterpret_cast<const CutRec*>(table));
    });
    return launch_status();
}
