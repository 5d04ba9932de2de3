// typical_accept.hip -- typical acceptance (Medusa's posterior_threshold / posterior_alpha, vLLM's TypicalAcceptanceSampler),
// gfx950: the one LOSSY verify rule of this library.  A proposal is accepted when the target gives it more than
// min(eps, alpha exp(-H)) of its mass, H the entropy of the target's temperature-scaled row: no uniform, no draft probability.
//
// logits[b][k][v] lies at b*ld_seq + k*ld_row + v (asd_logit_shape_rows' addressing; bf16 / f16 / f32; a row's first element
// aligned to the element size only).  All K rows of sequence b use the record table[b] = {inv_t, ln_eps, ln_alpha, pad}.
//
// TWO STREAM-ORDERED LAUNCHES, nothing else between workgroups: no grid barrier, no poll, no atomic, no last arriver.  What a
// workgroup of the second launch reads was written by workgroups of the first, which the stream has finished; a result is a
// function of the row's bytes, its record and `splits`.
//
// LAUNCH 1, THE SWEEP (k_typical_sweep; the rows' one trip to HBM).  Grid (B*K, splits), 1024 lanes.  A row is cut like
// cfg.hip's: `head` scalar elements up to the first 16-byte boundary, nvec 16-byte vectors, `tail` scalar elements.  Slice sl
// owns the vectors [sl*per, (sl+1)*per) of the body, per = ceil(nvec / splits); slice 0's wave 0 also takes the head and the
// tail.  Lane t owns the slice's vectors t, t + 1024, ...; four 16-byte buffer loads are issued before the first is used, and a
// vector behind the slice's end reads as zeros without a memory access and is not accumulated.
// The record a lane keeps is THREE terms in the log2 domain, y = x c2, c2 = float(log2 e * inv_t):
//     m = max y,   s = sum 2^(y - m),   w = sum (y - m) 2^(y - m)
// (m, s) are lse_device.hpp's recurrences.  w is the third accumulator: when the maximum moves from m to M, d = m - M <= 0,
//     s' = s 2^d,   w' = (w + d s) 2^d
// because every term's (y - m) becomes (y - m) + d.  w is a sum of terms of ONE sign (<= 0) of size at most s / (e ln 2) each,
// so it carries no cancellation, and the entropy needs no x-weighted sum at the row's offset:
//     H = ln 2 (log2 s - w / s)            -- m cancels
// An element at -inf (and one whose 2^(y - m) underflows) adds 0 to both sums: its product (y - m) 2^(y - m) is not formed.
// Lanes merge by the fixed DPP sequence (wave_max, then one rescale per lane and two wave_sums), the sixteen waves in wave order
// out of LDS by wave 0: one barrier.  Thread 0 writes the slice's {m, s, w} to the caller's workspace.
// A NaN or +inf element makes s NaN, which every merge carries to the end.
//
// LAUNCH 2, THE FINISH (k_typical_finish).  One wave per sequence.  Lane k < K merges its row's `splits` records in slice order
// in f64 (the largest m first, then s and w under 2^(m_sl - M), f64 exp2), gathers x_tok itself, forms L, H, lp_t and the
// threshold in f64 and votes; one ballot gives accept_bits and n_acc.
// No scratch; the compiler's register and LDS figures are in DESIGN 4.34.

#include <hip/hip_runtime.h>

#include <float.h>

#include "lse_device.hpp"

namespace asd {
namespace {

constexpr int kTaThreads = 1024;
constexpr int kTaWaves = kTaThreads / 64;
constexpr int kTaUnroll = 4;                                          // 16-byte loads a lane has in flight
constexpr uint32_t kTaStride = kTaThreads * 16u;                      // bytes between two vectors of one lane

struct TaRec {
    float inv_t, ln_eps, ln_alpha, pad;
};
static_assert(sizeof(TaRec) == ASD_TYPICAL_ACCEPT_REC_BYTES, "TaRec");

// one slice's record in the workspace
struct TaPartial {
    float m2, s, w, pad;
};
static_assert(sizeof(TaPartial) == 16, "TaPartial");

// a record the data contract allows (false for NaN anywhere)
__device__ __forceinline__ bool ta_rec_ok(const TaRec& r) {
    return r.inv_t > 0.0f && r.inv_t < 3.0e38f && fabsf(r.ln_eps) < INFINITY && fabsf(r.ln_alpha) < INFINITY;
}
// common.hpp's log2_scale on the device: the same f64 product, rounded once
__device__ __forceinline__ float ta_c2(float inv_t) {
    return static_cast<float>(1.4426950408889634074 * static_cast<double>(inv_t));
}

// (m2, s, w) (+) (m2b, sb, wb)
__device__ __forceinline__ void ta_merge(float& m2, float& s, float& w, float m2b, float sb, float wb) {
    const float M = fmaxf(m2, m2b);
    const float da = m2 - M, db = m2b - M;
    const float ea = fast_exp2(da), eb = fast_exp2(db);
    w = fmaf(fmaf(da, s, w), ea, fmaf(db, sb, wb) * eb);
    s = fmaf(s, ea, sb * eb);
    m2 = M;
}

// N unpacked elements into a lane's record: one move of the maximum per vector
template <int N>
__device__ __forceinline__ void ta_accum(const float (&x)[N], float c2, float& m2, float& s, float& w) {
    float vmax;
    if constexpr (N == 8) {
        vmax = max3(x[0], x[1], x[2]);
        vmax = max3(vmax, x[3], x[4]);
        vmax = max3(vmax, x[5], x[6]);
        vmax = max2(vmax, x[7]);
    } else if constexpr (N == 4) {
        vmax = max2(max3(x[0], x[1], x[2]), x[3]);
    } else {
        vmax = x[0];
    }
    const float M = max2(m2, vmax * c2);
    const float d = m2 - M;
    const float scale = fast_exp2(d);
    float e[N], t[N];
    float ww = 0.0f;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        t[i] = fmaf(x[i], c2, -M);
        e[i] = fast_exp2(t[i]);
        ww = fmaf(e[i] > 0.0f ? t[i] : 0.0f, e[i], ww);              // no mass: no product (-inf * 0)
    }
    float sum;
    if constexpr (N == 8) sum = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
    else if constexpr (N == 4) sum = (e[0] + e[1]) + (e[2] + e[3]);
    else sum = e[0];
    w = fmaf(fmaf(d, s, w), scale, ww);                               // the rescale of the third term: (w + d s) 2^d
    s = fmaf(s, scale, sum);
    m2 = M;
}

template <int DT>
__device__ __forceinline__ void ta_accum_vec(const u32x4& v, float c2, float& m2, float& s, float& w) {
    if constexpr (DT == ASD_DTYPE_F32) {
        float x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = __uint_as_float(v[i]);
        ta_accum<4>(x, c2, m2, s, w);
    } else {
        float x[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[2 * i] = Elem<DT>::from_raw(v[i] & 0xFFFFu);
            x[2 * i + 1] = Elem<DT>::from_raw(v[i] >> 16);
        }
        ta_accum<8>(x, c2, m2, s, w);
    }
}

template <int DT>
__global__ __launch_bounds__(kTaThreads) void k_typical_sweep(const void* logits, int64_t ld_seq, int64_t ld_row, int K, int V,
                                                              int S, const TaRec* __restrict__ table,
                                                              TaPartial* __restrict__ part) {
    using E = Elem<DT>;
    constexpr int N = E::kPerVec;
    __shared__ float sh_m[kTaWaves], sh_s[kTaWaves], sh_w[kTaWaves];

    const int tid = static_cast<int>(threadIdx.x);
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int row = static_cast<int>(blockIdx.x);
    const int sl = static_cast<int>(blockIdx.y);
    const int b = static_cast<int>(static_cast<uint32_t>(row) / static_cast<uint32_t>(K));
    const int k = row - b * K;
    const TaRec rec = table[b];                                                      // (uniform: scalar loads)
    if (!ta_rec_ok(rec)) return;                                                     // damaged: the finish does not read the slot
    const float c2 = ta_c2(rec.inv_t);

    const char* rowp = static_cast<const char*>(logits) +
                       (static_cast<int64_t>(b) * ld_seq + static_cast<int64_t>(k) * ld_row) * E::kBytes;
    const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(rowp) & 15u);        // (a multiple of the element size)
    int head = mis ? static_cast<int>((16u - mis) / E::kBytes) : 0;
    if (head > V) head = V;
    const int nvec = (V - head) / N;
    const int tail = V - head - nvec * N;
    const int per = (nvec + S - 1) / S;
    const int v0 = sl * per < nvec ? sl * per : nvec;
    const int v1 = v0 + per < nvec ? v0 + per : nvec;
    const char* body = rowp + static_cast<int64_t>(head) * E::kBytes + static_cast<int64_t>(v0) * 16;
    const uint32_t end = static_cast<uint32_t>(v1 - v0) * 16u;                       // launcher: V * element size < 2^31
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(body), 0, static_cast<int>(end), 0x00020000);

    float m2 = kSentinel, s = 0.0f, w = 0.0f;
    if (sl == 0 && tid < head) {                                                     // (head, tail <= 7: wave 0)
        const float x[1] = {E::scalar(rowp, tid)};
        ta_accum<1>(x, c2, m2, s, w);
    }
    for (uint32_t base = static_cast<uint32_t>(tid) * 16u; base < end; base += kTaUnroll * kTaStride) {
        u32x4 v[kTaUnroll];
#pragma unroll
        for (int i = 0; i < kTaUnroll; ++i) v[i] = load16<false>(rsrc, base + static_cast<uint32_t>(i) * kTaStride);
#pragma unroll
        for (int i = 0; i < kTaUnroll; ++i)
            if (base + static_cast<uint32_t>(i) * kTaStride < end) ta_accum_vec<DT>(v[i], c2, m2, s, w);
    }
    if (sl == 0 && tid < tail) {
        const float x[1] = {E::scalar(rowp, head + nvec * N + tid)};
        ta_accum<1>(x, c2, m2, s, w);
    }

    // lanes: the fixed DPP sequence; one rescale per lane
    const float M = wave_max(m2);
    const float d = m2 - M;
    const float f = fast_exp2(d);
    w = wave_sum(fmaf(d, s, w) * f);
    s = wave_sum(s * f);
    if (lane == 0) {
        sh_m[wave] = M;
        sh_s[wave] = s;
        sh_w[wave] = w;
    }
    __syncthreads();
    if (wave != 0) return;
    float rm = kSentinel, rs = 0.0f, rw = 0.0f;
#pragma unroll 1
    for (int i = 0; i < kTaWaves; ++i) ta_merge(rm, rs, rw, sh_m[i], sh_s[i], sh_w[i]);           // wave order
    if (tid == 0) {
        TaPartial p;
        p.m2 = rm; p.s = rs; p.w = rw; p.pad = 0.0f;
        part[static_cast<int64_t>(row) * S + sl] = p;
    }
}

template <int DT>
__global__ __launch_bounds__(64) void k_typical_finish(const void* logits, int64_t ld_seq, int64_t ld_row, int K, int V, int S,
                                                       const int32_t* __restrict__ tok, const TaRec* __restrict__ table,
                                                       const TaPartial* __restrict__ part, float* __restrict__ lp_t,
                                                       float* __restrict__ entropy, uint64_t* __restrict__ bits,
                                                       int32_t* __restrict__ n_acc) {
    using E = Elem<DT>;
    const int b = static_cast<int>(blockIdx.x);
    const int lane = static_cast<int>(threadIdx.x);
    const TaRec rec = table[b];
    const bool ok = ta_rec_ok(rec);
    bool accept = false;
    if (lane < K) {
        const int64_t row = static_cast<int64_t>(b) * K + lane;
        double lp = static_cast<double>(NAN), H = static_cast<double>(NAN);
        if (ok) {
            const TaPartial* p = part + row * S;
            float Mf = kSentinel;
            for (int sl = 0; sl < S; ++sl) Mf = fmaxf(Mf, p[sl].m2);
            const double M = static_cast<double>(Mf);
            double ss = 0.0, ww = 0.0;
            for (int sl = 0; sl < S; ++sl) {                                        // slice order
                const double d = static_cast<double>(p[sl].m2) - M;
                const double f = exp2(d);
                const double si = static_cast<double>(p[sl].s);
                ss += si * f;
                ww += (static_cast<double>(p[sl].w) + d * si) * f;
            }
            // ss == 0: no finite element; NaN: a NaN or +inf element, or x c2 beyond f32's range
            if (ss > 0.0 && ss < static_cast<double>(INFINITY)) {
                const double l2s = log2(ss);
                H = kLn2d * (l2s - ww / ss);
                H = H > 0.0 ? H : 0.0;                                              // (rounding below 0 on a one-token row)
                const int t = tok[row];
                lp = -static_cast<double>(INFINITY);
                if (t >= 0 && t < V) {
                    const char* rowp = static_cast<const char*>(logits) +
                                       (static_cast<int64_t>(b) * ld_seq + static_cast<int64_t>(lane) * ld_row) * E::kBytes;
                    const float x = E::scalar(rowp, t);
                    // the SAME c2 the sweep used, so its rounding cancels between y_tok and L
                    if (x > -INFINITY) lp = kLn2d * (static_cast<double>(x) * static_cast<double>(ta_c2(rec.inv_t)) - M - l2s);
                }
                const double a = static_cast<double>(rec.ln_alpha) - H, e = static_cast<double>(rec.ln_eps);
                accept = lp > (e < a ? e : a);                                      // (-inf never accepts)
            }
        }
        lp_t[row] = static_cast<float>(lp);
        entropy[row] = static_cast<float>(H);
    }
    finish_sequence(accept, lane, K, b, n_acc, bits);
}

// the launchers' common size rules; 0: fine
int ta_sizes(int B, int K, int V, int splits) {
    if (B < 0 || K < 0 || V < 0) return ASD_ERR_INVALID_ARG;
    if (K > ASD_TYPICAL_ACCEPT_MAX_K || splits < 0 || splits > ASD_TYPICAL_ACCEPT_MAX_SPLITS) return ASD_ERR_UNSUPPORTED;
    return ASD_OK;
}

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT size_t asd_typical_accept_workspace_bytes(int B, int K, int V, int splits) {
    (void)V;
    if (B <= 0 || K <= 0 || ta_sizes(B, K, V, splits) != ASD_OK) return 256;
    const size_t S = static_cast<size_t>(splits > 0 ? splits : ASD_TYPICAL_ACCEPT_MAX_SPLITS);   // 0: sized for any choice
    return round_up(static_cast<size_t>(B) * static_cast<size_t>(K) * S * sizeof(TaPartial), 256);
}

ASD_EXPORT int asd_typical_accept(const void* logits, int dtype, int B, int K, int V, int64_t ld_seq, int64_t ld_row,
                                  const int32_t* tok, const asd_typical_accept_rec* table, int splits, void* workspace,
                                  float* lp_t, float* entropy, uint64_t* accept_bits, int32_t* n_acc, void* stream) {
    const int rc = ta_sizes(B, K, V, splits);
    if (rc != ASD_OK) return rc;
    if (B == 0) return ASD_OK;
    if (K == 0 || V == 0) return ASD_ERR_INVALID_ARG;
    const int esz = dtype_size(dtype);
    if (esz == 0) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(B) * K * ASD_TYPICAL_ACCEPT_MAX_SPLITS > INT32_MAX) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(V) * esz > INT32_MAX - 16) return ASD_ERR_UNSUPPORTED;  // the sweep counts bytes in 32 bits
    if (!logits || !tok || !table || !workspace || !lp_t || !entropy || !accept_bits || !n_acc) return ASD_ERR_INVALID_ARG;
    if (ld_row < V || ld_seq < static_cast<int64_t>(K) * ld_row) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(logits, static_cast<size_t>(esz)) || !aligned_to(tok, 4) || !aligned_to(table, 16) || !aligned_to(workspace, 16) ||
        !aligned_to(lp_t, 4) || !aligned_to(entropy, 4) || !aligned_to(accept_bits, 8) || !aligned_to(n_acc, 4))
        return ASD_ERR_ALIGNMENT;
    const int64_t R = static_cast<int64_t>(B) * K;
    int S = splits > 0 ? splits : choose_splits(R, V, esz, current_device_cus());
    if (S > ASD_TYPICAL_ACCEPT_MAX_SPLITS) S = ASD_TYPICAL_ACCEPT_MAX_SPLITS;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const TaRec* recs = reinterpret_cast<const TaRec*>(table);
    TaPartial* part = static_cast<TaPartial*>(workspace);
    dispatch_dtype(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        hipLaunchKernelGGL((k_typical_sweep<DT>), dim3(static_cast<uint32_t>(R), static_cast<uint32_t>(S)), dim3(kTaThreads), 0, st,
                           logits, ld_seq, ld_row, K, V, S, recs, part);
        hipLaunchKernelGGL((k_typical_finish<DT>), dim3(static_cast<uint32_t>(B)), dim3(64), 0, st, logits, ld_seq, ld_row, K, V, S,
                           tok, recs, part, lp_t, entropy, accept_bits, n_acc);
    });
    return launch_status();
}
