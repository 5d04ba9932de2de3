// cfg.hip -- classifier-free guidance (HF generate's guidance_scale / negative_prompt_ids, llama.cpp's / koboldcpp's /
// ExLlamaV2's cfg-scale with a negative prompt), gfx950.  One launch turns a CONDITIONAL row c and an UNCONDITIONAL row u
// into the guided row, in place over c, ahead of every other processor:
//     g = u' + s (c' - u'),    c' = log_softmax(c),  u' = log_softmax(u)
// It is the first pass of this library that reads TWO rows per workgroup.
//
// cond[b][j][v] lies at b*ld_seq + j*ld_row + v (asd_logit_shape_rows' addressing; bf16 / f16 / f32; the first element of a row
// aligned to the element size only); uncond[q][j][v] at q*ld_useq + j*ld_urow + v from a base of its own.  All K1 rows of
// sequence b use the record table[b] = {scale s, uncond_seq q}.  q < 0 or s == 1: the sequence is off, nothing of it is read.
// s not in [0, 100] (NaN included) or q >= Bu: damaged device data, the sequence is skipped.  Per element of a row pair, with
// Lc = float(ln sum exp c) and Lu = float(ln sum exp u) over the rows' finite elements, c'_v = fl(c_v - Lc), u'_v = fl(u_v - Lu)
// and t = fl(1 - s):
//   c_v == -inf                    ->  -inf (the bits stay)
//   u_v == -inf, c_v finite        ->  c'_v: there is nothing to push against
//   otherwise                      ->  fl(fl(s c'_v) + fl(t u'_v)), contraction off
// rounded to the dtype to nearest even and clamped to the dtype's finite range (logit_shape.hip's ls_round rule).  A pair with
// a NaN or +inf element in either row, without a finite element in either row, or whose f32 sums leave f32's range (f32 /
// bf16 logits with |x| log2 e beyond it) is left as it is.  Unconditional rows are never written.
//
// GEOMETRY.  logit_shape.hip's: one workgroup of 1024 lanes per (b, j); lane t owns the 16-byte vectors t, t + 1024, ... of
// the CONDITIONAL row's aligned body, wave 0's lanes the up to 7 scalar elements in front of and behind it.  The unconditional
// row is cut at the SAME element indices, so a lane folds the same elements in the same order whatever the two rows' 16-byte
// phases are: equal data give equal bits at any pair of phases.  Its vectors are fetched by the widest load its address
// allows: a 16-byte buffer load needs a dword-aligned address only, so a body at a multiple of 4 bytes takes one load per
// vector; a 16-bit body at 2 mod 4 takes the 16 bytes from 2 bytes below and the dword behind them, and funnel-shifts the five
// dwords by 16 bits (both are aligned dwords that hold an element of the row; the descriptor ends behind the last of them).
// SWEEP 1 (the rows' one trip to HBM).  RESIDENT kernel (rows of at most ASD_CFG_RESIDENT_VECTORS = 19 * 1024 vectors): a
// lane's conditional vectors go into 19 x 4 registers in their packed form, all loads in flight at once; the unconditional
// vectors stream past four at a time behind them.  Two online (max, sum) pairs by the recurrences of lse_device.hpp.  Lanes
// merge by the fixed DPP sequence, the sixteen waves in wave order out of LDS by wave 0, which forms Lc and Lu once (f64, the
// split logarithm) and hands them to the others: two barriers per row.
// SWEEP 2.  The unconditional row again, four vectors per lane in flight -- hot in L2, one workgroup's row is 300 KB -- each
// combined with the held conditional vector, repacked into four registers and stored: every row leaves HBM once, the
// conditional row is written once.  76 held registers, 16 + 4 of an unconditional batch, 8 + 8 + 4 of one vector pair at a
// time: under the 128 a lane of a 1024-lane workgroup has.  Longer rows take the STREAMING kernel, which re-reads both.
// No workspace, no hand-off between workgroups: a row's result depends on the bytes of its pair and its record.

#include <hip/hip_runtime.h>

#include <float.h>

#include "lse_device.hpp"
#include "sample_device.hpp"

namespace asd {
namespace {

constexpr int kCfgThreads = 1024;
constexpr int kCfgWaves = kCfgThreads / 64;
constexpr int kCfgResVec = ASD_CFG_RESIDENT_VECTORS / kCfgThreads;   // 16-byte vectors a lane keeps: 76 dwords
constexpr int kCfgUnroll = 4;                                        // unconditional (streaming: and conditional) loads in flight
constexpr uint32_t kCfgStride = kCfgThreads * 16u;                   // bytes between two vectors of one lane
static_assert(kCfgResVec == 19 && kCfgResVec * kCfgThreads == ASD_CFG_RESIDENT_VECTORS, "the register budget is written for 19");

struct CfgRec {
    float scale;
    int32_t uncond_seq;
};
static_assert(sizeof(CfgRec) == ASD_CFG_REC_BYTES, "CfgRec");

// written once per row by lane 0 of each wave; go / lc / lu once by wave 0: two barriers per row
struct CfgLds {
    float m2c[kCfgWaves], sc[kCfgWaves], m2u[kCfgWaves], su[kCfgWaves];
    int go;
    float lc, lu;
};

// a row pair as the sweeps walk it: `head` scalar elements up to the conditional row's first 16-byte boundary, nvec vectors,
// `tail` scalar elements; the unconditional row at the same element indices
struct CfgPair {
    char* crow;
    const char* urow;
    char* cbody;
    __amdgpu_buffer_rsrc_t crsrc, ursrc;             // cbody .. + nvec*16; the unconditional body (odd: from 2 bytes below, + 4)
    uint32_t end;                                    // nvec * 16
    int head, nvec, tail;
    bool odd;                                        // the unconditional body lies at 2 mod 4 (uniform)
};

// an f32 result -> the dtype's bits (the low 16 for bf16 / f16): logit_shape.hip's ls_round, operation for operation
template <int DT>
__device__ __forceinline__ uint32_t cfg_round(float y) {
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

// kCfgUnroll unconditional vectors of this lane from byte offset `base` of the body on; a vector at or behind `end` reads as
// zeros without a memory access.  All loads are issued before the first shift.
__device__ __forceinline__ void cfg_load_u(const CfgPair& p, uint32_t base, u32x4 (&v)[kCfgUnroll]) {
    uint32_t x[kCfgUnroll];
#pragma unroll
    for (int i = 0; i < kCfgUnroll; ++i) v[i] = load16<false>(p.ursrc, base + static_cast<uint32_t>(i) * kCfgStride);
    if (!p.odd) return;
#pragma unroll
    for (int i = 0; i < kCfgUnroll; ++i)
        x[i] = __builtin_amdgcn_raw_buffer_load_b32(p.ursrc, base + static_cast<uint32_t>(i) * kCfgStride + 16u, 0, 0);
#pragma unroll
    for (int i = 0; i < kCfgUnroll; ++i) {
        const u32x4 w = v[i];
        v[i][0] = (w[0] >> 16) | (w[1] << 16);
        v[i][1] = (w[1] >> 16) | (w[2] << 16);
        v[i][2] = (w[2] >> 16) | (w[3] << 16);
        v[i][3] = (w[3] >> 16) | (x[i] << 16);
    }
}

// the guided element from the two stored values; `old`: the conditional element's bits
template <int DT>
__device__ __forceinline__ uint32_t cfg_elem(float xc, float xu, uint32_t old, float s, float t, float lc, float lu) {
    const float cp = xc - lc;
    const float up = xu - lu;
    const float y = xu > -INFINITY ? s * cp + t * up : cp;
    return xc > -INFINITY ? cfg_round<DT>(y) : old;
}

// one vector pair -> the conditional vector's new 16 bytes
template <int DT>
__device__ __forceinline__ u32x4 cfg_vec(const u32x4& vc, const u32x4& vu, float s, float t, float lc, float lu) {
    constexpr int N = Elem<DT>::kPerVec;
    float xc[N], xu[N];
    unpack<DT>(vc, xc);
    unpack<DT>(vu, xu);
    u32x4 w;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (N == 8) {
            const uint32_t lo = cfg_elem<DT>(xc[2 * i], xu[2 * i], vc[i] & 0xFFFFu, s, t, lc, lu);
            const uint32_t hi = cfg_elem<DT>(xc[2 * i + 1], xu[2 * i + 1], vc[i] >> 16, s, t, lc, lu);
            w[i] = lo | (hi << 16);
        } else {
            w[i] = cfg_elem<DT>(xc[i], xu[i], vc[i], s, t, lc, lu);
        }
    }
    return w;
}

template <int DT, bool kResident>
__global__ __launch_bounds__(kCfgThreads) void k_cfg_rows(void* cond, int64_t ld_seq, int64_t ld_row, const void* uncond,
                                                          int64_t ld_useq, int64_t ld_urow, int K1, int V, int Bu,
                                                          const CfgRec* __restrict__ table) {
    using E = Elem<DT>;
    constexpr int N = E::kPerVec;
    __shared__ CfgLds sh;

    const int tid = static_cast<int>(threadIdx.x);
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int row = static_cast<int>(blockIdx.x);
    const int b = static_cast<int>(static_cast<uint32_t>(row) / static_cast<uint32_t>(K1));
    const int j = row - b * K1;
    const float s = table[b].scale;                                                  // (uniform: scalar loads)
    const int q = table[b].uncond_seq;
    if (q < 0 || s == 1.0f) return;                                                  // off
    if (!(s >= 0.0f && s <= ASD_MAX_GUIDANCE_SCALE) || q >= Bu) return;                             // damaged, skipped
    const float t = 1.0f - s;

    CfgPair p;
    p.crow = static_cast<char*>(cond) + (static_cast<int64_t>(b) * ld_seq + static_cast<int64_t>(j) * ld_row) * E::kBytes;
    p.urow = static_cast<const char*>(uncond) + (static_cast<int64_t>(q) * ld_useq + static_cast<int64_t>(j) * ld_urow) * E::kBytes;
    const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p.crow) & 15u);      // (a multiple of the element size)
    p.head = mis ? static_cast<int>((16u - mis) / E::kBytes) : 0;
    if (p.head > V) p.head = V;
    p.nvec = (V - p.head) / N;                                                       // resident: <= V / N <= kCfgResVec * 1024
    p.tail = V - p.head - p.nvec * N;
    p.cbody = p.crow + static_cast<int64_t>(p.head) * E::kBytes;
    p.end = static_cast<uint32_t>(p.nvec) * 16u;                                     // launcher: V * element size < 2^31
    const char* ubody = p.urow + static_cast<int64_t>(p.head) * E::kBytes;
    p.odd = (reinterpret_cast<uintptr_t>(ubody) & 2u) != 0;                          // (16-bit only)
    p.crsrc = __builtin_amdgcn_make_buffer_rsrc(p.cbody, 0, static_cast<int>(p.end), 0x00020000);
    // odd: the descriptor starts at the aligned dword that holds the body's first element and ends behind the one that holds
    // its last; an empty body gets an empty descriptor
    p.ursrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(ubody) - (p.odd ? 2 : 0), 0,
                                                static_cast<int>(p.end + (p.odd && p.nvec ? 4u : 0u)), 0x00020000);
    const uint32_t off0 = static_cast<uint32_t>(tid) * 16u;
    u32x4 res[kCfgResVec];                                                           // (the streaming kernel never touches it)

    // ---- sweep 1: (m2, s) of both rows at temperature 1; a NaN or +inf element makes its row's sum NaN
    float m2c = kSentinel, sc = 0.0f, m2u = kSentinel, su = 0.0f;
    if (tid < p.head) {
        accum_scalar(E::scalar(p.crow, tid), kLog2e, m2c, sc);
        accum_scalar(E::scalar(p.urow, tid), kLog2e, m2u, su);
    }
    if constexpr (kResident) {
#pragma unroll
        for (int i = 0; i < kCfgResVec; ++i) res[i] = load16<false>(p.crsrc, off0 + static_cast<uint32_t>(i) * kCfgStride);
#pragma unroll
        for (int i0 = 0; i0 < kCfgResVec; i0 += kCfgUnroll) {
            const uint32_t base = off0 + static_cast<uint32_t>(i0) * kCfgStride;
            if (base >= p.end) break;                                                // (a lane's offsets ascend)
            u32x4 vu[kCfgUnroll];
            cfg_load_u(p, base, vu);
#pragma unroll
            for (int i = 0; i < kCfgUnroll; ++i)
                if (base + static_cast<uint32_t>(i) * kCfgStride < p.end) E::accum(vu[i], kLog2e, m2u, su);
        }
#pragma unroll
        for (int i = 0; i < kCfgResVec; ++i)
            if (off0 + static_cast<uint32_t>(i) * kCfgStride < p.end) E::accum(res[i], kLog2e, m2c, sc);
    } else {
        for (uint32_t base = off0; base < p.end; base += kCfgUnroll * kCfgStride) {
            u32x4 vc[kCfgUnroll], vu[kCfgUnroll];
#pragma unroll
            for (int i = 0; i < kCfgUnroll; ++i) vc[i] = load16<false>(p.crsrc, base + static_cast<uint32_t>(i) * kCfgStride);
            cfg_load_u(p, base, vu);
#pragma unroll
            for (int i = 0; i < kCfgUnroll; ++i)
                if (base + static_cast<uint32_t>(i) * kCfgStride < p.end) {
                    E::accum(vc[i], kLog2e, m2c, sc);
                    E::accum(vu[i], kLog2e, m2u, su);
                }
        }
    }
    if (tid < p.tail) {
        const int id = p.head + p.nvec * N + tid;
        accum_scalar(E::scalar(p.crow, id), kLog2e, m2c, sc);
        accum_scalar(E::scalar(p.urow, id), kLog2e, m2u, su);
    }
    wave_merge(m2c, sc);
    wave_merge(m2u, su);
    if (lane == 0) {
        sh.m2c[wave] = m2c;
        sh.sc[wave] = sc;
        sh.m2u[wave] = m2u;
        sh.su[wave] = su;
    }
    __syncthreads();
    // ---- wave 0 alone merges the sixteen partials in wave order and forms the two log-sum-exps ONCE (f64, the split logarithm)
    if (wave == 0) {
        float rm2c = kSentinel, rsc = 0.0f, rm2u = kSentinel, rsu = 0.0f;
#pragma unroll 1
        for (int w = 0; w < kCfgWaves; ++w) {
            ms_merge(rm2c, rsc, sh.m2c[w], sh.sc[w]);
            ms_merge(rm2u, rsu, sh.m2u[w], sh.su[w]);
        }
        // a sum of 0: no finite element; NaN: a NaN or +inf element, or |x| log2 e beyond f32's range -- the pair stays
        const bool go = rsc > 0.0f && rsc < INFINITY && rsu > 0.0f && rsu < INFINITY;
        if (lane == 0) {
            sh.go = go ? 1 : 0;
            sh.lc = static_cast<float>(kLn2d * (static_cast<double>(rm2c) + log2_split(rsc)));
            sh.lu = static_cast<float>(kLn2d * (static_cast<double>(rm2u) + log2_split(rsu)));
        }
    }
    __syncthreads();
    if (sh.go == 0) return;                                                          // (block-uniform)
    const float lc = sh.lc;
    const float lu = sh.lu;

    // ---- sweep 2: the unconditional row again (L2), combined with the conditional vectors, stored
    auto one = [&](int id) {
        const uint32_t old = E::raw(p.crow, id);
        const uint32_t now = cfg_elem<DT>(E::from_raw(old), E::scalar(p.urow, id), old, s, t, lc, lu);
        if constexpr (DT == ASD_DTYPE_F32) reinterpret_cast<uint32_t*>(p.crow)[id] = now;
        else reinterpret_cast<uint16_t*>(p.crow)[id] = static_cast<uint16_t>(now);
    };
    if (tid < p.head) one(tid);
    if constexpr (kResident) {
#pragma unroll
        for (int i0 = 0; i0 < kCfgResVec; i0 += kCfgUnroll) {
            const uint32_t base = off0 + static_cast<uint32_t>(i0) * kCfgStride;
            if (base >= p.end) break;
            u32x4 vu[kCfgUnroll];
            cfg_load_u(p, base, vu);
#pragma unroll
            for (int i = 0; i < kCfgUnroll; ++i) {
                const uint32_t off = base + static_cast<uint32_t>(i) * kCfgStride;
                if (i0 + i < kCfgResVec && off < p.end)
                    *reinterpret_cast<u32x4*>(p.cbody + off) = cfg_vec<DT>(res[i0 + i < kCfgResVec ? i0 + i : 0], vu[i], s, t, lc, lu);
            }
        }
    } else {
        for (uint32_t base = off0; base < p.end; base += kCfgUnroll * kCfgStride) {
            u32x4 vc[kCfgUnroll], vu[kCfgUnroll];
#pragma unroll
            for (int i = 0; i < kCfgUnroll; ++i) vc[i] = load16<false>(p.crsrc, base + static_cast<uint32_t>(i) * kCfgStride);
            cfg_load_u(p, base, vu);
#pragma unroll
            for (int i = 0; i < kCfgUnroll; ++i) {
                const uint32_t off = base + static_cast<uint32_t>(i) * kCfgStride;
                if (off < p.end) *reinterpret_cast<u32x4*>(p.cbody + off) = cfg_vec<DT>(vc[i], vu[i], s, t, lc, lu);
            }
        }
    }
    if (tid < p.tail) one(p.head + p.nvec * N + tid);
}

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT int asd_cfg_rows(void* cond, int dtype, int B, int K1, int V, int64_t ld_seq, int64_t ld_row, const void* uncond,
                            int Bu, int64_t ld_useq, int64_t ld_urow, const asd_cfg_rec* table, void* stream) {
    if (B < 0 || K1 < 0 || V < 0 || Bu < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0 || K1 == 0 || V == 0) return ASD_OK;
    const int esz = dtype_size(dtype);
    if (esz == 0) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(B) * K1 > INT32_MAX) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(V) * esz > INT32_MAX - 16) return ASD_ERR_UNSUPPORTED;  // the sweeps count bytes in 32 bits
    if (!cond || !table || (Bu > 0 && !uncond)) return ASD_ERR_INVALID_ARG;
    if (ld_row < V || ld_seq < static_cast<int64_t>(K1) * ld_row) return ASD_ERR_INVALID_ARG;
    if (Bu > 0 && (ld_urow < V || ld_useq < static_cast<int64_t>(K1) * ld_urow)) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(cond, static_cast<size_t>(esz)) || !aligned_to(uncond, static_cast<size_t>(esz)) || !aligned_to(table, 4))
        return ASD_ERR_ALIGNMENT;
    const dim3 grid(static_cast<uint32_t>(static_cast<int64_t>(B) * K1));
    const bool resident = V <= ASD_CFG_RESIDENT_VECTORS * (16 / esz);                // every row's nvec <= V / N
    dispatch_dtype(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (resident)
            hipLaunchKernelGGL((k_cfg_rows<DT, true>), grid, dim3(kCfgThreads), 0, static_cast<hipStream_t>(stream), cond, ld_seq,
                               ld_row, uncond, ld_useq, ld_urow, K1, V, Bu, reinterpret_cast<const CfgRec*>(table));
        else
            hipLaunchKernelGGL((k_cfg_rows<DT, false>), grid, dim3(kCfgThreads), 0, static_cast<hipStream_t>(stream), cond, ld_seq,
                               ld_row, uncond, ld_useq, ld_urow, K1, V, Bu, reinterpret_cast<const CfgRec*>(table));
    });
    return launch_status();
}
