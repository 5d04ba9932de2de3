// linear_fp8.hip -- weight-only FP8 (W8A16) projections: OCP E4M3 codes with one f32 scale per output row,
// bf16 / f16 activations, f32 accumulation, one rounding.
//
//   y[m][n] = round( scale[n] * sum_d x[m][d] * code[n][d]  + bias[n] + residual[m][n] )
//
// Every model pass is bound by the bytes of its projection weights; this moves half of them.  E4M3 -> bf16 / f16
// is exact, so the product is asd_linear's arithmetic on a different, exactly known matrix, plus ONE f32 multiply per output.
//
// The image (asd_fp8_quantize_weights writes it, asd_linear_fp8 streams it; N % 256 == 0, D % 64 == 0):
//
//   codes  [N / 256 column blocks][D / 64 superstages][8 waves][2 quarters q][64 lanes][16 bytes]     N * D bytes
//   scales [N] f32                                                                                    at byte N * D
//
// A superstage -- 256 weight rows x 64 reduction columns -- is ONE contiguous 16 KiB run, and inside it the bytes lie in the
// order the kernel's LDS reads want them: wave w owns weight rows 32 w .. 32 w + 31 of the block, lane (r = lane & 31,
// h = lane >> 5) of that wave owns the 32 codes of row r at reduction columns 32 h .. 32 h + 31, and quarter q holds its 16
// codes at columns 32 h + 16 q .. + 15.  So code (n, d) sits at
//
//   ((n / 256) * (D / 64) + d / 64) * 16384 + ((n % 256) / 32) * 2048 + ((d % 32) / 16) * 1024
//       + (((d % 64) / 32) * 32 + n % 32) * 16 + d % 16.
//
// The LDS-DMA copies the run verbatim (a wave moves exactly the 2 KiB it will read itself), and a fragment read is one
// ds_read_b128 at  slot + 2048 w + 1024 q + 16 lane : consecutive lanes, consecutive 16-byte words, no bank conflict and no
// swizzle.  One 16-byte read is the A operand of TWO 32 x 32 x 16 MFMA steps (k-step ks = 2 q + e / 8 covers reduction columns
// 32 h + 8 ks .. + 7 -- the k-slot map of the bf16 kernels, so the activations keep their swizzled 128-byte-row LDS image).
//
// k_linear_fp8<F16, MT>: 8 waves side by side on the 256 columns of a block, MT 32-row accumulator tiles each (MT = 1 for
// M <= 32, else 2: row blocks of 64).  Rings, in superstages:  MT = 2: 7 weight slots (112 KiB) + 6 activation slots (48 KiB);
// MT = 1: 8 weight slots (128 KiB) + 7 activation slots of 32 rows (28 KiB).  Behind the barrier that opens superstage S the
// waves issue  X(S + RH - 1), W(S + RW - 1)  (RW = RH + 1); a wave's vmcnt retires in order, so waiting for X(S) leaves
// W(S + 1) .. W(S + RH - 1) in flight: five (MT = 2) or six (MT = 1) weight superstages, 80 / 96 KiB per CU, stay outstanding
// at every barrier -- the bf16 kernel holds 64 KiB, which is the same DEPTH in 32 KiB superstages halved.
//
// Epilogue: a lane's 16 accumulator entries are 16 weight rows n of ONE activation row m, so the row scale is a per-lane
// vector: acc *= scale[n] (one f32 multiply, compiled without contraction), then bias, then residual, one rounding.  A reduction
// slice writes its SCALED f32 partials to [slice][M][N]; k_linear_fp8_reduce (or the decoder's slab consumers) add them in
// slice order, so the same bits result on every call.
#include "common.hpp"

namespace asd {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void glb_void;

constexpr int kThreads = 512;
constexpr int kBN = 256;            // weight rows (output columns) per workgroup
constexpr int kSuper = 64;          // reduction columns per superstage
constexpr int kWSlot = kBN * kSuper;   // 16 KiB of codes
constexpr int kRowBlock = 64;       // activation rows per workgroup
constexpr float kE4M3Max = 448.0f;

struct Fp8Params {
    const void* x;
    int64_t ld_x;
    const unsigned char* codes;
    const float* scale;
    int D, M, N;
    int m_blocks;        // row blocks of 64 (1 for M <= 64)
    int k_slices;
    float* slabs;        // [k_slices][M][N] scaled partials (k_slices > 1)
    void* out;
    int64_t ld_out;
    const void* bias;
    const void* residual;
    int64_t ld_res;
};

// ---- element helpers (the STORE epilogue's, as in lm_head_verify.hip)
template <bool F16>
__device__ __forceinline__ uint32_t pack_pair(float a, float b) {
    if constexpr (F16) {
        const _Float16 x = static_cast<_Float16>(a), y = static_cast<_Float16>(b);
        return static_cast<uint32_t>(__builtin_bit_cast(uint16_t, x)) | (static_cast<uint32_t>(__builtin_bit_cast(uint16_t, y)) << 16);
    } else {
        const __bf16 x = static_cast<__bf16>(a), y = static_cast<__bf16>(b);
        return static_cast<uint32_t>(__builtin_bit_cast(uint16_t, x)) | (static_cast<uint32_t>(__builtin_bit_cast(uint16_t, y)) << 16);
    }
}
template <bool F16>
__device__ __forceinline__ float unpack_elem(uint32_t w, int hi) {
    const uint16_t u = static_cast<uint16_t>(hi ? (w >> 16) : (w & 0xffffu));
    if constexpr (F16) return static_cast<float>(__builtin_bit_cast(_Float16, u));
    else return __uint_as_float(static_cast<uint32_t>(u) << 16);
}

// 8 E4M3 codes (two dwords) -> one MFMA operand register group; exact (v_cvt_scalef32_pk_{bf16,f16}_fp8, scale 1)
template <bool F16>
__device__ __forceinline__ bf16x8 widen8(uint32_t lo, uint32_t hi) {
    uint32_t o[4];
    if constexpr (F16) {
        o[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, false));
        o[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, true));
        o[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, false));
        o[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, true));
    } else {
        o[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false));
        o[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true));
        o[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false));
        o[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true));
    }
    u32x4 v = {o[0], o[1], o[2], o[3]};
    return __builtin_bit_cast(bf16x8, v);
}
template <bool F16>
__device__ __forceinline__ f32x16 mfma32(const bf16x8& a, const bf16x8& b, const f32x16& c) {
    if constexpr (F16)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

template <int PENDING>
__device__ __forceinline__ void wait_and_meet() {
    // lgkmcnt(0): the fragments this wave read from the slots about to be refilled have arrived
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(PENDING) : "memory");
}

// lane (r, h) of wave wv holds, per 32 x 32 tile, output columns n_first + 8 q + e (q, e = 0..3) of ONE row m
template <bool F16>
__device__ __forceinline__ void store_tile(const f32x16& a, int m, int n_first, int slice, const Fp8Params& p) {
    if (m >= p.M) return;
    f32x4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 sc = *reinterpret_cast<const f32x4*>(p.scale + n_first + 8 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[q][e] = a[4 * q + e] * sc[e];
    }
    if (p.k_slices > 1) {
        float* const row = p.slabs + (static_cast<int64_t>(slice) * p.M + m) * p.N;
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4*>(row + n_first + 8 * q) = v[q];
        return;
    }
    char* const row = static_cast<char*>(p.out) + static_cast<int64_t>(m) * p.ld_out * 2;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int n = n_first + 8 * q;
        if (p.bias) {
            const uint2 bw = *reinterpret_cast<const uint2*>(static_cast<const char*>(p.bias) + static_cast<int64_t>(n) * 2);
            v[q][0] += unpack_elem<F16>(bw.x, 0); v[q][1] += unpack_elem<F16>(bw.x, 1);
            v[q][2] += unpack_elem<F16>(bw.y, 0); v[q][3] += unpack_elem<F16>(bw.y, 1);
        }
        if (p.residual) {
            const uint2 rw = *reinterpret_cast<const uint2*>(static_cast<const char*>(p.residual) +
                                                             (static_cast<int64_t>(m) * p.ld_res + n) * 2);
            v[q][0] += unpack_elem<F16>(rw.x, 0); v[q][1] += unpack_elem<F16>(rw.x, 1);
            v[q][2] += unpack_elem<F16>(rw.y, 0); v[q][3] += unpack_elem<F16>(rw.y, 1);
        }
        uint2 o;
        o.x = pack_pair<F16>(v[q][0], v[q][1]);
        o.y = pack_pair<F16>(v[q][2], v[q][3]);
        *reinterpret_cast<uint2*>(row + static_cast<int64_t>(n) * 2) = o;
    }
}

template <bool F16, int MT>
__global__ __launch_bounds__(kThreads, 1) void k_linear_fp8(Fp8Params p) {
    constexpr int RH = MT == 1 ? 7 : 6;          // activation slots
    constexpr int RW = RH + 1;                   // weight slots
    constexpr int kXSlot = MT * 32 * 128;        // MT * 32 rows of 64 bf16
    constexpr int XWAVES = MT * 4;               // waves that move activations (1 KiB = 8 rows each)
    constexpr int WI = 2, XI = 1;                // DMA instructions per wave and superstage
    __shared__ __attribute__((aligned(1024))) unsigned char lds[RW * kWSlot + RH * kXSlot];
    unsigned char* const lds_x = lds + RW * kWSlot;
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wv = t >> 6;
    const int wv_s = __builtin_amdgcn_readfirstlane(wv);
    const int r = lane & 31;
    const int h = lane >> 5;
    // grid: column block, row block, reduction slice (slices of a block are neighbours, then its row blocks: one L2 footprint)
    const int slice = static_cast<int>(blockIdx.x) % p.k_slices;
    const int unit = static_cast<int>(blockIdx.x) / p.k_slices;
    const int mb = unit % p.m_blocks;
    const int nb = unit / p.m_blocks;
    const int n0 = nb * kBN;
    const int m0 = mb * kRowBlock;
    const int rows_x = min(MT * 32, p.M - m0);

    const int total_super = p.D / kSuper;
    const int s_begin = static_cast<int>(static_cast<int64_t>(slice) * total_super / p.k_slices);
    const int n_super = static_cast<int>(static_cast<int64_t>(slice + 1) * total_super / p.k_slices);
    const unsigned char* const wbase = p.codes + static_cast<int64_t>(nb) * total_super * kWSlot + wv * 2048 + lane * 16;
    const bool moves_x = wv_s < XWAVES;
    const int drow = wv * 8 + (lane >> 3);       // activation row this lane moves (waves < XWAVES)
    const char* const xbase = static_cast<const char*>(p.x) +
        (static_cast<int64_t>(m0) + min(drow, rows_x - 1)) * p.ld_x * 2 + (((lane & 7) ^ ((drow >> 1) & 7)) * 16);
    auto issue_w = [&](int stage) {
        const unsigned char* src = wbase + static_cast<int64_t>(stage) * kWSlot;
        unsigned char* dst = lds + (stage % RW) * kWSlot + wv_s * 2048;
        __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)dst, 16, 0, 2);
        __builtin_amdgcn_global_load_lds((glb_void*)(src + 1024), (lds_void*)(dst + 1024), 16, 0, 2);
    };
    auto issue_x = [&](int stage) {
        if (!moves_x) return;
        const char* src = xbase + static_cast<int64_t>(stage) * (kSuper * 2);
        unsigned char* dst = lds_x + (stage % RH) * kXSlot + wv_s * 1024;
        __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)dst, 16, 0, 0);
    };

    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[mt][i] = 0.0f;
    const int key = (r >> 1) & 7;
    auto compute = [&](int S) {
        const unsigned char* wb = lds + (S % RW) * kWSlot + wv * 2048 + lane * 16;
        const unsigned char* xb = lds_x + (S % RH) * kXSlot + r * 128;
        const u32x4 c0 = *reinterpret_cast<const u32x4*>(wb);
        const u32x4 c1 = *reinterpret_cast<const u32x4*>(wb + 1024);
        bf16x8 xf[4][MT];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                xf[ks][mt] = *reinterpret_cast<const bf16x8*>(xb + mt * 32 * 128 + (((4 * h + ks) ^ key) * 16));
        const bf16x8 wf[4] = {widen8<F16>(c0[0], c0[1]), widen8<F16>(c0[2], c0[3]), widen8<F16>(c1[0], c1[1]), widen8<F16>(c1[2], c1[3])};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma32<F16>(wf[ks], xf[ks][mt], acc[mt]);
    };
    // prologue in steady-state order: W(0) | X(0) W(1) | ... | X(RH - 2) W(RH - 1)
    int S = s_begin;
    if (S < n_super) issue_w(S);
#pragma unroll
    for (int j = 0; j + 1 < RH; ++j) {
        if (S + j < n_super) issue_x(S + j);
        if (S + j + 1 < n_super) issue_w(S + j + 1);
    }
    // steady state: behind X(S) a wave that moves activations has issued W(S + 1) and RH - 2 pairs; one that does not has
    // issued W(S + 1) .. W(S + RW - 2) behind its W(S)
    for (; S + RW - 1 < n_super; ++S) {
        if (moves_x) wait_and_meet<WI + (RH - 2) * (XI + WI)>();
        else wait_and_meet<(RW - 2) * WI>();
        issue_x(S + RH - 1);
        issue_w(S + RW - 1);
        compute(S);
    }
    for (; S < n_super; ++S) {                   // the last RW - 1 superstages: every load is issued, drain
        wait_and_meet<0>();
        if (S + RH - 1 < n_super) issue_x(S + RH - 1);
        compute(S);
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) store_tile<F16>(acc[mt], m0 + 32 * mt + r, n0 + 32 * wv + 4 * h, slice, p);
}

// the scaled partials of a sliced launch -> y: thread = 4 consecutive columns of one row; slices added in slice order, then
// bias, then residual, one rounding (the order of asd_linear_ex's reduce kernel and of the decoder's slab consumers)
template <bool F16>
__global__ __launch_bounds__(256) void k_linear_fp8_reduce(const float* __restrict__ slabs, int k_slices, int M, int N,
                                                           const void* __restrict__ bias, const void* residual, int64_t ld_res,
                                                           void* out, int64_t ld_out) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int n4 = N / 4;
    if (i >= static_cast<int64_t>(M) * n4) return;
    const int m = static_cast<int>(i / n4), n = static_cast<int>(i % n4) * 4;
    const float* src = slabs + static_cast<int64_t>(m) * N + n;
    const int64_t stride = static_cast<int64_t>(M) * N;
    f32x4 acc = *reinterpret_cast<const f32x4*>(src);
    for (int sl = 1; sl < k_slices; ++sl) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + sl * stride);
        acc[0] += v[0]; acc[1] += v[1]; acc[2] += v[2]; acc[3] += v[3];
    }
    if (bias) {
        const uint2 bw = *reinterpret_cast<const uint2*>(static_cast<const char*>(bias) + static_cast<int64_t>(n) * 2);
        acc[0] += unpack_elem<F16>(bw.x, 0); acc[1] += unpack_elem<F16>(bw.x, 1);
        acc[2] += unpack_elem<F16>(bw.y, 0); acc[3] += unpack_elem<F16>(bw.y, 1);
    }
    if (residual) {
        const uint2 rw = *reinterpret_cast<const uint2*>(static_cast<const char*>(residual) + (static_cast<int64_t>(m) * ld_res + n) * 2);
        acc[0] += unpack_elem<F16>(rw.x, 0); acc[1] += unpack_elem<F16>(rw.x, 1);
        acc[2] += unpack_elem<F16>(rw.y, 0); acc[3] += unpack_elem<F16>(rw.y, 1);
    }
    uint2 o;
    o.x = pack_pair<F16>(acc[0], acc[1]);
    o.y = pack_pair<F16>(acc[2], acc[3]);
    *reinterpret_cast<uint2*>(static_cast<char*>(out) + (static_cast<int64_t>(m) * ld_out + n) * 2) = o;
}

// ---- the quantiser.  f32 -> E4M3 (OCP "fn": bias 7, no infinities, 0x7f / 0xff = NaN), round to nearest even, for a finite
// |v| <= 448 (the caller clamps): integer arithmetic, so that its bits can be stated and checked anywhere.
__device__ __forceinline__ uint32_t e4m3_rne(float v) {
    const uint32_t u = __float_as_uint(v);
    const uint32_t sign = (u >> 24) & 0x80u;
    const uint32_t a = u & 0x7fffffffu;
    uint32_t code;
    if (a >= (121u << 23)) {                         // |v| >= 2^-6: normal; keep 3 mantissa bits, ties to even
        const uint32_t rounded = a + 0x7ffffu + ((a >> 20) & 1u);
        code = (rounded >> 20) - (120u << 3);        // rebias 127 -> 7; a carry out of the mantissa raises the exponent
    } else {                                         // subnormal: multiples of 2^-9 (8 * 2^-9 = 2^-6 carries into the normals)
        code = static_cast<uint32_t>(rintf(__uint_as_float(a) * 512.0f));
    }
    return sign | code;
}

// One workgroup of 256 threads per 32 weight rows (the rows of one wave of the product kernel), 8 threads per row, two
// sweeps: abs-max, then convert.  A thread converts 16 consecutive columns per step and writes them as ONE 16-byte piece of
// the image; the 32 rows' pieces of one (superstage, h, q) are 512 contiguous bytes.
template <bool F16>
__global__ __launch_bounds__(256) void k_fp8_quantize(const char* __restrict__ w, int64_t ld_w, int N, int D,
                                                      unsigned char* __restrict__ codes, float* __restrict__ scale) {
    const int t = threadIdx.x;
    const int r = t >> 3, sub = t & 7;
    const int64_t n = static_cast<int64_t>(blockIdx.x) * 32 + r;
    const char* const row = w + n * ld_w * 2;
    const int pieces = D / 16;
    float amax = 0.0f;
    for (int pc = sub; pc < pieces; pc += 8) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(row + pc * 32 + half * 16);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                amax = fmaxf(amax, fabsf(unpack_elem<F16>(v[i], 0)));
                amax = fmaxf(amax, fabsf(unpack_elem<F16>(v[i], 1)));
            }
        }
    }
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 4, 64));
    const float sc = amax > 0.0f ? __fdiv_rn(amax, kE4M3Max) : 1.0f;
    if (sub == 0) scale[n] = sc;
    const int n_super = D / kSuper;
    unsigned char* const blk = codes + (n >> 8) * n_super * kWSlot + ((n & 255) >> 5) * 2048 + (n & 31) * 16;
    for (int pc = sub; pc < pieces; pc += 8) {
        uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(row + pc * 32 + half * 16);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    float q = __fdiv_rn(unpack_elem<F16>(v[i], e), sc);
                    q = fminf(fmaxf(q, -kE4M3Max), kE4M3Max);          // saturate; a NaN weight becomes -448, never a NaN code
                    const int k = half * 8 + i * 2 + e;                // column within the piece
                    o[k >> 2] |= e4m3_rne(q) << (8 * (k & 3));
                }
        }
        const int s = pc >> 2, hh = (pc >> 1) & 1, q = pc & 1;         // columns 16 pc ..: superstage, half, quarter
        const u32x4 ov = {o[0], o[1], o[2], o[3]};
        *reinterpret_cast<u32x4*>(blk + static_cast<int64_t>(s) * kWSlot + q * 1024 + hh * 512) = ov;
    }
}

// Reduction slices.  Costs in superstage-times of one CU (16 KiB of codes).  A workgroup pays its share of the reduction, the
// ring's fill (RW - 1 superstages are requested before the first is multiplied) and, when sliced, the slab round trip: rows x
// 256 columns x 4 B written and read again = rows / 8 superstages' worth of bytes, a quarter of that while the partials stay
// in the MALL (DESIGN §4.9 measured this for the bf16 slabs; the bytes are the same here, the unit is half as large).  Whoever
// adds the partials walks the slices one after the other: 0.45 us per slice (§4.9) = 1.5 of these superstage-times.  The
// kernel is HBM-bound, so a partial last round shares the bandwidth the idle CUs leave: only fill and slabs count per round.
struct Fp8Plan {
    int k_slices;
    int m_blocks;
    int64_t units;       // workgroups before slicing
};
Fp8Plan fp8_plan(int M, int N, int D) {
    Fp8Plan pl{};
    pl.m_blocks = (M + kRowBlock - 1) / kRowBlock;
    pl.units = static_cast<int64_t>(N / kBN) * pl.m_blocks;
    pl.k_slices = 1;
    const int64_t cus = current_device_cus() > 0 ? current_device_cus() : 256;
    if (pl.units * 2 > cus) return pl;           // more than half a round of workgroups: unsliced (§4.9: slicing measured level or worse)
    const int total = D / kSuper;
    const int rows = M < kRowBlock ? M : kRowBlock;
    const double fill = 6.0;
    const double slab = rows / 32.0 > 1.0 ? rows / 32.0 : 1.0;
    double best = -1.0;
    for (int sl = 1; sl <= 32 && sl <= total; ++sl) {
        const double wgs = static_cast<double>(pl.units) * sl;
        const double share = wgs > static_cast<double>(cus) ? wgs / static_cast<double>(cus) : 1.0;
        const double rounds = static_cast<double>((pl.units * sl + cus - 1) / cus);
        double cost = share * static_cast<double>((total + sl - 1) / sl) + rounds * (fill + (sl > 1 ? slab : 0.0));
        if (sl > 1) cost += 1.5 * sl;
        if (best < 0.0 || cost < best) { best = cost; pl.k_slices = sl; }
    }
    return pl;
}

bool fp8_shape_ok(int N, int D) { return N > 0 && D > 0 && N % kBN == 0 && D % kSuper == 0; }

}  // namespace

// k_slices_out != NULL: a sliced plan stops after the product (asd_linear_partial's contract): the SCALED f32 partials stay in
// `workspace` as [k_slices][M][N] and the caller's next kernel adds them, the bias and the residual.
int linear_fp8_run(const void* x, int64_t ld_x, const void* image, size_t image_bytes, const void* bias, const void* residual,
                   int64_t ld_res, int dtype, int M, int N, int D, void* y, int64_t ld_y, void* workspace,
                   size_t workspace_bytes, void* stream, int* k_slices_out) {
    if (k_slices_out) *k_slices_out = 1;
    if (M < 0 || N < 1 || D < 1) return ASD_ERR_INVALID_ARG;
    if (residual && (ld_res < N || ld_res % 4 != 0 || !aligned_to(residual, 8))) return ld_res < N ? ASD_ERR_INVALID_ARG : ASD_ERR_ALIGNMENT;
    if (M == 0) return ASD_OK;
    if ((dtype != ASD_DTYPE_BF16 && dtype != ASD_DTYPE_F16) || !fp8_shape_ok(N, D)) return ASD_ERR_UNSUPPORTED;
    if (!x || !image || !y || ld_x < D || ld_y < N || image_bytes < asd_fp8_image_bytes(N, D)) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(x, 16) || !aligned_to(image, 16) || !aligned_to(y, 8) || (bias && !aligned_to(bias, 8)) || ld_x % 8 != 0 || ld_y % 4 != 0)
        return ASD_ERR_ALIGNMENT;
    const Fp8Plan pl = fp8_plan(M, N, D);
    const size_t slab_bytes = pl.k_slices > 1 ? static_cast<size_t>(pl.k_slices) * M * static_cast<size_t>(N) * sizeof(float) : 0;
    if (slab_bytes > 0 && (!workspace || workspace_bytes < slab_bytes)) return ASD_ERR_WORKSPACE;
    if (slab_bytes > 0 && !aligned_to(workspace, 16)) return ASD_ERR_ALIGNMENT;
    if (pl.units * pl.k_slices >= (1ll << 31) || static_cast<int64_t>(M) * N / 4 / 256 >= (1ll << 31)) return ASD_ERR_UNSUPPORTED;

    Fp8Params p{};
    p.x = x; p.ld_x = ld_x;
    p.codes = static_cast<const unsigned char*>(image);
    p.scale = reinterpret_cast<const float*>(p.codes + static_cast<size_t>(N) * D);
    p.D = D; p.M = M; p.N = N;
    p.m_blocks = pl.m_blocks;
    p.k_slices = pl.k_slices;
    p.slabs = static_cast<float*>(workspace);
    p.out = y; p.ld_out = ld_y; p.bias = bias; p.residual = residual; p.ld_res = ld_res;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<unsigned>(pl.units * pl.k_slices));
    if (k_slices_out) *k_slices_out = pl.k_slices;
    dispatch_bool(dtype == ASD_DTYPE_F16, [&](auto f) {
        constexpr bool F16 = decltype(f)::value;
        if (M <= 32) hipLaunchKernelGGL((k_linear_fp8<F16, 1>), grid, dim3(kThreads), 0, st, p);
        else hipLaunchKernelGGL((k_linear_fp8<F16, 2>), grid, dim3(kThreads), 0, st, p);
        if (pl.k_slices > 1 && !k_slices_out) {
            const int64_t n_threads = static_cast<int64_t>(M) * (N / 4);
            hipLaunchKernelGGL(k_linear_fp8_reduce<F16>, dim3(static_cast<unsigned>((n_threads + 255) / 256)), dim3(256), 0, st,
                               p.slabs, pl.k_slices, M, N, bias, residual, ld_res, y, ld_y);
        }
    });
    return launch_status();
}

}  // namespace asd

using namespace asd;

ASD_EXPORT size_t asd_fp8_image_bytes(int N, int D) {
    if (!fp8_shape_ok(N, D)) return 0;
    return static_cast<size_t>(N) * D + static_cast<size_t>(N) * sizeof(float);
}

ASD_EXPORT int asd_fp8_quantize_weights(const void* weight, int64_t ld_w, int dtype, int N, int D, void* image, size_t image_bytes,
                                        void* stream) {
    if (N < 1 || D < 1) return ASD_ERR_INVALID_ARG;
    if ((dtype != ASD_DTYPE_BF16 && dtype != ASD_DTYPE_F16) || !fp8_shape_ok(N, D)) return ASD_ERR_UNSUPPORTED;
    if (!weight || !image || ld_w < D || image_bytes < asd_fp8_image_bytes(N, D)) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(weight, 16) || !aligned_to(image, 16) || ld_w % 8 != 0) return ASD_ERR_ALIGNMENT;
    unsigned char* const codes = static_cast<unsigned char*>(image);
    float* const scale = reinterpret_cast<float*>(codes + static_cast<size_t>(N) * D);
    dispatch_bool(dtype == ASD_DTYPE_F16, [&](auto f) {
        constexpr bool F16 = decltype(f)::value;
        hipLaunchKernelGGL(k_fp8_quantize<F16>, dim3(static_cast<unsigned>(N / 32)), dim3(256), 0, static_cast<hipStream_t>(stream),
                           static_cast<const char*>(weight), ld_w, N, D, codes, scale);
    });
    return launch_status();
}

ASD_EXPORT size_t asd_linear_fp8_workspace_bytes(int M, int N, int D) {
    if (M <= 0 || !fp8_shape_ok(N, D)) return 0;
    const Fp8Plan pl = fp8_plan(M, N, D);
    const size_t slabs = pl.k_slices > 1 ? static_cast<size_t>(pl.k_slices) * M * static_cast<size_t>(N) * sizeof(float) : 0;
    return round_up(slabs, 256) + 256;
}

ASD_EXPORT int asd_linear_fp8(const void* x, int64_t ld_x, const void* image, size_t image_bytes, const void* bias,
                              const void* residual, int64_t ld_res, int dtype, int M, int N, int D, void* y, int64_t ld_y,
                              void* workspace, size_t workspace_bytes, void* stream) {
    return linear_fp8_run(x, ld_x, image, image_bytes, bias, residual, ld_res, dtype, M, N, D, y, ld_y, workspace, workspace_bytes,
                          stream, nullptr);
}
