// philox.hip -- every uniform of a decoding step in one launch, keyed by the request's seed (SamplingParams(seed=...)), gfx950.
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 generator):
// a counter-based generator, so the draw of (seed, step, slot, stage) is a pure function of those four numbers -- no state is
// kept between launches and no row of a batch sees another row's draws.
//
//   key     = (seed_lo, seed_hi)           the request's 64-bit seed
//   counter = (step, k, stage, 0)          the stage loop's step index, the draft slot, the stage's index
//   round   : (c0, c1, c2, c3) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), 10 rounds, the key bumped by
//             (W0, W1) between rounds
//   word 0  : the proposal uniform of slot k        -> r_draft[k][b]
//   word 1  : the accept uniform of slot k          -> u[b][k]
//   word 2  : the commit uniform, from k = 0 only   -> r_commit[b]
//   word 3  : unused
//   float   = float(x >> 8) * 2^-24                 exact, in [0, 1): torch.rand's range
//
// One thread per (b, k), k < max(K_draft, K_accept, 1); no LDS, no atomics, no workspace; plain vector stores.

#include <hip/hip_runtime.h>

#include "common.hpp"

namespace asd {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;
constexpr uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;

struct U4 {
    uint32_t x, y, z, w;
};

__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t hi0 = __umulhi(kM0, c.x), lo0 = kM0 * c.x;
        const uint32_t hi1 = __umulhi(kM1, c.z), lo1 = kM1 * c.z;
        c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += kW0;
        k1 += kW1;
    }
    return c;
}

__device__ __forceinline__ float to_uniform(uint32_t x) { return static_cast<float>(x >> 8) * 0x1.0p-24f; }

__global__ __launch_bounds__(kThreads) void k_step_uniforms(const uint64_t* __restrict__ seeds, uint32_t step, uint32_t stage,
                                                            int B, int K_draft, int K_accept, int K_max,
                                                            float* __restrict__ r_draft, float* __restrict__ u,
                                                            float* __restrict__ r_commit) {
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (idx >= static_cast<int64_t>(B) * K_max) return;
    const int b = static_cast<int>(idx / K_max);
    const int k = static_cast<int>(idx - static_cast<int64_t>(b) * K_max);
    const uint64_t seed = seeds[b];
    const U4 w = philox4x32_10(U4{step, static_cast<uint32_t>(k), stage, 0u}, static_cast<uint32_t>(seed),
                               static_cast<uint32_t>(seed >> 32));
    if (r_draft && k < K_draft) r_draft[static_cast<int64_t>(k) * B + b] = to_uniform(w.x);
    if (u && k < K_accept) u[static_cast<int64_t>(b) * K_accept + k] = to_uniform(w.y);
    if (r_commit && k == 0) r_commit[b] = to_uniform(w.z);
}

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT int asd_step_uniforms(const int64_t* seeds, uint32_t step, uint32_t stage, int B, int K_draft, int K_accept,
                                 float* r_draft, float* u, float* r_commit, void* stream) {
    if (B < 1 || K_draft < 0 || K_accept < 0 || K_draft > ASD_MAX_DRAFT_LEN || K_accept > ASD_MAX_DRAFT_LEN) return ASD_ERR_INVALID_ARG;
    if (!seeds || (!r_draft && !u && !r_commit)) return ASD_ERR_INVALID_ARG;
    if ((r_draft && K_draft < 1) || (u && K_accept < 1)) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(seeds, 8) || !aligned_to(r_draft, 4) || !aligned_to(u, 4) || !aligned_to(r_commit, 4)) return ASD_ERR_ALIGNMENT;
    const int K_max = K_draft > K_accept ? (K_draft > 1 ? K_draft : 1) : (K_accept > 1 ? K_accept : 1);
    const int64_t blocks = (static_cast<int64_t>(B) * K_max + kThreads - 1) / kThreads;      // <= 2^31 * 64 / 256
    hipLaunchKernelGGL(k_step_uniforms, dim3(static_cast<uint32_t>(blocks)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const uint64_t*>(seeds), step, stage, B, K_draft, K_accept, K_max, r_draft, u, r_commit);
    return launch_status();
}
