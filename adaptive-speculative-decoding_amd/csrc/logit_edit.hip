// logit_edit.hip -- a sparse in-place edit of a few logits per row ahead of the samplers (OpenAI's `logit_bias`, vLLM's
// `bad_words` / `logit_bias` / `min_tokens`), gfx950.
//
// logits[b][j][v] lies at b*ld_seq + j*ld_row + v (asd_top_logprobs' addressing; bf16 / f16 / f32).  Row b owns the entries
// [row_first[b], row_first[b+1]) of three parallel arrays (id, bias, until) -- or, with row_first == NULL, the entries [0, n)
// like every other row.  At position j the logits row decides generated token number
//   g = seq_len[b] - start + offset + j                (0-based among the row's generated tokens)
// and an entry does ONE of three things to element `id` of that row:
//   g < until            the element becomes -inf                          (a ban: until = INT32_MAX for ever, min_tokens until then)
//   else, bias != 0      the element becomes round_to_dtype((float)x + bias)   (one f32 addition, one rounding to nearest even)
//   else                 nothing is stored
// An id outside [0, V) is skipped.  The host packs distinct ids per row, so no two lanes write one element: no atomics, and
// nothing but the named elements is written.  Every store is an ordinary per-lane vector-memory store.
//
// One workgroup per (b, j) walks the row's entries, one per lane and round; at most ASD_MAX_LOGIT_EDITS entries of a row are
// honoured, and an entry index is clamped into [0, n) before it is read, so a damaged row_first cannot leave the arrays.
// Latency-bound: a launch touches at most 1024 * K1 elements per sequence.

#include <hip/hip_runtime.h>

#include "common.hpp"

namespace asd {
namespace {

constexpr int kThreads = 256;

// round to nearest even, the conversion of torch's .to(bfloat16); a NaN stays a (quiet) NaN
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return static_cast<uint16_t>((u >> 16) | 0x0040u);
    return static_cast<uint16_t>((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

template <int DT>
__device__ __forceinline__ void edit_one(void* logits, int64_t at, float bias, bool ban) {
    if constexpr (DT == ASD_DTYPE_BF16) {
        uint16_t* const p = static_cast<uint16_t*>(logits) + at;
        if (ban) *p = 0xFF80u;
        else *p = f32_to_bf16(__uint_as_float(static_cast<uint32_t>(*p) << 16) + bias);
    } else if constexpr (DT == ASD_DTYPE_F16) {
        _Float16* const p = static_cast<_Float16*>(logits) + at;
        if (ban) *p = __builtin_bit_cast(_Float16, static_cast<uint16_t>(0xFC00u));
        else *p = static_cast<_Float16>(static_cast<float>(*p) + bias);       // v_cvt_f16_f32: to nearest even
    } else {
        float* const p = static_cast<float*>(logits) + at;
        if (ban) *p = -INFINITY;
        else *p = *p + bias;
    }
}

template <int DT>
__global__ __launch_bounds__(kThreads) void k_logit_edit_rows(void* logits, int64_t ld_seq, int64_t ld_row, int K1, int V,
                                                              const int32_t* __restrict__ edit_id,
                                                              const float* __restrict__ edit_bias,
                                                              const int32_t* __restrict__ edit_until,
                                                              const int32_t* __restrict__ row_first, int n,
                                                              const int32_t* __restrict__ seq_len, int start, int offset) {
    const int row = static_cast<int>(blockIdx.x);
    const int b = static_cast<int>(static_cast<uint32_t>(row) / static_cast<uint32_t>(K1));
    const int j = row - b * K1;
    // the row's entries: [first, first + n_own) of the n uploaded ones, at most ASD_MAX_LOGIT_EDITS, never outside the arrays
    int first = 0, n_own = n;
    if (row_first) {
        first = row_first[b];
        n_own = row_first[b + 1] - first;
    }
    if (first < 0 || first > n) n_own = 0;
    n_own = n_own > n - first ? n - first : n_own;
    n_own = n_own < 0 ? 0 : (n_own > ASD_MAX_LOGIT_EDITS ? ASD_MAX_LOGIT_EDITS : n_own);
    const int64_t g = static_cast<int64_t>(seq_len[b]) - start + offset + j;
    const int64_t base = static_cast<int64_t>(b) * ld_seq + static_cast<int64_t>(j) * ld_row;
    for (int e = static_cast<int>(threadIdx.x); e < n_own; e += kThreads) {
        const int id = edit_id[first + e];
        if (id < 0 || id >= V) continue;                 // the launcher cannot check the ids: never written
        const float bias = edit_bias[first + e];
        const bool ban = g < static_cast<int64_t>(edit_until[first + e]);
        if (!ban && bias == 0.0f) continue;              // stores nothing: the bits stay
        edit_one<DT>(logits, base + id, bias, ban);
    }
}

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT int asd_logit_edit_rows(void* logits, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V,
                                   const int32_t* edit_id, const float* edit_bias, const int32_t* edit_until,
                                   const int32_t* row_first, int n_shared, const int32_t* seq_len, int start, int offset,
                                   void* stream) {
    if (B < 0 || K1 < 0 || V < 0 || n_shared < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0 || K1 == 0 || n_shared == 0) return ASD_OK;
    const int esz = dtype_size(dtype);
    if (esz == 0) return ASD_ERR_UNSUPPORTED;
    if (!row_first && n_shared > ASD_MAX_LOGIT_EDITS) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(B) * K1 > INT32_MAX) return ASD_ERR_UNSUPPORTED;
    if (!logits || !edit_id || !edit_bias || !edit_until || !seq_len) return ASD_ERR_INVALID_ARG;
    if (ld_row < V || ld_seq < static_cast<int64_t>(K1) * ld_row) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(logits, static_cast<size_t>(esz))) return ASD_ERR_ALIGNMENT;
    const dim3 grid(static_cast<uint32_t>(static_cast<int64_t>(B) * K1));
    dispatch_dtype(dtype, [&](auto dt) {
        hipLaunchKernelGGL((k_logit_edit_rows<decltype(dt)::value>), grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                           logits, ld_seq, ld_row, K1, V, edit_id, edit_bias, edit_until, row_first, n_shared, seq_len, start,
                           offset);
    });
    return launch_status();
}
