// common.hpp -- host-side helpers shared by the launchers of libasd_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "asd_hip.h"

#define ASD_EXPORT extern "C" __attribute__((visibility("default")))

namespace asd {

inline int launch_status() { return hipGetLastError() == hipSuccess ? ASD_OK : ASD_ERR_HIP; }

inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

inline int dtype_size(int dtype) {
    switch (dtype) {
        case ASD_DTYPE_F32: return 4;
        case ASD_DTYPE_BF16:
        case ASD_DTYPE_F16: return 2;
        default: return 0;
    }
}

// number of CUs of the CURRENT device (cached per device id; the query is slow)
int current_device_cus();

// workgroups per row of the row-streaming kernels that cut a row into vocabulary slices (greedy.hip, which defines it, and
// top_logprobs.hip): R rows of V elements of esz bytes on `cus` compute units
int choose_splits(int64_t R, int V, int esz, int cus);

// ---- shared by the launchers of the sampling steps, the verify step (verify_accept.hip) and the lm_head / linear kernels ----

// f(std::integral_constant<int, ASD_DTYPE_*>{}): the kernels take the element type as a template argument.  Whatever is not
// BF16 or F16 takes the F32 branch (the callers have rejected unknown dtypes through dtype_size before).
template <class F>
auto dispatch_dtype(int dtype, F&& f) {
    switch (dtype) {
        case ASD_DTYPE_BF16: return f(std::integral_constant<int, ASD_DTYPE_BF16>{});
        case ASD_DTYPE_F16: return f(std::integral_constant<int, ASD_DTYPE_F16>{});
        default: return f(std::integral_constant<int, ASD_DTYPE_F32>{});
    }
}
// f(std::true_type{}) or f(std::false_type{}): a run-time flag that the kernels take as a template argument
template <class F>
auto dispatch_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// a logits row as the sampling kernels stream it: 16-byte vectors, tiles of 64 vectors
struct RowGeom {
    int esz;              // bytes per element; 0: unknown dtype
    int nvec, n_tiles;
    bool whole;           // the row is a whole number of 16-byte vectors
};
inline RowGeom row_geom(int V, int dtype) {
    RowGeom g{};
    g.esz = dtype_size(dtype);
    const int64_t bytes = static_cast<int64_t>(V) * g.esz;
    g.nvec = static_cast<int>(bytes / 16);
    g.n_tiles = (g.nvec + 63) / 64;
    g.whole = bytes % 16 == 0;
    return g;
}
// rows of stride ld (elements) from p on start on 16-byte boundaries
inline bool rows_aligned(const void* p, int64_t ld, int esz) { return aligned_to(p, 16) && (ld * esz) % 16 == 0; }

inline bool valid_inv_temperature(float t) { return t > 0.0f && t < 3.0e38f; }      // (false for NaN)
// the kernels work in the log2 domain: 2^(x c2) = e^(x / T)
inline float log2_scale(float inv_temperature) { return static_cast<float>(1.4426950408889634074 * static_cast<double>(inv_temperature)); }

// what a call truncates the distribution to (HF's TopKLogitsWarper -> TopPLogitsWarper)
struct Truncation {
    bool nucleus;         // 0 < top_p < 1
    int top_k;            // the bound where it bounds anything (0 < top_k < V), else 0
    int levels;           // radix levels of the mass select: 0 without a nucleus, 2 for 16-bit logits, 3 for f32
};
inline Truncation truncation(int top_k, float top_p, int V, int dtype) {
    Truncation t{};
    t.nucleus = top_p > 0.0f && top_p < 1.0f;
    t.top_k = (top_k > 0 && top_k < V) ? top_k : 0;
    t.levels = t.nucleus ? (dtype == ASD_DTYPE_F32 ? 3 : 2) : 0;
    return t;
}


// min-p (HF's MinPLogitsWarper, behind top-k and top-p): <= 0 is the off switch, (0, 1] a bound, anything else (NaN included)
// an argument error
inline bool valid_min_p(float min_p) { return min_p <= 1.0f; }
// x_max + this is min-p's threshold on the raw logits: p_v >= min_p p_max  <=>  x_v >= x_max + T ln(min_p)
inline float min_p_delta(float min_p, float inv_temperature) {
    return static_cast<float>(log(static_cast<double>(min_p)) / static_cast<double>(inv_temperature));
}

// One sequence of the packed sampling table (asd_sampling_rows_pack, include/asd_hip.h "Per-sequence sampling parameters"):
// what a scalar launch with the sequence's (inv_temperature, top_k, top_p, min_p) puts into its parameter block, formed on
// the host by the functions above -- so row b of a *_rows launch works on the bits a scalar launch with its values would.
struct SamplingRow {
    float c2;             // log2_scale(inv_temperature)
    float top_p;          // as given (1 when the caller passed none); read by the mass select only when levels > 0
    int32_t levels;       // truncation(...).levels
    int32_t top_k;        // truncation(...).top_k: the bound where it bounds anything, else 0
    float mp_delta;       // min_p_delta(min_p, inv_temperature) where min_p > 0, else -inf
    uint32_t clamp;       // 1 where min_p > 0: the row takes the kMinP select and the "lp above 0 reads as 0" rule
    uint32_t reserved[2];
};
static_assert(sizeof(SamplingRow) == ASD_SAMPLING_ROW_BYTES, "SamplingRow");

}  // namespace asd
