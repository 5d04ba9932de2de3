// logit_mask.hip -- a dense allow-list ahead of the samplers (vLLM's `allowed_token_ids`; the [rows, ceil(V/32)] bitmask of
// grammar / structured-output back ends), gfx950.
//
// logits[b][j][v] lies at b*ld_seq + j*ld_row + v (asd_logit_edit_rows' addressing; bf16 / f16 / f32).  Sequence b uses mask
// r = mask_row[b] (mask 0 with mask_row == NULL); r outside [0, R) leaves the sequence alone.  mask_bits is [R, W] with
// W = (V + 31) / 32: bit v & 31 of word v >> 5 SET keeps token v, CLEAR makes element v of every position j -inf.  Bits at
// v >= V of the last word are never looked at.
//
// The write stream itself -- slice geometry, head / tail, 16-byte all-clear stores, blended mixed chunks -- is mask_slice of
// logit_mask_device.hpp, which asd_fsm_mask_rows (fsm.hip) instantiates too; this file picks the mask row per SEQUENCE.

#include <hip/hip_runtime.h>

#include "common.hpp"
#include "logit_mask_device.hpp"

namespace asd {
namespace {

using namespace mask_stream;

template <int DT>
__global__ __launch_bounds__(kThreads) void k_logit_mask_rows(void* logits, int64_t ld_seq, int64_t ld_row, int K1, int V,
                                                              const uint32_t* __restrict__ mask_bits, int R,
                                                              const int32_t* __restrict__ mask_row, int words_per_slice) {
    using T = typename Elem<DT>::type;
    const int row = static_cast<int>(blockIdx.x);
    const int b = static_cast<int>(static_cast<uint32_t>(row) / static_cast<uint32_t>(K1));
    const int j = row - b * K1;
    const int r = mask_row ? mask_row[b] : 0;
    if (r < 0 || r >= R) return;                                    // no list, or a damaged index: the sequence is not touched
    const int W = static_cast<int>((static_cast<int64_t>(V) + 31) >> 5);
    mask_slice<DT>(static_cast<T*>(logits) + static_cast<int64_t>(b) * ld_seq + static_cast<int64_t>(j) * ld_row,
                   mask_bits + static_cast<int64_t>(r) * W, V, words_per_slice);
}

}  // namespace
}  // namespace asd

using namespace asd;

ASD_EXPORT int asd_logit_mask_rows(void* logits, int dtype, int64_t ld_seq, int64_t ld_row, int B, int K1, int V,
                                   const uint32_t* mask_bits, int R, const int32_t* mask_row, void* stream) {
    if (B < 0 || K1 < 0 || V < 0 || R < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0 || K1 == 0 || V == 0 || R == 0) return ASD_OK;
    const int esz = dtype_size(dtype);
    if (esz == 0) return ASD_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(B) * K1 > INT32_MAX) return ASD_ERR_UNSUPPORTED;
    if (!logits || !mask_bits) return ASD_ERR_INVALID_ARG;
    if (ld_row < V || ld_seq < static_cast<int64_t>(K1) * ld_row) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(logits, static_cast<size_t>(esz)) || !aligned_to(mask_bits, 4)) return ASD_ERR_ALIGNMENT;
    const int64_t rows = static_cast<int64_t>(B) * K1;
    const int W = static_cast<int>((static_cast<int64_t>(V) + 31) / 32);
    const int words_per_slice = slice_words(rows, V, current_device_cus());
    const int S = (W + words_per_slice - 1) / words_per_slice;
    const dim3 grid(static_cast<uint32_t>(rows), static_cast<uint32_t>(S));
    dispatch_dtype(dtype, [&](auto dt) {
        hipLaunchKernelGGL((k_logit_mask_rows<decltype(dt)::value>), grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                           logits, ld_seq, ld_row, K1, V, mask_bits, R, mask_row, words_per_slice);
    });
    return launch_status();
}
