// logit_mask_device.hpp -- the write stream of the dense token masks, gfx950: ONE body for asd_logit_mask_rows (logit_mask.hip,
// a mask per sequence) and asd_fsm_mask_rows (fsm.hip, a mask per sequence AND position).  The two kernels differ only in how
// they pick the row of the [R, W] bit table; everything from there on -- the slice geometry, the head / tail handling, the
// 16-byte all-clear stores and the blended mixed chunks -- is mask_slice below, instantiated by both.
//
// A WRITE stream: the kernel needs the mask, never a logit's value.  A lane takes 16 bytes of a row per round -- 8 bf16 / f16
// elements (one mask byte) or 4 f32 elements (one nibble): all bits clear is one 16-byte store of -inf, all set is nothing.
// Mixed chunks number at most twice the allowed tokens, so with a short list the stream is the all-clear case: one
// global_store_dwordx4 per lane and round, the widest and cheapest store per byte.  A MIXED chunk is loaded, blended and stored
// back whole -- its kept elements receive the bits they had -- because single-element stores of its clear bits are bound by
// store issue, not by bytes: at a list of V / 2 ids (every chunk mixed, four 2-byte stores per lane and round) they took
// 55 us on [32, 9, 152064] bf16 against 44 us for torch's masked_fill_, which reads and writes everything.  One load and one
// store per mixed chunk never moves more bytes than that.  Nothing is shared: no LDS, no atomics, every access an ordinary
// per-lane vector-memory load or store.
//
// Alignment: a row base is aligned only to the element size (odd V with ld_row == V, a slice, a view at an odd offset), so a
// slice of a row is a head of single elements up to the first 16-byte boundary, whole 16-byte chunks, and a tail of single
// elements.  A chunk's mask bits start at an arbitrary bit: a funnel over two adjacent words; the second word is loaded only
// by a lane whose chunk crosses into it, which no lane does when the row base is 16-byte aligned.
//
// Geometry: grid (B*K1) x S.  A row's W mask words are cut into S slices of whole words (slice_words below), so slices begin
// on mask-word boundaries and no two workgroups share a word's elements -- or a 16-byte chunk: a chunk lies inside one slice.
// The result does not depend on S: there is nothing to reduce.
#pragma once

#include <hip/hip_runtime.h>

#include "common.hpp"

namespace asd {
namespace mask_stream {

constexpr int kThreads = 256;
constexpr int kUnroll = 2;               // chunks a lane has in flight: the mask loads of both are issued before the stores
constexpr int kSliceWords = 128;         // slices are whole multiples of this: 4096 elements, one round of kUnroll chunks per lane
                                         // of 16-bit elements (two of f32), so no round of a slice runs with most lanes idle

template <int DT>
struct Elem {
    using type = uint16_t;
    static constexpr uint32_t one = DT == ASD_DTYPE_BF16 ? 0xFF80u : 0xFC00u;       // -inf, as logit_edit.hip's edit_one writes it
    static constexpr uint32_t four = one | (one << 16);                           // a dword of them
};
template <>
struct Elem<ASD_DTYPE_F32> {
    using type = uint32_t;
    static constexpr uint32_t one = 0xFF800000u;
    static constexpr uint32_t four = one;
};

// Mask words per slice; S = ceil(W / words) workgroups per row.  The stream wants every CU busy with several waves (a wave has
// one 16-byte store instruction in issue at a time and hides its latency only behind other waves: 8 workgroups of 4 waves fill
// a CU's 32 wave slots), so the aim is 8 workgroups per CU over the whole launch; a slice is a whole multiple of kSliceWords
// (8 KiB of 16-bit elements: under that the head / tail handling and the launch itself outweigh the stores) unless the row is
// shorter.  V = 152064 (W = 4752) bf16 on 256 CUs: B = 32, K1 = 9 -> 288 rows want 8 slices, 640 words each, 2304 workgroups
// of 40 KB; B = 32, K1 = 1 -> 128 words, S = 38, 1216 workgroups of 8 KB; B = 1, K1 = 9 -> 128 words, 342 workgroups (one
// workgroup per row would use 9 of the CUs).
inline int slice_words(int64_t rows, int V, int cus) {
    if (cus <= 0) cus = 256;
    const int64_t W = (static_cast<int64_t>(V) + 31) / 32;
    if (W <= kSliceWords) return static_cast<int>(W);
    const int64_t want = (static_cast<int64_t>(cus) * 8 + rows - 1) / rows;         // slices per row for 8 workgroups per CU
    int64_t words = ((W + want - 1) / want + kSliceWords - 1) / kSliceWords * kSliceWords;
    while ((W + words - 1) / words > 65535) words += kSliceWords;                   // gridDim.y
    return static_cast<int>(words);
}

// Slice blockIdx.y of ONE logits row x[0 .. V) under ONE mask row bits[0 .. W): element v becomes -inf where bit v & 31 of
// word v >> 5 is clear.  Called by every thread of a kThreads workgroup with the same arguments.
template <int DT>
__device__ __forceinline__ void mask_slice(typename Elem<DT>::type* const x, const uint32_t* __restrict__ const bits, int V,
                                           int words_per_slice) {
    using T = typename Elem<DT>::type;
    constexpr int kPer = 16 / static_cast<int>(sizeof(T));          // elements of one 16-byte chunk: 8 or 4
    constexpr uint32_t kFull = (1u << kPer) - 1u;
    const int W = static_cast<int>((static_cast<int64_t>(V) + 31) >> 5);
    // this workgroup's elements [v0, v1) of the row: whole mask words, the last one cut at V
    const int64_t w0 = static_cast<int64_t>(blockIdx.y) * words_per_slice;
    if (w0 >= W) return;
    const int64_t w1 = w0 + words_per_slice < W ? w0 + words_per_slice : W;
    const int v0 = static_cast<int>(w0 << 5);
    const int v1 = static_cast<int>((w1 << 5) < V ? (w1 << 5) : V);
    const int tid = static_cast<int>(threadIdx.x);

    // head: the single elements in front of the first 16-byte boundary (at most kPer - 1 of them)
    const uintptr_t addr = reinterpret_cast<uintptr_t>(x + v0);
    int head = static_cast<int>(((16u - (addr & 15u)) & 15u) / sizeof(T));
    head = head < v1 - v0 ? head : v1 - v0;
    const int c0 = v0 + head;                                       // the first chunk's first element
    const int n_chunks = (v1 - c0) / kPer;
    const int t0 = c0 + n_chunks * kPer;                            // tail: [t0, v1), fewer than kPer elements
    {
        const int v = tid < head ? v0 + tid : t0 + (tid - head);
        if (tid < head + (v1 - t0) && !((bits[v >> 5] >> (v & 31)) & 1u)) x[v] = static_cast<T>(Elem<DT>::one);
    }

    const uint4 fill = make_uint4(Elem<DT>::four, Elem<DT>::four, Elem<DT>::four, Elem<DT>::four);
    for (int c = tid; c < n_chunks; c += kThreads * kUnroll) {
        uint32_t keep[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int cu = c + u * kThreads;
            keep[u] = kFull;                                        // past the slice: nothing to store
            if (cu < n_chunks) {
                const int v = c0 + cu * kPer;                       // v + kPer <= v1 <= V: every bit read below belongs to a token
                const int w = v >> 5, sh = v & 31;
                uint32_t m = bits[w] >> sh;
                if (sh + kPer > 32) m |= bits[w + 1] << (32 - sh);  // the chunk crosses into word w + 1 <= (V - 1) >> 5
                keep[u] = m & kFull;
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (keep[u] == kFull) continue;
            T* const p = x + c0 + (c + u * kThreads) * kPer;
            uint4* const q = reinterpret_cast<uint4*>(p);           // 16-byte aligned by the head
            if (keep[u] == 0u) {
                *q = fill;
            } else {                                                // mixed: the kept elements get their own bits back
                const uint4 old = *q;
                uint32_t km[4];                                     // per dword: ones over the kept elements
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if constexpr (kPer == 8)
                        km[i] = (((keep[u] >> (2 * i)) & 1u) ? 0x0000FFFFu : 0u) | (((keep[u] >> (2 * i + 1)) & 1u) ? 0xFFFF0000u : 0u);
                    else
                        km[i] = ((keep[u] >> i) & 1u) ? 0xFFFFFFFFu : 0u;
                }
                *q = make_uint4((old.x & km[0]) | (fill.x & ~km[0]), (old.y & km[1]) | (fill.y & ~km[1]),
                                (old.z & km[2]) | (fill.z & ~km[2]), (old.w & km[3]) | (fill.w & ~km[3]));
            }
        }
    }
}

}  // namespace mask_stream
}  // namespace asd
