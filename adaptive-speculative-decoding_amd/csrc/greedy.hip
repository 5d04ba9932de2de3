// greedy.hip -- greedy decoding (temperature 0): arg-max + log-sum-exp + accepted prefix + commit token in ONE launch, gfx950.
//
// One streaming pass over the target's [B][K+1][V] output, read IN PLACE (sequence stride ld_seq, row stride ld_row; bf16 / f16 /
// f32).  Row (b, k < K) scores the draft token tok[b, k], row (b, K) is the bonus row; K == 0 is the plain greedy step.  Per row
// the pass keeps the online log-sum-exp pair (m2, s) of lse_device.hpp and the arg-max (value, lowest id); there are no random
// numbers and the rows are read once (the sampled step reads them twice: verify, then the residual draw).
//
// Arg-max rules (those of asd_lm_head_verify_ex): the lowest id among the maxima; a NaN logit never wins; -1 when the row has no
// logit above -inf.  The running best is only replaced on a strict `>` while a lane walks increasing ids, and lanes / waves /
// slices are merged on (value, lowest id), so the result does not depend on the geometry.
//
// Geometry.  grid = (rows, splits): a row is cut into `splits` contiguous vocabulary slices (16-byte vectors; the unaligned head
// of the row belongs to slice 0, the ragged tail to the last slice, both done with scalar loads), one workgroup of 512 lanes per
// slice.  A slice without elements contributes the neutral partial.
//
// Hand-off (nobody waits for anybody: no polling, no status word).  Each slice writes its partial (m2, s, best value, best id)
// with a plain store; every wave drains vmcnt; workgroup barrier; lane 0 does ONE agent-scope release and a relaxed agent-scope
// fetch_add on the row's ticket.  The workgroup that draws the last ticket does one agent-scope acquire, a barrier, then plain
// loads, and combines the partials in SLICE order (its own included), so a geometry gives the same bits on every run.  The row's
// finisher writes the row's outputs and its (arg-max, lp) record, then takes a second ticket, the sequence's, the same way; the
// row that draws the last one reads the K + 1 records and writes n_acc / drawn / lp_drawn.  The tickets are zeroed by a
// hipMemsetAsync ahead of every launch, so the workspace needs no initialisation and two calls in flight need two workspaces.

#include <hip/hip_runtime.h>

#define ASD_DPP_ASM_REDUCTIONS 1   // (this file is built with -ffp-contract=off, like verify_accept.hip)
#include "lse_device.hpp"

namespace asd {
namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kUnroll = 4;                     // 16-byte loads per lane and batch; two batches in flight
constexpr int kNoIndex = 0x7fffffff;
constexpr int kTicketStride = 16;              // u32 units: one 64-byte line per ticket
constexpr uint32_t kBatchBytes = static_cast<uint32_t>(kUnroll) * kThreads * 16u;

struct __attribute__((aligned(16))) Partial {
    float m2, s, bv;
    int bi;
};
struct __attribute__((aligned(8))) RowRecord {
    int argmax;
    float lp;
};

struct GreedyParams {
    const void* logits;
    int64_t ld_seq, ld_row;
    const int32_t* tok;
    int B, K, V, S;
    float c2;
    int32_t* argmax_out;
    float* lp_argmax;
    float* lp_target;
    uint8_t* accept;
    int32_t* n_acc;
    int32_t* drawn;
    float* lp_drawn;
    uint32_t* seq_tickets;
    uint32_t* row_tickets;
    RowRecord* records;
    Partial* partials;
};

__device__ __forceinline__ void arg_merge(float& bv, int& bi, float v, int i) {
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

// one element: ids arrive in increasing order within a lane, so `>` keeps the lowest id of a maximum; NaN compares false
__device__ __forceinline__ void accum_one(float x, int id, float c2, float& m2, float& s, float& bv, int& bi) {
    if (x > bv) { bv = x; bi = id; }
    accum_scalar(x, c2, m2, s);
}

// one 16-byte vector whose first element has vocabulary id `id0`: accum8 / accum4's (m2, s) arithmetic, plus the arg-max.
// fmaxf, not the bare v_max of lse_device.hpp: a signalling NaN (any bf16 / f16 NaN pattern can be one after the integer unpack)
// would come OUT of a bare v_max in IEEE mode and hide the vector's real maximum from the arg-max.
template <int N>
__device__ __forceinline__ void accum_arg(const float (&x)[N], int id0, float c2, float& m2, float& s, float& bv, int& bi) {
    float vmax;
    if constexpr (N == 8) vmax = fmaxf(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])), fmaxf(fmaxf(x[4], x[5]), fmaxf(x[6], x[7])));
    else vmax = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
    if (vmax > bv) {
        int j = N - 1;
#pragma unroll
        for (int i = N - 2; i >= 0; --i) j = (x[i] == vmax) ? i : j;
        bv = vmax;
        bi = id0 + j;
    }
    const float M = fmaxf(m2, vmax * c2);
    const float scale = fast_exp2(m2 - M);
    float e[N];
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = fast_exp2(fmaf(x[i], c2, -M));
    float sum;
    if constexpr (N == 8) sum = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
    else sum = (e[0] + e[1]) + (e[2] + e[3]);
    s = fmaf(s, scale, sum);
    m2 = M;
}

template <int DT>
__device__ __forceinline__ void accum_vec(const u32x4& v, int id0, float c2, float& m2, float& s, float& bv, int& bi) {
    if constexpr (DT == ASD_DTYPE_BF16) {
        float x[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[2 * i] = __uint_as_float(v[i] << 16);
            x[2 * i + 1] = __uint_as_float(v[i] & 0xFFFF0000u);
        }
        accum_arg<8>(x, id0, c2, m2, s, bv, bi);
    } else if constexpr (DT == ASD_DTYPE_F16) {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        float x[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t w = v[i];
            const h2 h = __builtin_bit_cast(h2, w);
            x[2 * i] = static_cast<float>(h[0]);
            x[2 * i + 1] = static_cast<float>(h[1]);
        }
        accum_arg<8>(x, id0, c2, m2, s, bv, bi);
    } else {
        float x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = __uint_as_float(v[i]);
        accum_arg<4>(x, id0, c2, m2, s, bv, bi);
    }
}

// lp = ln2 * (x c2 - (m2 + log2 s)): finish_row's arithmetic, so an accepted token's lp_target and its row's lp_argmax are the
// same operations on the same bits
__device__ __forceinline__ float row_logprob(float x, float c2, double l2) {
    return static_cast<float>(kLn2d * (static_cast<double>(x) * static_cast<double>(c2) - l2));
}

template <int DT>
__global__ __launch_bounds__(kThreads) void k_greedy(const GreedyParams p) {
    using E = Elem<DT>;
    __shared__ Partial meet[kWaves + 1];       // the waves' partials; slot kWaves carries the "I drew the last ticket" word

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int S = p.S;
    const int K = p.K;
    const int K1 = K + 1;
    const float c2 = p.c2;
    const int row = static_cast<int>(blockIdx.x);
    const int split = static_cast<int>(blockIdx.y);
    const int b = static_cast<int>(static_cast<uint32_t>(row) / static_cast<uint32_t>(K1));
    const int k = row - b * K1;

    const char* rowp = static_cast<const char*>(p.logits) + (static_cast<int64_t>(b) * p.ld_seq + static_cast<int64_t>(k) * p.ld_row) * E::kBytes;
    const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(rowp) & 15u);   // (a multiple of the element size: launcher)
    int head = mis ? static_cast<int>((16u - mis) / E::kBytes) : 0;
    if (head > p.V) head = p.V;
    const int nvec = (p.V - head) / E::kPerVec;
    const int tail = p.V - head - nvec * E::kPerVec;
    const char* body = rowp + static_cast<int64_t>(head) * E::kBytes;
    const int v0 = static_cast<int>(static_cast<uint64_t>(nvec) * static_cast<uint32_t>(split) / static_cast<uint32_t>(S));
    const int v1 = static_cast<int>(static_cast<uint64_t>(nvec) * static_cast<uint32_t>(split + 1) / static_cast<uint32_t>(S));

    // the drafted token and its logit, fetched by lane 0 of EVERY slice under its stream: whichever slice ends up finishing the row
    // has them at hand (two dependent round trips that would otherwise sit behind the last ticket)
    int tk = -1;
    float x_tok = -INFINITY;
    bool tok_ok = false;
    if (tid == 0 && k < K) {
        tk = p.tok[static_cast<int64_t>(b) * K + k];
        if (tk >= 0 && tk < p.V) {
            x_tok = E::scalar(rowp, tk);
            tok_ok = true;
        }
    }

    float m2 = kSentinel, s = 0.0f, bv = -INFINITY;
    int bi = kNoIndex;
    if (wave == 0 && split == 0 && lane < head) accum_one(E::scalar(rowp, lane), lane, c2, m2, s, bv, bi);

    // ---- the stream: 16-byte buffer loads through a descriptor that ends with the slice (lanes past the end read nothing and are
    // skipped below); the next batch is issued before the current one is consumed
    const uint32_t end = v1 > v0 ? static_cast<uint32_t>(v1 - v0) * 16u : 0u;       // launcher: V * element size < 2^31
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(body) + static_cast<int64_t>(v0) * 16, 0, static_cast<int>(end), 0x00020000);
    const uint32_t lane_off = static_cast<uint32_t>(tid) * 16u;
    const int id_first = head + v0 * E::kPerVec;
    u32x4 cur[kUnroll], nxt[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) cur[j] = load16<true>(rsrc, lane_off + static_cast<uint32_t>(j) * (kThreads * 16u));
    for (uint32_t base = 0; base < end; base += kBatchBytes) {
#pragma unroll
        for (int j = 0; j < kUnroll; ++j)
            nxt[j] = load16<true>(rsrc, base + kBatchBytes + lane_off + static_cast<uint32_t>(j) * (kThreads * 16u));
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) {
            const uint32_t off = base + lane_off + static_cast<uint32_t>(j) * (kThreads * 16u);
            if (off < end) accum_vec<DT>(cur[j], id_first + static_cast<int>(off >> 4) * E::kPerVec, c2, m2, s, bv, bi);
        }
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) cur[j] = nxt[j];
    }
    if (wave == 0 && split == S - 1 && lane < tail) {
        const int id = head + nvec * E::kPerVec + lane;
        accum_one(E::scalar(rowp, id), id, c2, m2, s, bv, bi);
    }

    // ---- lanes -> wave (DPP; the lowest id among the lanes that hold the wave's maximum), waves -> workgroup in wave order
    const float wbv = wave_max(bv);                      // (bv is never NaN: it starts at -inf and only moves on `>`)
    int cand = (bv == wbv) ? bi : kNoIndex;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(cand, o, 64);
        cand = other < cand ? other : cand;
    }
    wave_merge(m2, s);
    if (lane == 0) {
        Partial w;
        w.m2 = m2; w.s = s; w.bv = wbv; w.bi = cand;
        meet[wave] = w;
    }
    __syncthreads();
    float rm2 = kSentinel, rs = 0.0f, rbv = -INFINITY;
    int rbi = kNoIndex;
    if (tid == 0) {
        for (int w = 0; w < kWaves; ++w) {
            const Partial q = meet[w];
            ms_merge(rm2, rs, q.m2, q.s);
            arg_merge(rbv, rbi, q.bv, q.bi);
        }
    }

    if (S > 1) {
        // ---- publish the slice; the workgroup that draws the row's last ticket combines all of them
        Partial* const mine = p.partials + static_cast<int64_t>(row) * S;
        if (tid == 0) {
            Partial w;
            w.m2 = rm2; w.s = rs; w.bv = rbv; w.bi = rbi;
            mine[split] = w;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const uint32_t old = __hip_atomic_fetch_add(p.row_tickets + static_cast<int64_t>(row) * kTicketStride, 1u, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT);
            const bool last = old == static_cast<uint32_t>(S - 1);
            if (last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            meet[kWaves].bi = last ? 1 : 0;
        }
        __syncthreads();
        if (meet[kWaves].bi == 0 || wave != 0) return;
        if (tid == 0) {
            rm2 = kSentinel; rs = 0.0f; rbv = -INFINITY; rbi = kNoIndex;
            for (int sl = 0; sl < S; ++sl) {       // slice order, not arrival order
                const Partial q = mine[sl];
                ms_merge(rm2, rs, q.m2, q.s);
                arg_merge(rbv, rbi, q.bv, q.bi);
            }
        }
    } else if (wave != 0) {
        return;
    }

    // ---- the row: wave 0 of the row's finisher; lane 0 holds (rm2, rs, rbv, rbi)
    if (lane == 0) {
        const int amax = rbi == kNoIndex ? -1 : rbi;
        const double l2 = static_cast<double>(rm2) + log2_split(rs);
        const float lp_a = amax >= 0 ? row_logprob(rbv, c2, l2) : NAN;
        if (p.argmax_out) p.argmax_out[row] = amax;
        if (p.lp_argmax) p.lp_argmax[row] = lp_a;
        if (k < K) {
            const int64_t at = static_cast<int64_t>(b) * K + k;
            if (p.lp_target) p.lp_target[at] = tok_ok ? row_logprob(x_tok, c2, l2) : -INFINITY;
            if (p.accept) p.accept[at] = (amax >= 0 && tk == amax) ? 1 : 0;
        }
        if (K == 0) {
            p.n_acc[b] = 0;
            p.drawn[b] = amax;
            p.lp_drawn[b] = lp_a;
        } else {
            RowRecord r;
            r.argmax = amax; r.lp = lp_a;
            p.records[row] = r;
        }
    }
    if (K == 0) return;

    // ---- the sequence's ticket: the row that draws the last of its K + 1 finishes the sequence (only this wave stored, and only
    // this wave reads: its own drain and its own acquire, no barrier)
    uint32_t last = 0;
    if (lane == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t old = __hip_atomic_fetch_add(p.seq_tickets + static_cast<int64_t>(b) * kTicketStride, 1u, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT);
        last = old == static_cast<uint32_t>(K) ? 1u : 0u;
    }
    last = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(last)));
    if (last == 0u) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const RowRecord* const recs = p.records + static_cast<int64_t>(b) * K1;
    bool flag = false;
    if (lane < K) {                                  // K <= 64: lane <-> draft position
        const RowRecord r = recs[lane];
        const int t = p.tok[static_cast<int64_t>(b) * K + lane];
        flag = r.argmax >= 0 && t == r.argmax;       // (a tok of -1 never matches)
    }
    const unsigned long long inv = ~__ballot(flag);
    int n = inv ? __builtin_ctzll(inv) : 64;
    if (n > K) n = K;
    if (lane == 0) {
        const RowRecord r = recs[n];                 // n == K: the bonus row
        p.n_acc[b] = n;
        p.drawn[b] = r.argmax;
        p.lp_drawn[b] = r.lp;
    }
}

// the workspace: the sequences' tickets, the rows' tickets (one 64-byte line each: zeroed before every launch), the rows' records,
// then `splits` partials per row
struct Layout {
    size_t ticket_bytes, record_off, partial_off, total;
};
inline Layout layout(int B, int K, int splits) {
    const size_t R = static_cast<size_t>(B) * (static_cast<size_t>(K) + 1);
    Layout w{};
    w.ticket_bytes = round_up((static_cast<size_t>(B) + R) * kTicketStride * sizeof(uint32_t), 256);
    w.record_off = w.ticket_bytes;
    w.partial_off = w.record_off + round_up(R * sizeof(RowRecord), 256);
    w.total = w.partial_off + round_up(R * static_cast<size_t>(splits) * sizeof(Partial), 256);
    return w;
}

}  // namespace

// Workgroups per row.  Whole rows where they fill the CUs evenly; otherwise the estimate verify_accept.hip fitted to its slice
// sweeps (bytes of the fullest CU, floored by the chip-wide stream, plus a fixed cost per workgroup), which this kernel has not
// been swept against.  A slice is never cut below 16 KiB.  (Declared in common.hpp: top_logprobs.hip streams the same geometry.)
int choose_splits(int64_t R, int V, int esz, int cus) {
    if (R <= 0 || cus <= 0) return 1;
    if (R >= cus && (R % cus == 0 || 10 * (R % cus) >= 6 * cus || R / cus >= 6)) return 1;
    const int64_t row_bytes = static_cast<int64_t>(V) * esz;
    int64_t cap = row_bytes / 16384;
    const int64_t most = R >= cus ? 8 : 16;
    if (cap > most) cap = most;
    if (cap < 1) cap = 1;
    const double a = 6.0 * static_cast<double>(row_bytes) / 304128.0, q = static_cast<double>(R) / cus;
    int best = 1;
    double best_est = 0.0;
    for (int S = 1; S <= cap; ++S) {
        const int64_t wgs = R * S;
        const double load = static_cast<double>((wgs + cus - 1) / cus) / S;
        const double est = a * (load > 1.05 * q ? load : 1.05 * q) + 0.2 * q * S;
        if (S == 1 || est < best_est - 1e-9) { best = S; best_est = est; }
    }
    return best;
}

}  // namespace asd

using namespace asd;

ASD_EXPORT size_t asd_verify_greedy_workspace_bytes(int B, int K, int V, int dtype) {
    (void)V;
    (void)dtype;
    if (B <= 0 || K < 0) return 256;
    return layout(B, K, ASD_MAX_SPLITS).total;
}

ASD_EXPORT int asd_verify_greedy(const void* logits, int dtype, int64_t ld_seq, int64_t ld_row, const int32_t* tok, int B, int K,
                                 int V, float inv_temperature, int splits, int32_t* argmax_out, float* lp_argmax, float* lp_target,
                                 uint8_t* accept, int32_t* n_acc, int32_t* drawn, float* lp_drawn, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (B > 0 && (!n_acc || !drawn || !lp_drawn)) return ASD_ERR_INVALID_ARG;
    if (!valid_inv_temperature(inv_temperature)) return ASD_ERR_INVALID_ARG;
    if (B < 0 || K < 0 || V < 0) return ASD_ERR_INVALID_ARG;
    if (B == 0) return ASD_OK;
    if (V == 0) return ASD_ERR_INVALID_ARG;
    if (K > ASD_MAX_DRAFT_LEN) return ASD_ERR_UNSUPPORTED;
    const int esz = dtype_size(dtype);
    if (esz == 0) return ASD_ERR_UNSUPPORTED;
    if (splits < 0 || splits > ASD_MAX_SPLITS) return ASD_ERR_UNSUPPORTED;
    if (!logits || !workspace || (K > 0 && !tok)) return ASD_ERR_INVALID_ARG;
    if (ld_row < V || ld_seq < (static_cast<int64_t>(K) + 1) * ld_row) return ASD_ERR_INVALID_ARG;
    if (!aligned_to(logits, static_cast<size_t>(esz))) return ASD_ERR_ALIGNMENT;
    if (!aligned_to(workspace, 256)) return ASD_ERR_WORKSPACE;
    const int64_t R = static_cast<int64_t>(B) * (K + 1);
    if (static_cast<int64_t>(V) * esz >= (int64_t{1} << 31)) return ASD_ERR_UNSUPPORTED;      // 32-bit byte offsets within a row
    const int S = splits > 0 ? splits : choose_splits(R, V, esz, current_device_cus());
    if (R * S > INT32_MAX) return ASD_ERR_UNSUPPORTED;
    const Layout w = layout(B, K, S);
    if (workspace_bytes < w.total) return ASD_ERR_WORKSPACE;

    GreedyParams p{};
    p.logits = logits; p.ld_seq = ld_seq; p.ld_row = ld_row; p.tok = tok;
    p.B = B; p.K = K; p.V = V; p.S = S;
    p.c2 = log2_scale(inv_temperature);
    p.argmax_out = argmax_out; p.lp_argmax = lp_argmax; p.lp_target = lp_target; p.accept = accept;
    p.n_acc = n_acc; p.drawn = drawn; p.lp_drawn = lp_drawn;
    char* const ws = static_cast<char*>(workspace);
    p.seq_tickets = reinterpret_cast<uint32_t*>(ws);
    p.row_tickets = p.seq_tickets + static_cast<size_t>(B) * kTicketStride;
    p.records = reinterpret_cast<RowRecord*>(ws + w.record_off);
    p.partials = reinterpret_cast<Partial*>(ws + w.partial_off);

    hipStream_t st = static_cast<hipStream_t>(stream);
    if (K > 0 || S > 1) {      // (K == 0 with whole rows takes no ticket at all)
        if (hipMemsetAsync(workspace, 0, w.ticket_bytes, st) != hipSuccess) return ASD_ERR_HIP;
    }
    const dim3 grid(static_cast<uint32_t>(R), static_cast<uint32_t>(S));
    dispatch_dtype(dtype, [&](auto dt) {
        hipLaunchKernelGGL((k_greedy<decltype(dt)::value>), grid, dim3(kThreads), 0, st, p);
    });
    return launch_status();
}
