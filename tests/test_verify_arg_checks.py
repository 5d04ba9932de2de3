"""Which argument error the verify, lm_head and linear entry points report, in which order, and what their size queries answer.

Every call below is REJECTED BEFORE ANY LAUNCH (or returns ASD_OK early on an empty batch), so no GPU is needed -- and none
is allowed: the pointers are made-up addresses, and on a machine with a GPU a regression that let one of these calls through
would launch on them.  The expected codes and sizes are the ones the library returned before the host halves of
verify_accept.hip and lm_head_verify.hip were put on the shared launch helpers; a case with two faults pins which of them is
reported.  (The entropy route takes no options through the ABI: its "forced geometry" is the one asd_verify_accept_stats
sets itself, which a 4 MiB row does not fit.)"""
import ctypes as C

import pytest

OK, INVALID, UNSUPPORTED, WORKSPACE, ALIGNMENT = 0, -1, -2, -3, -5
NAN, INF = float("nan"), float("inf")
F32, BF16, F16, BAD_DTYPE = 0, 1, 2, 7
V = 1024                    # 2 KB bf16 rows
LONG_V = 1 << 20            # a 2 MiB bf16 row: 1025 tiles of 2 KiB, one more than a slice has LDS slots for
A = [0x7F0000000000 + (i << 24) for i in range(20)]      # made-up, 256-byte aligned "device" addresses

# ---- the arguments of a valid call of each family (it would launch: every case below breaks at least one of them)
VERIFY = dict(logits=A[0], dtype=BF16, ld=V, tok=A[1], lp_draft=A[2], u=A[3], B=4, K=4, V=V, lp_target=A[4], accept=A[5],
              n_acc=A[6], accept_bits=A[7], row_max_lp=A[8], row_entropy=None, workspace=A[9], workspace_bytes=1 << 30,
              inv_temperature=1.0, opt=None, feat=A[10], ldf=64, stats_col=5, packed_w=A[11], in_dim=64, hidden=32, risk=1,
              n_obs=100, alpha=1.0, beta=1.0, p_hist=A[12], C=A[13], lam=1.0, L=3, stage_idx=0, prefix_rule=0, theta=None,
              score=A[14], k_star=A[15], stop=A[16], thr_stop=None, stats=None, v_offset=0, msg=A[17], msg_all=A[18],
              n_shards=2, stream=None)
HEAD_V, HEAD_D = 4096, 256
HEAD = dict(hidden=A[0], ld_h=HEAD_D, weight=A[1], ld_w=HEAD_D, dtype=BF16, D=HEAD_D, tok=A[2], lp_draft=A[3], u=A[4], B=4,
            K=4, V=HEAD_V, v_offset=0, inv_temperature=1.0, greedy=0, lp_target=A[5], accept=A[6], n_acc=A[7],
            accept_bits=A[8], argmax_out=None, msg=A[9], workspace=A[10], workspace_bytes=1 << 30, packed=A[11],
            packed_bytes=1 << 30, stream=None)
LIN_M, LIN_N, LIN_D = 32, 4608, 3584        # the 7B qkv projection at 32 rows: a sliced plan (it needs the workspace)
LINEAR = dict(x=A[0], ld_x=LIN_D, w=A[1], ld_w=LIN_D, bias=None, residual=None, ld_res=0, dtype=BF16, M=LIN_M, N=LIN_N,
              D=LIN_D, y=A[2], ld_y=LIN_N, workspace=A[3], workspace_bytes=1 << 30, k_slices="host int", stream=None)

# ---- entry point -> (defaults, the names of its arguments in ABI order)
_VA = ["logits", "dtype", "ld", "tok", "lp_draft", "u", "B", "K", "V", "lp_target", "accept", "n_acc", "accept_bits"]
_W = ["workspace", "workspace_bytes"]
_EPI = ["feat", "ldf", "stats_col", "packed_w", "in_dim", "hidden", "risk", "n_obs", "alpha", "beta", "p_hist", "C", "lam", "L",
        "stage_idx", "prefix_rule", "theta", "score", "k_star", "stop", "thr_stop", "stats"]
_LH = ["hidden", "ld_h", "weight", "ld_w", "dtype", "D", "tok"]
_LHO = ["lp_target", "accept", "n_acc", "accept_bits"]
_LIN = ["dtype", "M", "N", "D", "y", "ld_y"] + _W
ENTRY = {
    "asd_verify_accept": (VERIFY, _VA + _W + ["stream"]),
    "asd_verify_accept_ex": (VERIFY, _VA + _W + ["opt", "stream"]),
    "asd_verify_accept_stats": (VERIFY, _VA + ["row_max_lp", "row_entropy"] + _W + ["inv_temperature", "stream"]),
    "asd_verify_accept_fused": (VERIFY, _VA + _W + _EPI + ["stream"]),
    "asd_verify_accept_fused_ex": (VERIFY, _VA + _W + _EPI + ["opt", "stream"]),
    "asd_lse_partial": (VERIFY, ["logits", "dtype", "ld", "tok", "B", "K", "V", "v_offset", "inv_temperature", "msg"] + _W + ["stream"]),
    "asd_accept_from_partials": (VERIFY, ["msg_all", "n_shards", "lp_draft", "u", "B", "K", "inv_temperature", "lp_target",
                                          "accept", "n_acc", "accept_bits", "stream"]),
    "asd_lm_head_verify": (HEAD, _LH + ["lp_draft", "u", "B", "K", "V", "inv_temperature"] + _LHO + _W + ["stream"]),
    "asd_lm_head_verify_ex": (HEAD, _LH + ["lp_draft", "u", "B", "K", "V", "inv_temperature", "greedy"] + _LHO + ["argmax_out"] + _W + ["stream"]),
    "asd_lm_head_partial": (HEAD, _LH + ["B", "K", "V", "v_offset", "inv_temperature", "msg"] + _W + ["stream"]),
    "asd_lm_head_pack_weights": (HEAD, ["weight", "ld_w", "dtype", "V", "D", "packed", "packed_bytes", "stream"]),
    "asd_linear": (LINEAR, ["x", "ld_x", "w", "ld_w", "bias"] + _LIN + ["stream"]),
    "asd_linear_ex": (LINEAR, ["x", "ld_x", "w", "ld_w", "bias", "residual", "ld_res"] + _LIN + ["stream"]),
    "asd_linear_partial": (LINEAR, ["x", "ld_x", "w", "ld_w", "bias", "residual", "ld_res"] + _LIN + ["stream", "k_slices"]),
}
PLAIN = ("asd_verify_accept", "asd_verify_accept_ex")
STATS = ("asd_verify_accept_stats",)
FUSED = ("asd_verify_accept_fused", "asd_verify_accept_fused_ex")
ACCEPTS = PLAIN + STATS + FUSED                                  # the five entries that run the acceptance test
WITH_OPT = ("asd_verify_accept_ex", "asd_verify_accept_fused_ex")
LSE = ("asd_lse_partial",)
STREAMS = ACCEPTS + LSE                                          # everything that goes through launch_verify
FROM_PARTIALS = ("asd_accept_from_partials",)
HEAD_VERIFY = ("asd_lm_head_verify", "asd_lm_head_verify_ex")
HEAD_PARTIAL = ("asd_lm_head_partial",)
HEADS = HEAD_VERIFY + HEAD_PARTIAL
PACK = ("asd_lm_head_pack_weights",)
LINEAR_RES = ("asd_linear_ex", "asd_linear_partial")            # the entries that take residual / ld_res
LINEARS = ("asd_linear",) + LINEAR_RES
# sentinels for workspace_bytes / packed_bytes, resolved through the library's own size queries for the case's shape
WS_QUERY_LESS_1 = "query-1"

BIG_B = dict(B=1 << 26, K=64)                                    # B K = 2^32 rows
NOT_IN_KERNEL = dict(in_dim=128, hidden=64, ldf=128)             # a predictor shape the fused entries run as two launches


def opt(inv_temperature=1.0, splits=0, threads=0, unroll=0, nontemporal=-1):
    return dict(inv_temperature=inv_temperature, splits=splits, threads=threads, unroll=unroll, nontemporal=nontemporal)


# (entry points, what the call changes, the code it must return)
CASES = [
    # ---- everything that goes through launch_verify: sizes, then the empty batch, then K, dtype, pointers, strides, alignment
    (STREAMS, dict(B=-1), INVALID),
    (STREAMS, dict(K=-1), INVALID),
    (STREAMS, dict(V=-1, ld=-1), INVALID),
    (STREAMS, dict(B=-1, K=0), INVALID),                                     # negative sizes before the empty-batch return
    (STREAMS, dict(B=0, V=-1, ld=-1), INVALID),
    (STREAMS, dict(B=0), OK),
    (STREAMS, dict(K=0), OK),
    (STREAMS, dict(B=0, K=65, dtype=BAD_DTYPE, logits=None, workspace=None), OK),   # the empty batch before K > 64
    (STREAMS, dict(K=65), UNSUPPORTED),
    (STREAMS, dict(K=65, dtype=BAD_DTYPE), UNSUPPORTED),
    (STREAMS, dict(K=65, logits=None), UNSUPPORTED),                         # K > 64 before dtype and pointers
    (STREAMS, dict(dtype=BAD_DTYPE), UNSUPPORTED),
    (STREAMS, dict(dtype=BAD_DTYPE, logits=None), UNSUPPORTED),              # dtype before null pointers
    (STREAMS, dict(dtype=BAD_DTYPE, tok=None, workspace=None), UNSUPPORTED),
    (STREAMS, dict(logits=None), INVALID),
    (STREAMS, dict(tok=None), INVALID),
    (STREAMS, dict(workspace=None), INVALID),
    (STREAMS, dict(workspace=None, logits=A[0] + 1), INVALID),               # null pointers before alignment
    (STREAMS, dict(ld=V - 8), INVALID),                                      # ld < V
    (STREAMS, dict(ld=V - 8, logits=A[0] + 1), INVALID),
    (STREAMS, dict(logits=A[0] + 1), ALIGNMENT),                             # operand alignment: the element size
    (STREAMS, dict(logits=A[0] + 2, dtype=F32), ALIGNMENT),
    (STREAMS, dict(logits=A[0] + 1, workspace=A[9] + 16), ALIGNMENT),        # ... before the workspace's
    (STREAMS, dict(workspace=A[9] + 16), WORKSPACE),                         # workspace alignment is reported as WORKSPACE
    (STREAMS, dict(workspace=A[9] + 16, **BIG_B), WORKSPACE),                # ... before the row count
    (STREAMS, dict(workspace=A[9] + 128, workspace_bytes=0), WORKSPACE),
    (STREAMS, BIG_B, UNSUPPORTED),                                           # B K > INT32_MAX
    (STREAMS, dict(B=1 << 28, K=16), UNSUPPORTED),                           # (K <= 16: the fused entries' one-launch route)
    (STREAMS, dict(workspace_bytes=0, **BIG_B), UNSUPPORTED),                # ... before the workspace size
    (STREAMS, dict(workspace_bytes=0), WORKSPACE),
    (STREAMS, dict(workspace_bytes=255), WORKSPACE),
    (STREAMS, dict(workspace_bytes=0, dtype=F16), WORKSPACE),
    (STREAMS, dict(workspace_bytes=0, K=64, B=2), WORKSPACE),
    # ---- the five acceptance entries: lp_draft / u / outputs are tested at the entry, before anything else
    (ACCEPTS, dict(lp_draft=None), INVALID),
    (ACCEPTS, dict(u=None), INVALID),
    (ACCEPTS, dict(lp_target=None), INVALID),
    (ACCEPTS, dict(accept=None), INVALID),
    (ACCEPTS, dict(n_acc=None), INVALID),
    (ACCEPTS, dict(lp_draft=None, K=65), INVALID),
    (ACCEPTS, dict(u=None, dtype=BAD_DTYPE), INVALID),
    (ACCEPTS, dict(n_acc=None, **BIG_B), INVALID),
    (ACCEPTS, dict(lp_draft=None, u=None, lp_target=None, accept=None, n_acc=None, B=0), OK),
    (ACCEPTS, dict(lp_draft=None, K=0), OK),
    (ACCEPTS, dict(lp_draft=None, B=-1), INVALID),
    # ---- options (asd_verify_options / the inv_temperature argument): after the entry's null checks, before launch_verify
    (WITH_OPT, dict(opt=opt(inv_temperature=0.0)), INVALID),
    (WITH_OPT, dict(opt=opt(inv_temperature=-1.0)), INVALID),
    (WITH_OPT, dict(opt=opt(inv_temperature=INF)), INVALID),
    (WITH_OPT, dict(opt=opt(inv_temperature=NAN)), INVALID),
    (WITH_OPT, dict(opt=opt(inv_temperature=0.0), K=65), INVALID),           # (K = 65 alone: UNSUPPORTED)
    (WITH_OPT, dict(opt=opt(inv_temperature=NAN), dtype=BAD_DTYPE), INVALID),
    (WITH_OPT, dict(opt=opt(inv_temperature=0.0), B=0), INVALID),            # ... and before the empty-batch return
    (WITH_OPT, dict(opt=opt(inv_temperature=0.0), lp_draft=None), INVALID),
    (WITH_OPT, dict(opt=opt(), B=0), OK),
    (WITH_OPT, dict(opt=opt(inv_temperature=0.5), K=65), UNSUPPORTED),
    (STATS + LSE, dict(inv_temperature=0.0), INVALID),
    (STATS + LSE, dict(inv_temperature=INF), INVALID),
    (STATS + LSE, dict(inv_temperature=NAN), INVALID),
    (STATS + LSE, dict(inv_temperature=0.0, K=65), INVALID),
    (STATS + LSE, dict(inv_temperature=0.0, B=0), INVALID),
    (STATS + LSE, dict(inv_temperature=NAN, B=-1), INVALID),
    # ---- forced geometry
    (WITH_OPT, dict(opt=opt(splits=65)), UNSUPPORTED),                       # splits above max_splits_for(K): K = 4 -> 64
    (WITH_OPT, dict(opt=opt(splits=33), K=32), UNSUPPORTED),                 # K = 32 -> 32
    (WITH_OPT, dict(opt=opt(splits=17), K=64, B=2), UNSUPPORTED),            # K = 64 -> 16
    (WITH_OPT, dict(opt=opt(splits=65), workspace_bytes=0), UNSUPPORTED),    # ... before the workspace size
    (WITH_OPT, dict(opt=opt(splits=65), workspace=A[9] + 16), WORKSPACE),    # ... after the workspace alignment
    (WITH_OPT, dict(opt=opt(splits=65), **BIG_B), UNSUPPORTED),
    (WITH_OPT, dict(opt=opt(splits=1, unroll=2), V=LONG_V, ld=LONG_V), UNSUPPORTED),        # more tiles than LDS slots
    (WITH_OPT, dict(opt=opt(splits=1, unroll=2), V=LONG_V // 2, ld=LONG_V // 2, dtype=F32), UNSUPPORTED),
    (WITH_OPT, dict(opt=opt(splits=1, unroll=2), V=LONG_V, ld=LONG_V, workspace_bytes=0), UNSUPPORTED),
    (WITH_OPT, dict(opt=opt(splits=1, unroll=3), V=2 * LONG_V, ld=2 * LONG_V), UNSUPPORTED),
    (WITH_OPT, dict(opt=opt(splits=64), workspace_bytes=WS_QUERY_LESS_1), WORKSPACE),       # the query sizes for the most splits
    (WITH_OPT, dict(opt=opt(splits=1), workspace_bytes=3583), WORKSPACE),                   # 2560 ticket bytes + 4 x 256
    (WITH_OPT, dict(opt=opt(splits=2), workspace_bytes=3583), WORKSPACE),
    (WITH_OPT, dict(opt=opt(splits=64), V=1 << 26, ld=1 << 26), UNSUPPORTED),               # V x splits > INT32_MAX
    (WITH_OPT, dict(opt=opt(splits=64), V=1 << 26, ld=1 << 26, workspace_bytes=0), WORKSPACE),
    (WITH_OPT, dict(opt=opt(threads=128)), UNSUPPORTED),                     # no such instantiation (the fused entries: via _ex)
    (WITH_OPT, dict(opt=opt(threads=768)), UNSUPPORTED),
    (WITH_OPT, dict(opt=opt(threads=128), workspace_bytes=0), WORKSPACE),
    (("asd_verify_accept_ex",), dict(opt=opt(unroll=5)), UNSUPPORTED),
    (("asd_verify_accept_ex",), dict(opt=opt(unroll=1)), UNSUPPORTED),
    (("asd_verify_accept_ex",), dict(opt=opt(threads=512, unroll=16, nontemporal=0)), UNSUPPORTED),
    # ---- the entropy route of asd_verify_accept_stats: one workgroup per row at its own geometry, K <= 32
    (STATS, dict(row_entropy=A[19], K=33), UNSUPPORTED),
    (STATS, dict(row_entropy=A[19], K=64, B=2), UNSUPPORTED),
    (STATS, dict(row_entropy=A[19], K=33, workspace_bytes=0), WORKSPACE),
    (STATS, dict(row_entropy=A[19], K=33, logits=None), INVALID),
    (STATS, dict(row_entropy=A[19], V=2 * LONG_V, ld=2 * LONG_V), UNSUPPORTED),   # its geometry is not widened for a long row
    (STATS, dict(row_entropy=A[19], workspace_bytes=0), WORKSPACE),
    (STATS, dict(row_entropy=A[19], B=0), OK),
    # ---- the fused entries: their own checks come first, ahead of the options, launch_verify and the two-launch fall-back
    (FUSED, dict(L=0), INVALID),
    (FUSED, dict(stage_idx=-1), INVALID),
    (FUSED, dict(stage_idx=3), INVALID),
    (FUSED, dict(L=17), UNSUPPORTED),
    (FUSED, dict(L=17, stage_idx=17), INVALID),
    (FUSED, dict(L=0, K=65), INVALID),
    (FUSED, dict(L=17, B=-1), UNSUPPORTED),
    (FUSED, dict(L=17, B=0), UNSUPPORTED),
    (FUSED, dict(L=17, lp_draft=None), INVALID),
    (FUSED, dict(L=17, feat=None), UNSUPPORTED),
    (FUSED, dict(L=16, stage_idx=15, K=65), UNSUPPORTED),
    (FUSED, dict(feat=None), INVALID),
    (FUSED, dict(packed_w=None), INVALID),
    (FUSED, dict(ldf=63), INVALID),
    (FUSED, dict(feat=None, K=65), INVALID),
    (FUSED, dict(feat=None, dtype=BAD_DTYPE), INVALID),
    (FUSED, dict(feat=None, packed_w=None, ldf=0, B=0), OK),
    (FUSED, dict(feat=None, K=0), INVALID),
    (FUSED, dict(stats_col=60), INVALID),
    (FUSED, dict(stats_col=60, B=0), INVALID),
    (FUSED, dict(stats_col=60, K=65), INVALID),
    (FUSED, dict(stats_col=-1, K=65), UNSUPPORTED),
    (FUSED, dict(p_hist=None), INVALID),
    (FUSED, dict(C=None), INVALID),
    (FUSED, dict(p_hist=None, k_star=None), INVALID),
    (FUSED, dict(p_hist=None, stop=None), INVALID),
    (FUSED, dict(p_hist=None, B=0), INVALID),
    (FUSED, dict(p_hist=None, K=65), INVALID),
    (FUSED, dict(p_hist=None, C=None, k_star=None, stop=None, K=65), UNSUPPORTED),
    (("asd_verify_accept_fused_ex",), dict(p_hist=None, opt=opt(splits=65)), INVALID),
    (("asd_verify_accept_fused_ex",), dict(L=17, opt=opt(inv_temperature=0.0)), UNSUPPORTED),
    (("asd_verify_accept_fused_ex",), dict(opt=opt(inv_temperature=0.0), **NOT_IN_KERNEL), INVALID),
    # two launches: asd_verify_accept_ex's codes, then asd_predictor_stop's
    (FUSED, dict(K=65, **NOT_IN_KERNEL), UNSUPPORTED),
    (FUSED, dict(L=0, **NOT_IN_KERNEL), INVALID),
    (FUSED, dict(B=0, **NOT_IN_KERNEL), OK),
    (FUSED, dict(workspace=None, **NOT_IN_KERNEL), INVALID),
    (FUSED, dict(workspace_bytes=0, **NOT_IN_KERNEL), WORKSPACE),
    (FUSED, dict(B=0, L=5, stage_idx=4), OK),
    (FUSED, dict(B=0, in_dim=2048, hidden=32), UNSUPPORTED),                 # (asd_predictor_stop's own: no such predictor)
    (FUSED, dict(B=-1, in_dim=2048, hidden=32), INVALID),
    (FUSED, dict(in_dim=256, hidden=128, ldf=256, logits=None), INVALID),    # (16 rows < CUs: two launches)
    (FUSED, dict(in_dim=256, hidden=128, ldf=256, B=64, logits=A[0] + 1), ALIGNMENT),   # (256 rows: one launch)
    (FUSED, dict(in_dim=256, hidden=128, ldf=256, B=64, workspace_bytes=0), WORKSPACE),
    # ---- asd_lse_partial's own
    (LSE, dict(msg=None), INVALID),
    (LSE, dict(msg=None, K=65), INVALID),
    (LSE, dict(msg=None, B=0), OK),
    (LSE, dict(msg=None, B=-1), INVALID),
    (LSE, dict(v_offset=1 << 40, K=65), UNSUPPORTED),
    # ---- asd_accept_from_partials
    (FROM_PARTIALS, dict(B=-1), INVALID),
    (FROM_PARTIALS, dict(K=-1), INVALID),
    (FROM_PARTIALS, dict(n_shards=0), INVALID),
    (FROM_PARTIALS, dict(n_shards=0, B=0), INVALID),
    (FROM_PARTIALS, dict(inv_temperature=0.0), INVALID),
    (FROM_PARTIALS, dict(inv_temperature=INF), INVALID),
    (FROM_PARTIALS, dict(inv_temperature=NAN), INVALID),
    (FROM_PARTIALS, dict(inv_temperature=0.0, B=0), INVALID),
    (FROM_PARTIALS, dict(inv_temperature=0.0, K=65), INVALID),
    (FROM_PARTIALS, dict(B=0), OK),
    (FROM_PARTIALS, dict(K=0, msg_all=None, lp_draft=None, u=None, lp_target=None, accept=None, n_acc=None), OK),
    (FROM_PARTIALS, dict(B=0, K=65), OK),
    (FROM_PARTIALS, dict(K=65), UNSUPPORTED),
    (FROM_PARTIALS, dict(K=65, msg_all=None), UNSUPPORTED),
    (FROM_PARTIALS, dict(msg_all=None), INVALID),
    (FROM_PARTIALS, dict(lp_draft=None), INVALID),
    (FROM_PARTIALS, dict(u=None), INVALID),
    (FROM_PARTIALS, dict(lp_target=None), INVALID),
    (FROM_PARTIALS, dict(accept=None), INVALID),
    (FROM_PARTIALS, dict(n_acc=None), INVALID),
    # ---- asd_lm_head_verify, _ex, asd_lm_head_partial
    (HEADS, dict(B=-1), INVALID),
    (HEADS, dict(K=-1), INVALID),
    (HEADS, dict(V=0), INVALID),
    (HEADS, dict(D=0, ld_h=0, ld_w=0), INVALID),
    (HEADS, dict(B=-1, K=0), INVALID),
    (HEADS, dict(inv_temperature=0.0), INVALID),
    (HEADS, dict(inv_temperature=INF), INVALID),
    (HEADS, dict(inv_temperature=NAN), INVALID),
    (HEADS, dict(inv_temperature=0.0, B=0), INVALID),                        # the temperature before the empty-batch return
    (HEADS, dict(inv_temperature=0.0, K=65), INVALID),
    (HEADS, dict(B=0), OK),
    (HEADS, dict(K=0), OK),
    (HEADS, dict(B=0, K=65, dtype=F32, hidden=None, workspace=None), OK),
    (HEADS, dict(K=65), UNSUPPORTED),
    (HEADS, dict(K=65, dtype=F32), UNSUPPORTED),
    (HEADS, dict(K=65, hidden=None), UNSUPPORTED),
    (HEADS, dict(dtype=F32), UNSUPPORTED),
    (HEADS, dict(dtype=BAD_DTYPE), UNSUPPORTED),
    (HEADS, dict(D=200, ld_h=200, ld_w=200), UNSUPPORTED),
    (HEADS, dict(dtype=F32, hidden=None), UNSUPPORTED),                      # dtype before null pointers
    (HEADS, dict(D=200, ld_h=200, ld_w=200, tok=None), UNSUPPORTED),
    (HEADS, dict(hidden=None), INVALID),
    (HEADS, dict(weight=None), INVALID),
    (HEADS, dict(tok=None), INVALID),
    (HEADS, dict(hidden=None, workspace=None), INVALID),
    (HEADS, dict(ld_h=HEAD_D - 8), INVALID),
    (HEADS, dict(ld_w=HEAD_D - 8), INVALID),
    (HEADS, dict(ld_h=HEAD_D - 8, hidden=A[0] + 8), INVALID),
    (HEADS, dict(hidden=A[0] + 8), ALIGNMENT),
    (HEADS, dict(weight=A[1] + 8), ALIGNMENT),
    (HEADS, dict(ld_h=HEAD_D + 4), ALIGNMENT),
    (HEADS, dict(ld_w=HEAD_D + 4), ALIGNMENT),
    (HEADS, dict(hidden=A[0] + 8, workspace=None), ALIGNMENT),               # operands before the workspace
    (HEADS, dict(workspace=None), WORKSPACE),
    (HEADS, dict(workspace_bytes=0), WORKSPACE),
    (HEADS, dict(workspace_bytes=WS_QUERY_LESS_1), WORKSPACE),
    (HEADS, dict(workspace_bytes=WS_QUERY_LESS_1, workspace=A[10] + 8), WORKSPACE),     # size before alignment
    (HEADS, dict(workspace=A[10] + 8), ALIGNMENT),
    (HEADS, dict(ld_w=0, workspace=None), WORKSPACE),                        # (ld_w = 0: a packed image, a valid stride)
    (HEADS, dict(workspace_bytes=0, **BIG_B), WORKSPACE),
    (HEADS, dict(workspace_bytes=1 << 62, **BIG_B), UNSUPPORTED),            # B K >= 2^31, behind the workspace checks
    (HEAD_VERIFY, dict(lp_target=None), INVALID),
    (HEAD_VERIFY, dict(accept=None), INVALID),
    (HEAD_VERIFY, dict(n_acc=None), INVALID),
    (HEAD_VERIFY, dict(lp_draft=None), INVALID),
    (HEAD_VERIFY, dict(u=None), INVALID),
    (HEAD_VERIFY, dict(lp_target=None, dtype=F32), UNSUPPORTED),
    (HEAD_VERIFY, dict(lp_target=None, ld_h=HEAD_D - 8), INVALID),
    (HEAD_VERIFY, dict(lp_draft=None, hidden=A[0] + 8), INVALID),
    (("asd_lm_head_verify_ex",), dict(greedy=1, lp_draft=None, u=None, workspace=None), WORKSPACE),   # greedy needs neither
    (("asd_lm_head_verify_ex",), dict(greedy=1, lp_target=None), INVALID),
    (HEAD_PARTIAL, dict(msg=None), INVALID),
    (HEAD_PARTIAL, dict(msg=None, K=65), INVALID),
    (HEAD_PARTIAL, dict(msg=None, B=0), OK),
    (HEAD_PARTIAL, dict(v_offset=-1), INVALID),
    (HEAD_PARTIAL, dict(v_offset=-1, B=0), INVALID),
    (HEAD_PARTIAL, dict(v_offset=(1 << 31) - HEAD_V), UNSUPPORTED),
    (HEAD_PARTIAL, dict(v_offset=(1 << 31) - HEAD_V, hidden=None), UNSUPPORTED),
    (HEAD_PARTIAL, dict(v_offset=(1 << 31) - HEAD_V - 1, workspace=None), WORKSPACE),
    # ---- asd_lm_head_pack_weights
    (PACK, dict(V=0), INVALID),
    (PACK, dict(D=0, ld_w=0), INVALID),
    (PACK, dict(weight=None), INVALID),
    (PACK, dict(packed=None), INVALID),
    (PACK, dict(ld_w=HEAD_D - 8), INVALID),
    (PACK, dict(ld_w=0), INVALID),
    (PACK, dict(V=0, dtype=F32), INVALID),
    (PACK, dict(dtype=F32), UNSUPPORTED),
    (PACK, dict(D=200, ld_w=200), UNSUPPORTED),
    (PACK, dict(dtype=F32, weight=A[1] + 8), UNSUPPORTED),
    (PACK, dict(weight=A[1] + 8), ALIGNMENT),
    (PACK, dict(packed=A[11] + 8), ALIGNMENT),
    (PACK, dict(ld_w=HEAD_D + 4), ALIGNMENT),
    (PACK, dict(weight=A[1] + 8, packed_bytes=0), ALIGNMENT),
    (PACK, dict(packed_bytes=0), WORKSPACE),
    (PACK, dict(packed_bytes=WS_QUERY_LESS_1), WORKSPACE),
    # ---- asd_linear, _ex, _partial
    (LINEARS, dict(M=-1), INVALID),
    (LINEARS, dict(N=0, ld_y=0), INVALID),
    (LINEARS, dict(D=0, ld_x=0, ld_w=0), INVALID),
    (LINEARS, dict(M=-1, dtype=F32), INVALID),
    (LINEARS, dict(M=0), OK),
    (LINEARS, dict(M=0, dtype=F32, x=None, w=None, y=None, workspace=None), OK),
    (LINEARS, dict(dtype=F32), UNSUPPORTED),
    (LINEARS, dict(dtype=BAD_DTYPE), UNSUPPORTED),
    (LINEARS, dict(D=200, ld_x=200, ld_w=200), UNSUPPORTED),
    (LINEARS, dict(N=LIN_N + 2, ld_y=LIN_N + 4), UNSUPPORTED),
    (LINEARS, dict(dtype=F32, x=None), UNSUPPORTED),
    (LINEARS, dict(x=None), INVALID),
    (LINEARS, dict(w=None), INVALID),
    (LINEARS, dict(y=None), INVALID),
    (LINEARS, dict(ld_x=LIN_D - 8), INVALID),
    (LINEARS, dict(ld_w=LIN_D - 8), INVALID),
    (LINEARS, dict(ld_y=LIN_N - 4), INVALID),
    (LINEARS, dict(x=None, w=A[1] + 8), INVALID),
    (LINEARS, dict(x=A[0] + 8), ALIGNMENT),
    (LINEARS, dict(w=A[1] + 8), ALIGNMENT),
    (LINEARS, dict(y=A[2] + 4), ALIGNMENT),
    (LINEARS, dict(bias=A[4] + 4), ALIGNMENT),
    (LINEARS, dict(ld_x=LIN_D + 4), ALIGNMENT),
    (LINEARS, dict(ld_w=LIN_D + 4), ALIGNMENT),
    (LINEARS, dict(ld_y=LIN_N + 2), ALIGNMENT),
    (LINEARS, dict(x=A[0] + 8, workspace=None), ALIGNMENT),
    (LINEARS, dict(workspace=None), WORKSPACE),                              # (a sliced plan: it needs the workspace)
    (LINEARS, dict(workspace_bytes=0), WORKSPACE),
    (LINEARS, dict(workspace_bytes=WS_QUERY_LESS_1), WORKSPACE),
    (LINEARS, dict(workspace_bytes=WS_QUERY_LESS_1, workspace=A[3] + 8), WORKSPACE),
    (LINEARS, dict(workspace=A[3] + 8), ALIGNMENT),
    (LINEARS, dict(ld_w=0, workspace=None), WORKSPACE),
    # the ld_res pair: a short stride is INVALID_ARG, a misaligned one (or a misaligned pointer) ALIGNMENT -- ahead of the rest
    (LINEAR_RES, dict(residual=A[5], ld_res=LIN_N - 4), INVALID),
    (LINEAR_RES, dict(residual=A[5], ld_res=LIN_N + 2), ALIGNMENT),
    (LINEAR_RES, dict(residual=A[5] + 4, ld_res=LIN_N), ALIGNMENT),
    (LINEAR_RES, dict(residual=A[5] + 4, ld_res=LIN_N - 4), INVALID),
    (LINEAR_RES, dict(residual=A[5] + 4, ld_res=LIN_N - 2), INVALID),
    (LINEAR_RES, dict(residual=A[5], ld_res=LIN_N - 4, M=0), INVALID),       # ... and of the empty-batch return
    (LINEAR_RES, dict(residual=A[5], ld_res=LIN_N + 2, M=0), ALIGNMENT),
    (LINEAR_RES, dict(residual=A[5], ld_res=LIN_N + 2, dtype=F32), ALIGNMENT),
    (LINEAR_RES, dict(residual=A[5], ld_res=LIN_N - 4, M=-1), INVALID),
    (LINEAR_RES, dict(residual=A[5], ld_res=LIN_N + 2, M=-1), INVALID),
    (LINEAR_RES, dict(residual=None, ld_res=-1, M=0), OK),
    (LINEAR_RES, dict(residual=A[5], ld_res=LIN_N, workspace=None), WORKSPACE),
    (("asd_linear_partial",), dict(k_slices=None), INVALID),
    (("asd_linear_partial",), dict(k_slices=None, M=0), INVALID),
    (("asd_linear_partial",), dict(k_slices=None, M=-1), INVALID),
    (("asd_linear_partial",), dict(k_slices=None, dtype=F32), INVALID),
]

# ---- the pure size queries (256 CUs)
MS = (1, 32, 64, 65, 128, 256, 272, 288, 512)
VERIFY_WS = {      # (B, K) -> asd_verify_accept_workspace_bytes
    (1, 1): 1280, (1, 4): 2816, (8, 4): 21504, (32, 4): 86016, (64, 8): 303104, (33, 16): 291584, (4, 32): 35328, (2, 64): 17664,
    (128, 5): 409600,
}
LM_HEAD_WS = {     # V -> asd_lm_head_verify_workspace_bytes(M, 1, V) for M in MS
    152064: [67136768, 67873280, 68633600, 68657408, 70154240, 73195520, 73575680, 73955840, 79278080],
    4096: [67113728, 67133440, 67153920, 67154688, 67194880, 67276800, 67287040, 67297280, 67440640],
}
PACKED = {(152064, 3584): 1089994752, (152064, 8192): 2491416576, (4096, 256): 2097152, (1000, 128): 262144, (1000, 100): 0}
LINEAR_PLAN = {    # (N, D) of the 7B qkv, down, gate|up, the 32B o and the 72B down projections -> [(slices, workspace bytes) for M in MS]
    (4608, 3584): [(8, 147712), (8, 4718848), (8, 9437440), (8, 9584896), (8, 18874624), (8, 37748992), (8, 40108288), (8, 42467584), (7, 66060544)],
    (3584, 18944): [(18, 258304), (18, 8257792), (18, 16515328), (18, 16773376), (18, 33030400), (18, 66060544), (18, 70189312), (18, 74318080), (9, 66060544)],
    (37888, 3584): [(1, 256), (1, 256), (1, 256), (3, 29552896), (3, 58196224), (3, 116392192), (3, 123666688), (1, 256), (1, 256)],
    (5120, 5120): [(10, 205056), (10, 6553856), (10, 13107456), (10, 13312256), (10, 26214656), (10, 52429056), (10, 55705856), (10, 58982656), (6, 62914816)],
    (8192, 29568): [(8, 262400), (8, 8388864), (8, 16777472), (8, 17039616), (8, 33554688), (8, 67109120), (8, 71303424), (8, 75497728), (4, 67109120)],
}


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: these calls carry made-up device addresses, and the sizes below are those of 256 CUs")
    from asd_amd import _binding
    return _binding, _binding.load_library()


def _query_less_1(lib, name, a):
    """The size the library's own query asks for the case's shape, less one byte."""
    if name.startswith("asd_verify") or name == "asd_lse_partial":
        return lib.asd_verify_accept_workspace_bytes(a["B"], a["K"], a["V"], a["dtype"]) - 1
    if name == "asd_lm_head_pack_weights":
        return lib.asd_lm_head_packed_bytes(a["V"], a["D"]) - 1
    if name.startswith("asd_lm_head"):
        return lib.asd_lm_head_verify_workspace_bytes(a["B"], a["K"], a["V"]) - 1
    slices = lib.asd_linear_slices(a["M"], a["N"], a["D"])
    assert slices > 1                          # the slabs: [slices][M][N] f32 (the query rounds up and adds a block)
    return slices * a["M"] * a["N"] * 4 - 1


def test_rejected_calls_return_the_same_code_in_the_same_order():
    binding, lib = _no_gpu()
    wrong, n, keep = [], 0, []
    for entries, change, want in CASES:
        for name in entries:
            defaults, order = ENTRY[name]
            args = dict(defaults, **change)
            for size in ("workspace_bytes", "packed_bytes"):
                if args.get(size) == WS_QUERY_LESS_1:
                    args[size] = _query_less_1(lib, name, args)
            if isinstance(args.get("opt"), dict):
                keep.append(binding.verify_options(**args["opt"]))
                args["opt"] = C.addressof(keep[-1])
            if args.get("k_slices") == "host int":             # asd_linear_partial writes the slice count through it
                keep.append(C.c_int(-7))
                args["k_slices"] = C.addressof(keep[-1])
            got = getattr(lib, name)(*[args[a] for a in order])
            n += 1
            if got != want:
                shown = {k: v for k, v in change.items() if k in order}
                wrong.append(f"{name}({shown}): returned {got}, expected {want}")
    assert n == sum(len(entries) for entries, _, _ in CASES) == 728
    assert not wrong, "\n".join(wrong)


def test_size_queries_answer_the_same_values():
    _, lib = _no_gpu()
    wrong, n = [], 0

    def expect(what, got, want):
        nonlocal n
        n += 1
        if got != want:
            wrong.append(f"{what}: returned {got}, expected {want}")

    for (B, K), want in VERIFY_WS.items():
        for dtype, V in ((BF16, 152064), (F32, 1000)):                    # (neither enters the size)
            expect(f"asd_verify_accept_workspace_bytes({B}, {K}, {V}, {dtype})", lib.asd_verify_accept_workspace_bytes(B, K, V, dtype), want)
    for B, K in ((0, 4), (4, 0), (-1, 4)):
        expect(f"asd_verify_accept_workspace_bytes({B}, {K})", lib.asd_verify_accept_workspace_bytes(B, K, 1024, BF16), 256)
    for V, row in LM_HEAD_WS.items():
        for M, want in zip(MS, row):
            expect(f"asd_lm_head_verify_workspace_bytes({M}, 1, {V})", lib.asd_lm_head_verify_workspace_bytes(M, 1, V), want)
            if M % 4 == 0:
                expect(f"asd_lm_head_verify_workspace_bytes({M // 4}, 4, {V})", lib.asd_lm_head_verify_workspace_bytes(M // 4, 4, V), want)
    for B, K, V in ((0, 4, 4096), (4, 0, 4096), (4, 4, 0)):
        expect(f"asd_lm_head_verify_workspace_bytes({B}, {K}, {V})", lib.asd_lm_head_verify_workspace_bytes(B, K, V), 0)
    for (V, D), want in PACKED.items():
        expect(f"asd_lm_head_packed_bytes({V}, {D})", lib.asd_lm_head_packed_bytes(V, D), want)
    for (N, D), row in LINEAR_PLAN.items():
        for M, (slices, nbytes) in zip(MS, row):
            expect(f"asd_linear_slices({M}, {N}, {D})", lib.asd_linear_slices(M, N, D), slices)
            expect(f"asd_linear_workspace_bytes({M}, {N}, {D})", lib.asd_linear_workspace_bytes(M, N, D), nbytes)
    for M, N, D in ((0, 4608, 3584), (32, 0, 3584), (32, 4608, 0), (32, 4608, 100)):
        expect(f"asd_linear_slices({M}, {N}, {D})", lib.asd_linear_slices(M, N, D), 0)
        expect(f"asd_linear_workspace_bytes({M}, {N}, {D})", lib.asd_linear_workspace_bytes(M, N, D), 0)
    assert n == 2 * len(VERIFY_WS) + 3 + sum(len(MS) + sum(M % 4 == 0 for M in MS) for _ in LM_HEAD_WS) + 3 + len(PACKED) + \
        2 * len(MS) * len(LINEAR_PLAN) + 8
    assert not wrong, "\n".join(wrong)
