"""Which argument error each of the eight sampling entry points reports, and in which order.

Every call below is REJECTED BEFORE ANY LAUNCH (or returns ASD_OK early on an empty batch), so no GPU is needed -- and none
is allowed: the pointers are made-up addresses, and on a machine with a GPU a regression that let one of these calls through
would launch on them.  The expected codes are the ones the library returned before its plain / top-p / top-k launchers
were folded into one per step; a case with two faults pins which of them is reported."""
import pytest

OK, INVALID, UNSUPPORTED, WORKSPACE, ALIGNMENT = 0, -1, -2, -3, -5
NAN, INF = float("nan"), float("inf")
BF16, F32, BAD_DTYPE = 1, 0, 7
V = 1024                    # 2 KB bf16 rows: 128 whole 16-byte vectors
ODD_V = 1028                # 2056 bytes: not a whole number of 16-byte vectors
LONG_V = 1 << 21            # 4096 tiles of 64 vectors: more than the one-workgroup-per-row kernels hold
A = [0x7F0000000000 + (i << 24) for i in range(12)]      # made-up, 256-byte aligned "device" addresses

# the arguments of a valid call (it would launch: every case below breaks at least one of them)
DRAFT = dict(logits=A[0], ld=V, dtype=BF16, r=A[1], B=4, V=V, inv_temperature=1.0, top_k=0, top_p=0.9, tok=A[2], lp=A[3],
             thr=A[4], workspace=A[5], workspace_bytes=1 << 30, stream=None)
VERIFY = dict(logits=A[0], dtype=BF16, ld=V, tok=A[1], lp_draft=A[2], u=A[3], B=4, K=4, V=V, inv_temperature=1.0, top_k=0,
              top_p=0.9, lp_target=A[4], accept=A[5], n_acc=A[6], accept_bits=A[7], t_nucleus_logit=A[8], n_finite=A[9],
              workspace=A[10], workspace_bytes=1 << 30, stream=None)
RESIDUAL = dict(t=A[0], ld_t=V, d=A[1], ld_d=V, bonus=A[2], ld_b=V, dtype=BF16, n_acc=A[3], r=A[4], B=4, K=4, V=V,
                inv_temperature=1.0, top_k=0, top_p=0.9, t_threshold=A[5], d_threshold=A[6], token=A[7], workspace=A[8],
                workspace_bytes=1 << 30, stream=None)
# entry point -> (defaults, the names of its arguments in ABI order)
_D = ["logits", "ld", "dtype", "r", "B", "V", "inv_temperature"]
_V = ["logits", "dtype", "ld", "tok", "lp_draft", "u", "B", "K", "V", "inv_temperature"]
_VO = ["lp_target", "accept", "n_acc", "accept_bits", "t_nucleus_logit", "n_finite", "workspace", "workspace_bytes", "stream"]
_R = ["t", "ld_t", "d", "ld_d", "bonus", "ld_b", "dtype", "n_acc", "r", "B", "K", "V", "inv_temperature"]
_W = ["workspace", "workspace_bytes", "stream"]
ENTRY = {
    "asd_draft_sample": (DRAFT, _D + ["top_p", "tok", "lp", "thr"] + _W),
    "asd_draft_sample_top_k": (DRAFT, _D + ["top_k", "top_p", "tok", "lp", "thr"] + _W),
    "asd_verify_accept_top_p": (VERIFY, _V + ["top_p"] + _VO),
    "asd_verify_accept_top_k": (VERIFY, _V + ["top_k", "top_p"] + _VO),
    "asd_residual_sample": (RESIDUAL, _R + ["token"] + _W),
    "asd_residual_sample_ex": (RESIDUAL, _R + ["d_threshold", "token"] + _W),
    "asd_residual_sample_top_p": (RESIDUAL, _R + ["top_p", "t_threshold", "d_threshold", "token"] + _W),
    "asd_residual_sample_top_k": (RESIDUAL, _R + ["top_k", "top_p", "t_threshold", "d_threshold", "token"] + _W),
}
DRAFTS = ("asd_draft_sample", "asd_draft_sample_top_k")
VERIFIES = ("asd_verify_accept_top_p", "asd_verify_accept_top_k")
RESIDUALS = ("asd_residual_sample", "asd_residual_sample_ex", "asd_residual_sample_top_p", "asd_residual_sample_top_k")
TRUNCATED = ("asd_residual_sample_top_p", "asd_residual_sample_top_k")      # (the residual entries that take top_p / t_threshold)
# sentinels for workspace_bytes, resolved through the library's own size functions for the case's (B, V, dtype)
PLAIN_WS, PLAIN_WS_LESS_1, TOP_P_WS_LESS_1 = "plain", "plain-1", "top_p-1"

# (entry points, top_k settings tried on the *_top_k entries, what the call changes, the code it must return)
K_ANY = (0, 8, V)           # no bound, a live bound, a bound that bounds nothing
K_LIVE, K_DEAD = (8,), (0, V)
CASES = [
    # ---- asd_draft_sample / asd_draft_sample_top_k
    (DRAFTS, K_ANY, dict(B=-1), INVALID),
    (DRAFTS, K_ANY, dict(V=0, ld=0), INVALID),
    (DRAFTS, K_ANY, dict(B=0), OK),
    (DRAFTS, K_ANY, dict(B=0, dtype=BAD_DTYPE, logits=None, inv_temperature=0.0), OK),
    (DRAFTS, K_ANY, dict(B=0, V=0), INVALID),
    (DRAFTS, K_ANY, dict(dtype=BAD_DTYPE), UNSUPPORTED),
    (DRAFTS, K_ANY, dict(dtype=BAD_DTYPE, logits=None), UNSUPPORTED),
    (DRAFTS, K_ANY, dict(dtype=BAD_DTYPE, B=-1), INVALID),
    (DRAFTS, K_ANY, dict(logits=None), INVALID),
    (DRAFTS, K_ANY, dict(r=None), INVALID),
    (DRAFTS, K_ANY, dict(tok=None), INVALID),
    (DRAFTS, K_ANY, dict(ld=V - 8), INVALID),
    (DRAFTS, K_ANY, dict(inv_temperature=0.0), INVALID),
    (DRAFTS, K_ANY, dict(inv_temperature=-1.0), INVALID),
    (DRAFTS, K_ANY, dict(inv_temperature=INF), INVALID),
    (DRAFTS, K_ANY, dict(inv_temperature=NAN), INVALID),
    (DRAFTS, K_ANY, dict(top_p=NAN), INVALID),
    (DRAFTS, K_ANY, dict(top_p=NAN, V=ODD_V, ld=ODD_V), INVALID),
    (DRAFTS, K_ANY, dict(tok=None, logits=A[0] + 2), INVALID),
    (DRAFTS, K_ANY, dict(V=ODD_V, ld=ODD_V), ALIGNMENT),
    (DRAFTS, K_ANY, dict(logits=A[0] + 2), ALIGNMENT),
    (DRAFTS, K_ANY, dict(ld=V + 4), ALIGNMENT),
    (DRAFTS, K_ANY, dict(top_p=1.0, logits=A[0] + 8), ALIGNMENT),
    (DRAFTS, K_ANY, dict(V=LONG_V, ld=LONG_V), UNSUPPORTED),
    (DRAFTS, K_ANY, dict(V=LONG_V, ld=LONG_V, logits=A[0] + 2), ALIGNMENT),
    (DRAFTS, K_ANY, dict(V=LONG_V // 2, ld=LONG_V // 2, dtype=F32), UNSUPPORTED),
    # ---- asd_verify_accept_top_p / asd_verify_accept_top_k
    (VERIFIES, K_ANY, dict(B=-1), INVALID),
    (VERIFIES, K_ANY, dict(K=-1), INVALID),
    (VERIFIES, K_ANY, dict(V=0, ld=0), INVALID),
    (VERIFIES, K_ANY, dict(B=0), OK),
    (VERIFIES, K_ANY, dict(K=0), OK),
    (VERIFIES, K_ANY, dict(B=0, K=65, dtype=BAD_DTYPE, logits=None), OK),
    (VERIFIES, K_ANY, dict(K=0, V=0), INVALID),
    (VERIFIES, K_ANY, dict(K=65), UNSUPPORTED),
    (VERIFIES, K_ANY, dict(K=65, logits=None), UNSUPPORTED),
    (VERIFIES, K_ANY, dict(dtype=BAD_DTYPE), UNSUPPORTED),
    (VERIFIES, K_ANY, dict(dtype=BAD_DTYPE, tok=None), UNSUPPORTED),
    (VERIFIES, K_ANY, dict(logits=None), INVALID),
    (VERIFIES, K_ANY, dict(tok=None), INVALID),
    (VERIFIES, K_ANY, dict(lp_draft=None), INVALID),
    (VERIFIES, K_ANY, dict(u=None), INVALID),
    (VERIFIES, K_ANY, dict(lp_target=None), INVALID),
    (VERIFIES, K_ANY, dict(accept=None), INVALID),
    (VERIFIES, K_ANY, dict(n_acc=None), INVALID),
    (VERIFIES, K_ANY, dict(ld=V - 8), INVALID),
    (VERIFIES, K_ANY, dict(inv_temperature=0.0), INVALID),
    (VERIFIES, K_ANY, dict(inv_temperature=INF), INVALID),
    (VERIFIES, K_ANY, dict(inv_temperature=NAN), INVALID),
    (VERIFIES, K_ANY, dict(top_p=NAN), INVALID),
    (VERIFIES, K_ANY, dict(top_p=NAN, B=1 << 26, K=64), INVALID),
    (VERIFIES, K_ANY, dict(B=1 << 26, K=64), UNSUPPORTED),
    (VERIFIES, K_ANY, dict(B=1 << 26, K=64, logits=A[0] + 2), UNSUPPORTED),
    (VERIFIES, K_ANY, dict(B=1 << 26, K=64, top_p=1.0, workspace=None), UNSUPPORTED),
    (VERIFIES, K_ANY, dict(V=ODD_V, ld=ODD_V), ALIGNMENT),
    (VERIFIES, K_ANY, dict(logits=A[0] + 2), ALIGNMENT),
    (VERIFIES, K_ANY, dict(ld=V + 4), ALIGNMENT),
    (VERIFIES, K_ANY, dict(V=LONG_V, ld=LONG_V), UNSUPPORTED),
    (VERIFIES, K_ANY, dict(V=LONG_V, ld=LONG_V, logits=A[0] + 2), ALIGNMENT),
    (VERIFIES, K_LIVE, dict(top_p=1.0, V=ODD_V, ld=ODD_V), ALIGNMENT),      # a live top-k alone takes the select's route
    (VERIFIES, K_LIVE, dict(top_p=1.0, V=LONG_V, ld=LONG_V), UNSUPPORTED),
    # nothing to truncate: asd_verify_accept_ex's own checks, behind the ones above
    (VERIFIES, K_DEAD, dict(top_p=1.0, workspace=None), INVALID),
    (VERIFIES, K_DEAD, dict(top_p=0.0, workspace=None), INVALID),
    (VERIFIES, K_DEAD, dict(top_p=1.0, workspace=A[10] + 16), WORKSPACE),
    (VERIFIES, K_DEAD, dict(top_p=1.0, workspace=None, inv_temperature=0.0), INVALID),
    (VERIFIES, K_DEAD, dict(top_p=1.0, workspace=A[10] + 16, dtype=BAD_DTYPE), UNSUPPORTED),
    # ---- asd_residual_sample, _ex, _top_p, _top_k: what residual_launch tests
    (RESIDUALS, K_ANY, dict(B=-1), INVALID),
    (RESIDUALS, K_ANY, dict(K=-1), INVALID),
    (RESIDUALS, K_ANY, dict(V=0, ld_t=0, ld_d=0, ld_b=0), INVALID),
    (RESIDUALS, K_ANY, dict(B=0), OK),
    (RESIDUALS, K_ANY, dict(B=0, dtype=BAD_DTYPE, n_acc=None, workspace=None, t_threshold=None, workspace_bytes=0), OK),
    (RESIDUALS, K_ANY, dict(B=0, K=-1), INVALID),
    (RESIDUALS, K_ANY, dict(dtype=BAD_DTYPE), UNSUPPORTED),
    (RESIDUALS, K_ANY, dict(dtype=BAD_DTYPE, n_acc=None), UNSUPPORTED),
    (RESIDUALS, K_ANY, dict(n_acc=None), INVALID),
    (RESIDUALS, K_ANY, dict(r=None), INVALID),
    (RESIDUALS, K_ANY, dict(token=None), INVALID),
    (RESIDUALS, K_ANY, dict(workspace=None), INVALID),
    (RESIDUALS, K_ANY, dict(workspace=None, workspace_bytes=0), INVALID),
    (RESIDUALS, K_ANY, dict(t=None), INVALID),
    (RESIDUALS, K_ANY, dict(d=None), INVALID),
    (RESIDUALS, K_ANY, dict(ld_t=V - 8), INVALID),
    (RESIDUALS, K_ANY, dict(ld_d=V - 8), INVALID),
    (RESIDUALS, K_ANY, dict(ld_b=V - 8), INVALID),
    (RESIDUALS, K_ANY, dict(inv_temperature=0.0), INVALID),
    (RESIDUALS, K_ANY, dict(inv_temperature=INF), INVALID),
    (RESIDUALS, K_ANY, dict(inv_temperature=NAN), INVALID),
    (RESIDUALS, K_ANY, dict(inv_temperature=0.0, V=ODD_V, ld_t=ODD_V, ld_d=ODD_V, ld_b=ODD_V), INVALID),
    (RESIDUALS, K_ANY, dict(V=ODD_V, ld_t=ODD_V, ld_d=ODD_V, ld_b=ODD_V), ALIGNMENT),
    (RESIDUALS, K_ANY, dict(t=A[0] + 2), ALIGNMENT),
    (RESIDUALS, K_ANY, dict(d=A[1] + 4), ALIGNMENT),
    (RESIDUALS, K_ANY, dict(bonus=A[2] + 8), ALIGNMENT),
    (RESIDUALS, K_ANY, dict(ld_t=V + 4), ALIGNMENT),
    (RESIDUALS, K_ANY, dict(ld_d=V + 4), ALIGNMENT),
    (RESIDUALS, K_ANY, dict(ld_b=V + 4), ALIGNMENT),
    (RESIDUALS, K_ANY, dict(workspace=A[8] + 16), WORKSPACE),
    (RESIDUALS, K_ANY, dict(workspace=A[8] + 16, t=A[0] + 2), ALIGNMENT),
    (RESIDUALS, K_ANY, dict(workspace_bytes=PLAIN_WS_LESS_1), WORKSPACE),
    (RESIDUALS, K_ANY, dict(workspace_bytes=0), WORKSPACE),
    (("asd_residual_sample", "asd_residual_sample_ex"), K_ANY, dict(workspace_bytes=0, inv_temperature=0.0), INVALID),
    (RESIDUALS, K_ANY, dict(workspace_bytes=0, B=-1), INVALID),
    (RESIDUALS, K_ANY, dict(workspace_bytes=0, workspace=None), INVALID),
    (("asd_residual_sample", "asd_residual_sample_ex"), K_ANY, dict(workspace_bytes=0, t=A[0] + 2), ALIGNMENT),
    # ---- asd_residual_sample_top_p / _top_k: their own checks come FIRST (NaN top_p, then -- only with something to truncate --
    # t_threshold, then the size of the workspace with the bonus thresholds behind it)
    (TRUNCATED, K_ANY, dict(top_p=NAN), INVALID),
    (TRUNCATED, K_ANY, dict(top_p=NAN, dtype=BAD_DTYPE), INVALID),
    (TRUNCATED, K_ANY, dict(top_p=NAN, B=0), INVALID),
    (TRUNCATED, K_ANY, dict(top_p=NAN, V=ODD_V, ld_t=ODD_V, ld_d=ODD_V, ld_b=ODD_V, workspace_bytes=0), INVALID),
    (TRUNCATED, K_ANY, dict(t_threshold=None), INVALID),
    (TRUNCATED, K_ANY, dict(t_threshold=None, dtype=BAD_DTYPE), INVALID),
    (TRUNCATED, K_ANY, dict(t_threshold=None, workspace_bytes=0), INVALID),
    (TRUNCATED, K_ANY, dict(t_threshold=None, B=0), OK),
    (TRUNCATED, K_ANY, dict(workspace_bytes=TOP_P_WS_LESS_1), WORKSPACE),
    (TRUNCATED, K_ANY, dict(workspace_bytes=PLAIN_WS), WORKSPACE),
    (TRUNCATED, K_ANY, dict(workspace_bytes=0, t=A[0] + 2), WORKSPACE),
    (TRUNCATED, K_ANY, dict(workspace_bytes=0, dtype=BAD_DTYPE), WORKSPACE),
    (TRUNCATED, K_ANY, dict(workspace_bytes=0, inv_temperature=0.0), WORKSPACE),
    (TRUNCATED, K_ANY, dict(workspace_bytes=0, K=-1), WORKSPACE),
    (TRUNCATED, K_ANY, dict(workspace_bytes=1 << 20, dtype=BAD_DTYPE), UNSUPPORTED),
    (TRUNCATED, K_ANY, dict(workspace_bytes=0, B=0), OK),
    (TRUNCATED, K_LIVE, dict(top_p=1.0, t_threshold=None), INVALID),           # a live top-k alone truncates
    (TRUNCATED, K_LIVE, dict(top_p=1.0, workspace_bytes=PLAIN_WS), WORKSPACE),
    (TRUNCATED, K_LIVE, dict(top_p=1.0, workspace_bytes=0, t=A[0] + 2), WORKSPACE),
    # nothing to truncate: t_threshold and the larger workspace are not asked for, the order is asd_residual_sample_ex's
    (TRUNCATED, K_DEAD, dict(top_p=1.0, t_threshold=None, dtype=BAD_DTYPE), UNSUPPORTED),
    (TRUNCATED, K_DEAD, dict(top_p=0.0, t_threshold=None, n_acc=None), INVALID),
    (TRUNCATED, K_DEAD, dict(top_p=1.0, workspace_bytes=PLAIN_WS, t=A[0] + 2), ALIGNMENT),
    (TRUNCATED, K_DEAD, dict(top_p=1.0, workspace_bytes=PLAIN_WS_LESS_1), WORKSPACE),
    (TRUNCATED, K_DEAD, dict(top_p=1.0, workspace_bytes=0, t=A[0] + 2), ALIGNMENT),
]


def _calls():
    for entries, top_ks, change, want in CASES:
        for name in entries:
            defaults, order = ENTRY[name]
            for top_k in (top_ks if "top_k" in order else top_ks[:1]):
                if "top_k" not in order and top_ks is K_LIVE:
                    continue                                      # a case about a live top-k: the other entries have none
                args = dict(defaults, top_k=top_k, **change)
                if top_k == V:
                    args["top_k"] = args["V"]                     # "bounds nothing" follows the case's vocabulary
                yield name, order, args, want


def test_rejected_calls_return_the_same_code_in_the_same_order():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: these calls carry made-up device addresses")
    from asd_amd import _binding
    lib = _binding.load_library()
    wrong, n = [], 0
    for name, order, args, want in _calls():
        ws = args["workspace_bytes"]
        if isinstance(ws, str):
            plain = lib.asd_residual_sample_workspace_bytes(args["B"], args["V"], args["dtype"])
            top_p = lib.asd_residual_sample_top_p_workspace_bytes(args["B"], args["V"], args["dtype"])
            assert top_p > plain
            args["workspace_bytes"] = {PLAIN_WS: plain, PLAIN_WS_LESS_1: plain - 1, TOP_P_WS_LESS_1: top_p - 1}[ws]
        got = getattr(lib, name)(*[args[a] for a in order])
        n += 1
        if got != want:
            shown = {k: v for k, v in args.items() if k in order and ENTRY[name][0][k] != v}
            wrong.append(f"{name}({shown}): returned {got}, expected {want}")
    assert n > 400
    assert not wrong, "\n".join(wrong)
