"""Which argument error asd_verify_greedy reports, and what its size query answers.

Every call below is REJECTED BEFORE ANY LAUNCH (or returns ASD_OK on the empty batch), so no GPU is needed -- and none is
allowed, as in tests/test_verify_arg_checks.py: the pointers are made-up addresses."""
import pytest

OK, INVALID, UNSUPPORTED, WORKSPACE, ALIGNMENT = 0, -1, -2, -3, -5
NAN, INF = float("nan"), float("inf")
F32, BF16, F16, BAD_DTYPE = 0, 1, 2, 7
V, K, B = 1000, 4, 3
A = [0x7F0000000000 + (i << 24) for i in range(12)]      # made-up, 256-byte aligned "device" addresses
ORDER = ["logits", "dtype", "ld_seq", "ld_row", "tok", "B", "K", "V", "inv_temperature", "splits", "argmax_out", "lp_argmax",
         "lp_target", "accept", "n_acc", "drawn", "lp_drawn", "workspace", "workspace_bytes", "stream"]
VALID = dict(logits=A[0], dtype=BF16, ld_seq=(K + 1) * V, ld_row=V, tok=A[1], B=B, K=K, V=V, inv_temperature=1.0, splits=0,
             argmax_out=A[2], lp_argmax=A[3], lp_target=A[4], accept=A[5], n_acc=A[6], drawn=A[7], lp_drawn=A[8],
             workspace=A[9], workspace_bytes=1 << 30, stream=None)
QUERY_LESS_1 = "query-1"

CASES = [
    # ---- null outputs / logits
    (dict(n_acc=None), INVALID),
    (dict(drawn=None), INVALID),
    (dict(lp_drawn=None), INVALID),
    (dict(logits=None), INVALID),
    (dict(workspace=None), INVALID),
    (dict(n_acc=None, K=65), INVALID),                                   # the outputs before K
    (dict(n_acc=None, drawn=None, lp_drawn=None, logits=None, workspace=None, B=0), OK),
    # ---- inv_temperature not > 0, before the empty-batch return
    (dict(inv_temperature=0.0), INVALID),
    (dict(inv_temperature=-1.0), INVALID),
    (dict(inv_temperature=INF), INVALID),
    (dict(inv_temperature=NAN), INVALID),
    (dict(inv_temperature=0.0, B=0), INVALID),
    (dict(inv_temperature=0.0, K=65), INVALID),
    # ---- sizes
    (dict(B=-1), INVALID),
    (dict(K=-1), INVALID),
    (dict(V=-1), INVALID),
    (dict(V=0, ld_row=0, ld_seq=0), INVALID),
    # ---- tok == NULL needs K == 0
    (dict(tok=None), INVALID),
    (dict(tok=None, K=0, ld_seq=V, workspace_bytes=0), WORKSPACE),       # (K = 0 takes no tok: the call gets as far as the workspace)
    # ---- ld too small
    (dict(ld_row=V - 1), INVALID),
    (dict(ld_seq=(K + 1) * V - 1), INVALID),
    (dict(ld_row=V + 8), INVALID),                                       # ld_seq < (K+1) ld_row
    (dict(ld_row=V - 1, logits=A[0] + 1), INVALID),                      # strides before alignment
    # ---- K too large, bad dtype, bad splits
    (dict(K=65, ld_seq=66 * V), UNSUPPORTED),
    (dict(K=65, ld_seq=66 * V, logits=None), UNSUPPORTED),               # K before the pointers
    (dict(dtype=BAD_DTYPE), UNSUPPORTED),
    (dict(dtype=BAD_DTYPE, tok=None), UNSUPPORTED),
    (dict(splits=-1), UNSUPPORTED),
    (dict(splits=65), UNSUPPORTED),
    (dict(splits=65, workspace_bytes=0), UNSUPPORTED),
    (dict(V=1 << 30, ld_row=1 << 30, ld_seq=5 << 30), UNSUPPORTED),      # a 2 GiB bf16 row
    # ---- alignment
    (dict(logits=A[0] + 1), ALIGNMENT),
    (dict(logits=A[0] + 2, dtype=F32), ALIGNMENT),
    (dict(logits=A[0] + 2, workspace_bytes=0), WORKSPACE),               # an element-aligned base is valid (scalar head): on to the workspace
    (dict(workspace=A[9] + 16), WORKSPACE),
    # ---- a short workspace
    (dict(workspace_bytes=0), WORKSPACE),
    (dict(workspace_bytes=255), WORKSPACE),
    (dict(splits=64, workspace_bytes=QUERY_LESS_1), WORKSPACE),          # the query sizes for the most splits
    (dict(splits=64, workspace_bytes=QUERY_LESS_1, dtype=F16), WORKSPACE),
    # ---- the empty batch
    (dict(B=0), OK),
    (dict(B=0, K=65, dtype=BAD_DTYPE, splits=99), OK),
]


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: these calls carry made-up device addresses")
    from asd_amd import _binding
    return _binding.load_library()


def test_rejected_calls_return_their_codes():
    lib = _no_gpu()
    wrong = []
    for change, want in CASES:
        args = dict(VALID, **change)
        if args["workspace_bytes"] == QUERY_LESS_1:
            args["workspace_bytes"] = lib.asd_verify_greedy_workspace_bytes(args["B"], args["K"], args["V"], args["dtype"]) - 1
        got = lib.asd_verify_greedy(*[args[a] for a in ORDER])
        if got != want:
            wrong.append(f"asd_verify_greedy({change}): returned {got}, expected {want}")
    assert not wrong, "\n".join(wrong)


def test_workspace_query_is_a_multiple_of_256_and_monotone():
    lib = _no_gpu()
    q = lambda b, k: lib.asd_verify_greedy_workspace_bytes(b, k, 152064, BF16)
    sizes = {(b, k): q(b, k) for b in (1, 2, 3, 8, 32, 33, 64) for k in (0, 1, 4, 8, 63, 64)}
    assert all(s > 0 and s % 256 == 0 for s in sizes.values())
    for (b, k), s in sizes.items():
        for (b2, k2), s2 in sizes.items():
            if b2 >= b and k2 >= k:
                assert s2 >= s, ((b, k), (b2, k2))
            if (b2 > b and k2 >= k) or (b2 >= b and k2 > k):
                assert s2 > s
    assert q(0, 4) == 256 and q(-1, 4) == 256 and q(4, -1) == 256
    assert q(4, 4) == lib.asd_verify_greedy_workspace_bytes(4, 4, 1000, F32)          # neither V nor the dtype enters the size
