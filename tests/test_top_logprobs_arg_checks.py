"""Which argument error asd_top_logprobs and asd_commit_top_logprobs report, and what the size query answers.

Every call below is REJECTED BEFORE ANY LAUNCH (or returns ASD_OK on the empty batch), so no GPU is needed -- and none is
allowed, as in tests/test_greedy_arg_checks.py: the pointers are made-up addresses."""
import pytest

OK, INVALID, UNSUPPORTED, WORKSPACE, ALIGNMENT = 0, -1, -2, -3, -5
NAN, INF = float("nan"), float("inf")
F32, BF16, F16, BAD_DTYPE = 0, 1, 2, 7
V, K1, B, N = 1000, 5, 3, 5
A = [0x7F0000000000 + (i << 24) for i in range(12)]      # made-up, 256-byte aligned "device" addresses
ORDER = ["logits", "dtype", "ld_seq", "ld_row", "B", "K1", "V", "inv_temperature", "N", "splits", "top_id", "top_lp", "workspace",
         "workspace_bytes", "stream"]
VALID = dict(logits=A[0], dtype=BF16, ld_seq=K1 * V, ld_row=V, B=B, K1=K1, V=V, inv_temperature=1.0, N=N, splits=0, top_id=A[1],
             top_lp=A[2], workspace=A[3], workspace_bytes=1 << 30, stream=None)
QUERY_LESS_1 = "query-1"

CASES = [
    # ---- null outputs, ahead of everything
    (dict(top_id=None), INVALID),
    (dict(top_lp=None), INVALID),
    (dict(top_id=None, N=9), INVALID),
    (dict(top_id=None, top_lp=None, logits=None, workspace=None, B=0), OK),
    # ---- inv_temperature not > 0, before the empty-batch return
    (dict(inv_temperature=0.0), INVALID),
    (dict(inv_temperature=-1.0), INVALID),
    (dict(inv_temperature=INF), INVALID),
    (dict(inv_temperature=NAN), INVALID),
    (dict(inv_temperature=0.0, B=0), INVALID),
    (dict(inv_temperature=0.0, N=9), INVALID),
    # ---- sizes
    (dict(B=-1), INVALID),
    (dict(K1=-1), INVALID),
    (dict(V=-1), INVALID),
    (dict(N=-1), INVALID),
    (dict(V=0, ld_row=0, ld_seq=0), INVALID),
    (dict(K1=0, ld_seq=0), INVALID),
    (dict(N=0), INVALID),
    (dict(N=0, dtype=BAD_DTYPE), INVALID),                               # N < 1 before the dtype
    # ---- pointers and strides
    (dict(logits=None), INVALID),
    (dict(workspace=None), INVALID),
    (dict(ld_row=V - 1), INVALID),
    (dict(ld_seq=K1 * V - 1), INVALID),
    (dict(ld_row=V + 8), INVALID),                                       # ld_seq < K1 ld_row
    (dict(ld_row=V - 1, logits=A[0] + 1), INVALID),                      # strides before alignment
    # ---- N, K1 too large, bad dtype, bad splits, a row too long
    (dict(N=9), UNSUPPORTED),
    (dict(N=9, logits=None), UNSUPPORTED),                               # N before the pointers
    (dict(K1=66, ld_seq=66 * V), UNSUPPORTED),
    (dict(K1=65, ld_seq=65 * V, workspace_bytes=0), WORKSPACE),          # K + 1 rows with K = 64: supported
    (dict(dtype=BAD_DTYPE), UNSUPPORTED),
    (dict(splits=-1), UNSUPPORTED),
    (dict(splits=65), UNSUPPORTED),
    (dict(splits=65, workspace_bytes=0), UNSUPPORTED),
    (dict(V=1 << 30, ld_row=1 << 30, ld_seq=5 << 30), UNSUPPORTED),      # a 2 GiB bf16 row
    # ---- alignment
    (dict(logits=A[0] + 1), ALIGNMENT),
    (dict(logits=A[0] + 2, dtype=F32), ALIGNMENT),
    (dict(logits=A[0] + 2, workspace_bytes=0), WORKSPACE),               # an element-aligned base is valid (scalar head)
    (dict(workspace=A[3] + 16), WORKSPACE),
    # ---- a short workspace
    (dict(workspace_bytes=0), WORKSPACE),
    (dict(workspace_bytes=255), WORKSPACE),
    (dict(splits=64, workspace_bytes=QUERY_LESS_1), WORKSPACE),          # the query sizes for the most splits
    (dict(splits=64, workspace_bytes=QUERY_LESS_1, dtype=F16, N=1), WORKSPACE),
    # ---- the empty batch
    (dict(B=0), OK),
    (dict(B=0, K1=99, N=99, dtype=BAD_DTYPE, splits=99), OK),
]

C_ORDER = ["top_id", "top_lp", "seq_len", "n_commit", "B", "K1", "N", "out_id", "out_lp", "max_len", "stream"]
C_VALID = dict(top_id=A[0], top_lp=A[1], seq_len=A[2], n_commit=A[3], B=B, K1=K1, N=N, out_id=A[4], out_lp=A[5], max_len=32,
               stream=None)
C_CASES = [
    (dict(B=-1), INVALID),
    (dict(K1=-1), INVALID),
    (dict(N=-1), INVALID),
    (dict(max_len=-1), INVALID),
    (dict(B=0), OK),
    (dict(B=0, top_id=None, top_lp=None, seq_len=None, n_commit=None, out_id=None, out_lp=None, K1=99, N=99), OK),
    (dict(K1=66), UNSUPPORTED),
    (dict(N=9), UNSUPPORTED),
    (dict(N=9, top_id=None), UNSUPPORTED),
    (dict(K1=0), INVALID),
    (dict(N=0), INVALID),
] + [(dict(**{k: None}), INVALID) for k in ("top_id", "top_lp", "seq_len", "n_commit", "out_id", "out_lp")]


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
            args["workspace_bytes"] = lib.asd_top_logprobs_workspace_bytes(args["B"], args["K1"], args["N"]) - 1
        got = lib.asd_top_logprobs(*[args[a] for a in ORDER])
        if got != want:
            wrong.append(f"asd_top_logprobs({change}): returned {got}, expected {want}")
    for change, want in C_CASES:
        args = dict(C_VALID, **change)
        got = lib.asd_commit_top_logprobs(*[args[a] for a in C_ORDER])
        if got != want:
            wrong.append(f"asd_commit_top_logprobs({change}): returned {got}, expected {want}")
    assert not wrong, "\n".join(wrong)


def test_workspace_query_is_a_multiple_of_256_and_monotone():
    lib = _no_gpu()
    q = lambda b, k1: lib.asd_top_logprobs_workspace_bytes(b, k1, 5)
    sizes = {(b, k): q(b, k) for b in (1, 2, 3, 8, 32, 33, 64) for k in (1, 2, 5, 9, 64, 65)}
    assert all(s > 0 and s % 256 == 0 for s in sizes.values())
    for (b, k), s in sizes.items():
        for (b2, k2), s2 in sizes.items():
            if b2 >= b and k2 >= k:
                assert s2 >= s, ((b, k), (b2, k2))
            if (b2 > b and k2 >= k) or (b2 >= b and k2 > k):
                assert s2 > s
    assert q(0, 4) == 256 and q(-1, 4) == 256 and q(4, 0) == 256
    assert q(4, 4) == lib.asd_top_logprobs_workspace_bytes(4, 4, 8)                  # N does not enter the size
