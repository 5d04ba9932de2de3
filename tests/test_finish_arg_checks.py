"""Which argument error asd_commit_step_finish reports.

Every call below is REJECTED BEFORE ANY LAUNCH (or returns ASD_OK on the empty batch), so no GPU is needed -- and none is
allowed, as in tests/test_greedy_arg_checks.py: the pointers are made-up addresses.  The codes are asd_commit_step_stop's for the
arguments the two share (checked against that entry point itself), plus the rules of the sequence tables and `start`."""
import pytest

OK, INVALID, UNSUPPORTED = 0, -1, -2
K, B, T = 8, 4, 32
A = [0x7F0000000000 + (i << 24) for i in range(16)]      # made-up, 256-byte aligned "device" addresses
ORDER = ["tok", "lp_tok", "n_acc", "drawn", "lp_drawn", "B", "K", "seq_tok", "seq_n", "n_seq", "row_first", "row_max_len", "start",
         "seq_len", "out_tokens", "out_lp", "ld_out", "n_commit", "finished", "n_finished", "matched", "max_len", "stream"]
VALID = dict(tok=A[0], lp_tok=A[1], n_acc=A[2], drawn=A[3], lp_drawn=A[4], B=B, K=K, seq_tok=A[5], seq_n=A[6], n_seq=3,
             row_first=A[7], row_max_len=A[8], start=5, seq_len=A[9], out_tokens=A[10], out_lp=A[11], ld_out=T, n_commit=A[12],
             finished=A[13], n_finished=A[14], matched=A[15], max_len=T, stream=None)
STOP_ORDER = ["tok", "lp_tok", "n_acc", "drawn", "lp_drawn", "B", "K", "seq_tok", "n_seq", "seq_len", "out_tokens", "out_lp",
              "ld_out", "n_commit", "finished", "n_finished", "max_len", "stream"]

SHARED = [dict(B=-1), dict(K=-1), dict(max_len=-1), dict(n_seq=-1), dict(B=0), dict(B=0, K=65), dict(K=65), dict(tok=None),
          dict(lp_tok=None), dict(n_acc=None), dict(drawn=None), dict(lp_drawn=None), dict(seq_len=None), dict(out_tokens=None),
          dict(out_lp=None), dict(ld_out=T - 1), dict(finished=None), dict(K=65, finished=None), dict(B=-1, K=65),
          dict(B=-1, n_seq=0, seq_tok=None)]

OWN = [
    (dict(start=-1), INVALID),
    (dict(start=-1, B=0), INVALID),                           # sizes before the empty batch
    (dict(start=0, finished=None), INVALID),                  # (start = 0 is valid: on to the pointers)
    (dict(seq_tok=None), INVALID),
    (dict(seq_n=None), INVALID),
    (dict(seq_tok=None, seq_n=None, n_seq=1), INVALID),
    (dict(n_seq=17, row_first=None), UNSUPPORTED),
    (dict(n_seq=17, row_first=None, tok=None), UNSUPPORTED),  # the limit before the pointers, like K
    (dict(n_seq=16, row_first=None, finished=None), INVALID),
    (dict(n_seq=1000, finished=None), INVALID),               # with row_first any total is allowed: on to the pointers
    (dict(B=0, n_seq=1000, row_first=None, K=99, tok=None, finished=None, start=0), OK),
    (dict(B=0, tok=None, lp_tok=None, n_acc=None, drawn=None, lp_drawn=None, seq_tok=None, seq_n=None, seq_len=None,
          out_tokens=None, out_lp=None, finished=None), OK),
]


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: these calls carry made-up device addresses")
    from asd_amd import _binding
    return _binding.load_library()


def test_the_shared_arguments_are_judged_as_commit_step_stop_judges_them():
    lib = _no_gpu()
    wrong, seen = [], set()
    for change in SHARED:
        args = dict(VALID, **change)
        got = lib.asd_commit_step_finish(*[args[a] for a in ORDER])
        want = lib.asd_commit_step_stop(*[args[a] for a in STOP_ORDER])
        seen.add(want)
        if got != want:
            wrong.append(f"asd_commit_step_finish({change}): returned {got}, asd_commit_step_stop {want}")
    assert not wrong, "\n".join(wrong)
    assert seen == {OK, INVALID, UNSUPPORTED}


def test_rejected_calls_return_their_codes():
    lib = _no_gpu()
    wrong = []
    for change, want in OWN:
        args = dict(VALID, **change)
        got = lib.asd_commit_step_finish(*[args[a] for a in ORDER])
        if got != want:
            wrong.append(f"asd_commit_step_finish({change}): returned {got}, expected {want}")
    assert not wrong, "\n".join(wrong)


def test_the_binding_and_the_header_agree_on_the_limits():
    import os
    import re
    from asd_amd import _binding
    from asd_amd.serving import stages
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "asd_hip.h")).read()
    limits = {k: int(v) for k, v in re.findall(r"#define (ASD_MAX_STOP_SEQS|ASD_MAX_STOP_SEQ_LEN) (\d+)", text)}
    assert limits == {"ASD_MAX_STOP_SEQS": 16, "ASD_MAX_STOP_SEQ_LEN": 8}
    assert (_binding.MAX_STOP_SEQS, _binding.MAX_STOP_SEQ_LEN) == (16, 8) == (stages.MAX_STOP_SEQS, stages.MAX_STOP_SEQ_LEN)


def test_pack_stop_sequences_checks_the_host_lists():
    import torch
    from asd_amd.kernels import pack_stop_sequences
    tok, n, first = pack_stop_sequences([[(1, 2)], [], [(3,), (4, 5, 6, 7, 8, 9, 10, 11)]], "cpu")
    assert tok.dtype == n.dtype == first.dtype == torch.int32 and tok.shape == (3, 8)
    assert n.tolist() == [2, 1, 8] and first.tolist() == [0, 1, 1, 3] and tok[0].tolist() == [1, 2, 0, 0, 0, 0, 0, 0]
    tok, n, first = pack_stop_sequences([(1, 2), (3,)], "cpu", shared=True)
    assert first is None and n.tolist() == [2, 1]
    with pytest.raises(ValueError):
        pack_stop_sequences([[(i,) for i in range(17)]], "cpu")
    with pytest.raises(ValueError):
        pack_stop_sequences([(i,) for i in range(17)], "cpu", shared=True)
    with pytest.raises(ValueError):
        pack_stop_sequences([[()]], "cpu")
    with pytest.raises(ValueError):
        pack_stop_sequences([[tuple(range(9))]], "cpu")
    assert pack_stop_sequences([[(i,) for i in range(16)]] * 3, "cpu")[2].tolist() == [0, 16, 32, 48]
