"""prompt_logprobs, host side: every ValueError of serving/stage_args.py::_check_prompt_logprobs, raised by Stage.generate before
the prompts are encoded and before any op is called (a stub that counts every ops call); and which argument error
asd_prompt_logprobs reports, in the header's order, with what its size query answers.  The C calls below are REJECTED BEFORE ANY
LAUNCH, so no GPU is needed -- and none is allowed, as in tests/test_top_logprobs_arg_checks.py: the pointers are made up."""
import numpy as np
import pytest

import asd_amd
from asd_amd.serving.stage_args import MAX_TOP_LOGPROBS, _check_prompt_logprobs
from asd_amd.serving.stages import StageConfig, StageManager
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import NAMES, PROMPTS, stage_configs

BAD = (True, False, 1.0, 2.5, float("nan"), "2", -1, 9, 1 << 40, [2], (1, 2), [1] * len(PROMPTS), np.float32(1.0), np.bool_(True))


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


class CountingOps:
    """Every attribute is an op that counts its call and returns nothing: a refused call must leave `calls` at 0."""

    def __init__(self):
        self.calls = 0

    def __getattr__(self, name):
        def op(*a, **kw):
            self.calls += 1
        return op


def test_check_prompt_logprobs():
    assert MAX_TOP_LOGPROBS == 8
    assert _check_prompt_logprobs(None) is None
    assert [_check_prompt_logprobs(n) for n in (0, 1, 8, np.int64(5))] == [0, 1, 8, 5]
    assert type(_check_prompt_logprobs(np.int32(3))) is int
    for bad in BAD:
        with pytest.raises(ValueError, match="prompt_logprobs"):
            _check_prompt_logprobs(bad)


@pytest.mark.parametrize("name", NAMES)
def test_generate_refuses_bad_values_before_encoding_and_before_any_op(name):
    ops = CountingOps()
    stage = StageManager(stage_configs(vocab=64), ops=ops).get_stage(name)
    encoded = []
    stage._encode = lambda prompts: encoded.append(prompts)
    for bad in BAD:
        for temperature in (0.0, 0.7):
            with pytest.raises(ValueError, match="prompt_logprobs"):
                stage.generate(prompts=PROMPTS, max_tokens=4, temperature=temperature, prompt_logprobs=bad)
    assert ops.calls == 0 and not encoded


@pytest.mark.parametrize("bad", [True, 1.5, 9, -1, [1]])
def test_a_bad_configuration_value_is_refused_at_the_call(bad):
    ops = CountingOps()
    stage = StageManager(stage_configs(vocab=64, prompt_logprobs=bad), ops=ops).get_stage(NAMES[1])
    with pytest.raises(ValueError, match="prompt_logprobs"):
        stage.generate(prompts=PROMPTS, max_tokens=4, temperature=0.0)
    assert ops.calls == 0
    assert StageConfig(model_name="m", model_size="s").prompt_logprobs is None       # off by default


# ------------------------------------------------------------------------------------------ the C entry point
OK, INVALID, UNSUPPORTED, WORKSPACE, ALIGNMENT = 0, -1, -2, -3, -5
F32, BF16, F16, BAD_DTYPE = 0, 1, 2, 7
V, T, B, N = 1000, 70, 3, 5
A = [0x7F0000000000 + (i << 24) for i in range(12)]      # made-up, 256-byte aligned "device" addresses
ORDER = ["logits", "dtype", "ld_seq", "ld_row", "B", "T", "V", "target", "ld_target", "first", "inv_temperature", "N", "splits", "lp",
         "rank", "top_id", "top_lp", "workspace", "workspace_bytes", "stream"]
VALID = dict(logits=A[0], dtype=BF16, ld_seq=T * V, ld_row=V, B=B, T=T, V=V, target=A[1], ld_target=T, first=A[2], inv_temperature=1.0,
             N=N, splits=0, lp=A[3], rank=A[4], top_id=A[5], top_lp=A[6], workspace=A[7], workspace_bytes=1 << 30, stream=None)
QUERY_LESS_1 = "query-1"

CASES = [
    # ---- NULL outputs, ahead of everything; the table's only with N > 0
    (dict(lp=None), INVALID),
    (dict(rank=None), INVALID),
    (dict(top_id=None), INVALID),
    (dict(top_lp=None), INVALID),
    (dict(lp=None, N=9), INVALID),
    (dict(top_id=None, top_lp=None, N=0, workspace_bytes=0), WORKSPACE),            # N == 0: no table, a valid call
    (dict(inv_temperature=0.0), INVALID),
    (dict(inv_temperature=float("nan")), INVALID),
    # ---- negative sizes, then the empty batch
    (dict(B=-1), INVALID),
    (dict(T=-1), INVALID),
    (dict(V=-1), INVALID),
    (dict(N=-1), INVALID),
    (dict(B=0), OK),
    (dict(B=0, lp=None, rank=None, top_id=None, top_lp=None, logits=None, target=None, workspace=None, dtype=BAD_DTYPE, N=99), OK),
    (dict(T=0, ld_seq=0, lp=None, rank=None), OK),
    (dict(V=0, ld_row=0, ld_seq=0), INVALID),
    # ---- dtype, then N and splits
    (dict(dtype=BAD_DTYPE), UNSUPPORTED),
    (dict(dtype=BAD_DTYPE, N=9, ld_row=V - 1), UNSUPPORTED),
    (dict(N=9), UNSUPPORTED),
    (dict(N=9, ld_row=V - 1), UNSUPPORTED),                                         # N before the strides
    (dict(splits=-1), UNSUPPORTED),
    (dict(splits=65), UNSUPPORTED),
    # ---- pointers and strides
    (dict(logits=None), INVALID),
    (dict(target=None), INVALID),
    (dict(workspace=None), INVALID),
    (dict(ld_row=V - 1), INVALID),
    (dict(ld_seq=T * V - 1), INVALID),
    (dict(ld_target=T - 1), INVALID),
    (dict(ld_target=T - 1, logits=A[0] + 1), INVALID),                              # strides before alignment
    (dict(first=None, workspace_bytes=0), WORKSPACE),                               # first may be NULL
    # ---- a row of 2 GiB, then alignment, then the workspace
    (dict(V=1 << 30, ld_row=1 << 30, ld_seq=T << 30, logits=A[0] + 1), UNSUPPORTED),
    (dict(logits=A[0] + 1), ALIGNMENT),
    (dict(logits=A[0] + 2, dtype=F32), ALIGNMENT),
    (dict(logits=A[0] + 2, workspace_bytes=0), WORKSPACE),                          # an element-aligned base is valid (scalar head)
    (dict(workspace=A[7] + 16), WORKSPACE),
    (dict(workspace_bytes=255), WORKSPACE),
    (dict(T=300, ld_seq=300 * V, ld_target=300, workspace_bytes=0), WORKSPACE),     # no 65-row limit
    (dict(splits=64, workspace_bytes=QUERY_LESS_1), WORKSPACE),
    (dict(splits=2, workspace_bytes=QUERY_LESS_1, dtype=F16, N=0), WORKSPACE),
    (dict(splits=1, workspace_bytes=QUERY_LESS_1), WORKSPACE),
    (dict(splits=0, workspace_bytes=QUERY_LESS_1), WORKSPACE),
    (dict(B=1 << 20, T=1 << 10, ld_seq=V << 10, ld_target=1 << 10, splits=4), UNSUPPORTED),       # B*T*S > INT32_MAX
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
            args["workspace_bytes"] = lib.asd_prompt_logprobs_workspace_bytes(args["B"], args["T"], args["V"], args["dtype"],
                                                                              args["splits"]) - 1
        got = lib.asd_prompt_logprobs(*[args[a] for a in ORDER])
        if got != want:
            wrong.append(f"asd_prompt_logprobs({change}): returned {got}, expected {want}")
    assert not wrong, "\n".join(wrong)


def test_workspace_query_is_sized_for_the_splits_in_use():
    lib = _no_gpu()
    q = lib.asd_prompt_logprobs_workspace_bytes
    # a real prompt: B*T around 65k rows take one slice each (a host without a device counts 256 CUs) and need no partials
    assert q(32, 2047, 152064, BF16, 0) < (1 << 20) and q(32, 2047, 152064, BF16, 0) % 256 == 0
    assert q(32, 2047, 152064, BF16, 1) == 256
    sizes = [q(2, 70, 4099, dt, s) for dt in (F32, BF16, F16) for s in (0, 1, 2, 3, 7, 64)]
    assert all(s >= 256 and s % 256 == 0 for s in sizes)
    assert q(2, 70, 4099, BF16, 2) < q(2, 70, 4099, BF16, 3) < q(2, 70, 4099, BF16, 64)
    assert q(2, 70, 4099, BF16, 64) == 2 * 70 * 64 + -(-2 * 70 * 64 * 80 // 256) * 256       # a ticket line and 64 partials per row
    assert q(0, 70, 4099, BF16, 0) == q(2, 0, 4099, BF16, 0) == q(2, 70, 4099, BAD_DTYPE, 0) == q(2, 70, 4099, BF16, 65) == 256
