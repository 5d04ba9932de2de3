"""Per-request sampling parameters, the host side: every ValueError of Stage.generate and the pipeline (raised before any ops
call), the status codes of asd_sampling_rows_pack, and the packed fields against log2_scale / truncation / min_p_delta restated
in numpy (as tests/min_p_ref.min_p_delta restates the launcher's delta).  The library loads without a GPU; nothing here launches."""
import ctypes as C

import numpy as np
import pytest

import asd_amd
from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
from asd_amd.serving.stages import StageManager, check_per_prompt
from tests.min_p_ref import min_p_delta
from tests.oracle_backend import OracleBackend
from tests.per_request_ref import RowsOracleOps
from tests.stage_scenario import PROMPTS, stage_configs
from tests.test_seeded_stages import SeedRecordingManager, WordPredictor

NAN = float("nan")
OK, INVALID, UNSUPPORTED = 0, -1, -2
DT_F32, DT_BF16, DT_F16 = 0, 1, 2
ROW_BYTES = 32


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def _five(v, at=1, bad=None):
    out = [v] * 5
    out[at] = bad
    return out


BAD = [
    # a bool, a NaN
    (dict(temperature=True), "temperature"), (dict(temperature=NAN), "temperature"), (dict(temperature=_five(0.7, bad=True)), "temperature"),
    (dict(temperature=_five(0.7, bad=NAN)), "temperature"), (dict(top_p=True), "top_p"), (dict(top_p=NAN), "top_p"),
    (dict(top_p=_five(0.9, bad=NAN)), "top_p"), (dict(top_p=_five(0.9, bad=False)), "top_p"), (dict(top_p="0.9"), "top_p"),
    (dict(min_p=True), "min_p"), (dict(min_p=NAN), "min_p"), (dict(min_p=_five(0.1, bad=NAN)), "min_p"),
    (dict(top_k=True), "top_k"), (dict(top_k=_five(5, bad=False)), "top_k"),
    # a negative temperature
    (dict(temperature=-0.5), "temperature"), (dict(temperature=_five(0.7, bad=-1.0)), "temperature"),
    # min_p outside [0, 1]
    (dict(min_p=1.5), "min_p"), (dict(min_p=-0.1), "min_p"), (dict(min_p=_five(0.1, bad=1.0000001)), "min_p"),
    (dict(min_p=_five(0.1, bad=-1e-9)), "min_p"),
    # a non-integer top_k
    (dict(top_k=1.5), "top_k"), (dict(top_k=50.0), "top_k"), (dict(top_k=_five(5, bad=2.0)), "top_k"), (dict(top_k="5"), "top_k"),
    (dict(top_k=NAN), "top_k"),
    # a sequence of the wrong length, or one holding None
    (dict(temperature=[0.7] * 4), "temperature"), (dict(temperature=[0.7] * 6), "temperature"), (dict(temperature=[]), "temperature"),
    (dict(top_p=[0.9] * 4), "top_p"), (dict(top_k=[5] * 6), "top_k"), (dict(min_p=[0.1]), "min_p"),
    (dict(temperature=_five(0.7)), "temperature"), (dict(top_p=_five(0.9)), "top_p"), (dict(top_k=_five(5)), "top_k"),
    (dict(min_p=_five(0.1)), "min_p"),
    # greedy and sampled rows in one call
    (dict(temperature=[0.0, 0.7, 0.7, 0.7, 0.7]), "greedy"), (dict(temperature=[0.7, 0.7, 0.0, 0.0, 1.0]), "greedy"),
]


@pytest.mark.parametrize("kw,match", BAD)
def test_bad_values_raise_before_any_ops_call(kw, match):
    ops = RowsOracleOps()
    sm = StageManager(stage_configs(), ops=ops)
    for name in ("8b", "13b"):
        with pytest.raises(ValueError, match=match):
            sm.get_stage(name).generate(prompts=PROMPTS, max_tokens=3, **kw)
    assert ops.trace == []


def test_check_per_prompt_collapses_equal_sequences():
    assert check_per_prompt(None, 3, "top_p") is None
    assert check_per_prompt([0.9, 0.9, 0.9], 3, "top_p") == 0.9 and check_per_prompt((5, 5), 2, "top_k") == 5
    assert check_per_prompt(np.array([0.5, 0.5]), 2, "temperature") == 0.5
    assert check_per_prompt([0.9, 1.0, 0.9], 3, "top_p") == [0.9, 1.0, 0.9]
    assert check_per_prompt([0, -3, 10 ** 6], 3, "top_k") == [0, -3, 10 ** 6]          # off values are values, not errors
    assert check_per_prompt([0.0, 1.0, 2.5, -1.0], 4, "top_p") == [0.0, 1.0, 2.5, -1.0]
    assert check_per_prompt(np.int64(7), 4, "top_k") == 7 and check_per_prompt(np.float32(0.5), 4, "min_p") == 0.5


def _pipeline():
    sm = SeedRecordingManager()
    return AdaptiveSpeculativePipeline(sm, WordPredictor(), object(),
                                       PipelineConfig(lambda_value=30.0, stop_rule="full", risk_adjustment=False)), sm


def test_pipeline_validation_runs_nothing():
    pipe, sm = _pipeline()
    three = ["easy a", "hard a", "mid a"]
    for kw, match in [(dict(top_p=[0.9, 0.8]), "top_p"), (dict(top_p=[0.9, None, 0.8]), "top_p"), (dict(top_k=[1, 2.5, 3]), "top_k"),
                      (dict(top_k=True), "top_k"), (dict(min_p=[0.1, 0.2, 1.5]), "min_p"), (dict(min_p=NAN), "min_p"),
                      (dict(temperature=[0.7, 0.7]), "temperature"), (dict(temperature=[0.7, -1.0, 0.7]), "temperature"),
                      (dict(temperature=[0.7, None, 0.7]), "temperature"), (dict(temperature=[0.7, NAN, 0.7]), "temperature")]:
        with pytest.raises(ValueError, match=match):
            pipe.batch_process(three, max_tokens=4, **kw)
    for kw, match in [(dict(top_k=1.5), "top_k"), (dict(top_p=NAN), "top_p"), (dict(min_p=2.0), "min_p"), (dict(top_p=[0.9, 0.8]), "top_p")]:
        with pytest.raises(ValueError, match=match):
            pipe.process_request("hard x", max_tokens=4, **kw)
    assert not any(st.calls for st in sm.stages.values())
    pipe.shutdown()


# ------------------------------------------------------------------------------------------ asd_sampling_rows_pack
def _lib():
    from asd_amd import _binding
    return _binding.load_library()


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _pack(inv_t, top_k=None, top_p=None, min_p=None, V=1000, dtype=DT_BF16, B=None, out=True):
    inv_t = None if inv_t is None else np.ascontiguousarray(inv_t, np.float32)
    n = (0 if inv_t is None else len(inv_t)) if B is None else B
    arr = lambda v, dt: None if v is None else np.ascontiguousarray(v, dt)           # noqa: E731
    packed = np.full(max(n, 1) * ROW_BYTES + 8, 0xAB, np.uint8) if out else None
    rc = _lib().asd_sampling_rows_pack(_vp(inv_t), _vp(arr(top_k, np.int32)), _vp(arr(top_p, np.float32)), _vp(arr(min_p, np.float32)),
                                       n, V, dtype, _vp(packed))
    return rc, packed


def test_pack_status_codes():
    lib = _lib()
    assert lib.asd_sampling_rows_bytes(0) == 0 and lib.asd_sampling_rows_bytes(-3) == 0 and lib.asd_sampling_rows_bytes(7) == 7 * ROW_BYTES
    assert _pack([1.0, 2.0])[0] == OK
    assert _pack([1.0], [5], [0.9], [0.1])[0] == OK
    assert _pack([], B=0)[0] == OK and _pack(None, B=0, out=False)[0] == OK
    for bad in (0.0, -1.0, NAN, float("inf"), 3.0e38):
        assert _pack([1.0, bad, 1.0])[0] == INVALID, bad
    assert _pack([1.0, 1.0], top_p=[0.9, NAN])[0] == INVALID
    for bad in (NAN, 1.0000001, 1.5, float("inf")):
        assert _pack([1.0, 1.0], min_p=[0.1, bad])[0] == INVALID, bad
    for off in (0.0, -0.0, -1.0, float("-inf")):                                   # min_p <= 0 is the off switch, not an error
        assert _pack([1.0, 1.0], min_p=[0.1, off])[0] == OK
    for any_top_p in (0.0, 1.0, -2.0, 7.0, float("inf")):                          # top_p outside (0, 1) likewise
        assert _pack([1.0], top_p=[any_top_p])[0] == OK
    assert _pack([1.0], top_k=[-5])[0] == OK and _pack([1.0], top_k=[2 ** 31 - 1])[0] == OK
    assert _pack([1.0], dtype=3)[0] == UNSUPPORTED and _pack([1.0], dtype=-1)[0] == UNSUPPORTED
    assert _pack([1.0], B=-1)[0] == INVALID and _pack([1.0], V=0)[0] == INVALID
    assert _pack(None, B=2)[0] == INVALID and _pack([1.0, 1.0], out=False)[0] == INVALID
    # a rejected call and the bytes behind the table are left alone
    rc, packed = _pack([1.0, NAN])
    assert rc == INVALID and (packed == 0xAB).all()
    rc, packed = _pack([1.0, 2.0])
    assert rc == OK and (packed[2 * ROW_BYTES:] == 0xAB).all()


def log2_scale(inv_t):
    """(float)(1.4426950408889634074 * (double)inv_temperature)"""
    return np.float32(1.4426950408889634074 * float(np.float32(inv_t)))


@pytest.mark.parametrize("dtype,V", [(DT_BF16, 1000), (DT_F16, 8200), (DT_F32, 4100), (DT_BF16, 152064)])
def test_packed_fields_are_the_launchers_own_values(dtype, V):
    temps = [0.5, 0.7, 0.9, 1.0, 1.3, 2.0, 0.7, 1e-3, 100.0]
    inv_t = np.array([np.float32(1.0 / t) for t in temps], np.float32)
    n = len(temps)
    top_k = np.array([0, 50, -1, V, V - 1, 1, V + 5, 50, 0], np.int32)
    top_p = np.array([0.9, 1.0, 0.0, 0.5, 1.5, 0.999, -0.1, 0.9, 1e-6], np.float32)
    min_p = np.array([0.0, 0.1, 1.0, -1.0, 1e-6, 0.3, 0.0, 1e-30, 0.05], np.float32)
    rc, packed = _pack(inv_t, top_k, top_p, min_p, V=V, dtype=dtype)
    assert rc == OK
    words = packed[:n * ROW_BYTES].view(np.uint32).reshape(n, 8)
    f32 = lambda col: words[:, col].copy().view(np.float32)                          # noqa: E731
    i32 = lambda col: words[:, col].copy().view(np.int32)                            # noqa: E731
    want_c2 = np.array([log2_scale(v) for v in inv_t], np.float32)
    assert f32(0).tobytes() == want_c2.tobytes()
    assert f32(1).tobytes() == top_p.tobytes()
    nucleus = (top_p > 0) & (top_p < 1)
    assert np.array_equal(i32(2), np.where(nucleus, 3 if dtype == DT_F32 else 2, 0))
    assert np.array_equal(i32(3), np.where((top_k > 0) & (top_k < V), top_k, 0))
    on = min_p > 0
    want_delta = np.array([min_p_delta(m, v) if o else -np.inf for m, v, o in zip(min_p, inv_t, on)], np.float32)
    assert f32(4).tobytes() == want_delta.tobytes() and (want_delta[on] <= 0).all()
    assert np.array_equal(words[:, 5], on.astype(np.uint32))
    assert (words[:, 6:] == 0).all()
    # NULL arrays are "off for every sequence"
    rc, packed = _pack(inv_t, V=V, dtype=dtype)
    w = packed[:n * ROW_BYTES].view(np.uint32).reshape(n, 8)
    assert rc == OK and w[:, 0].tobytes() == want_c2.view(np.uint32).tobytes()
    assert (w[:, 1].copy().view(np.float32) == 1.0).all() and (w[:, 2] == 0).all() and (w[:, 3] == 0).all()
    assert np.isneginf(w[:, 4].copy().view(np.float32)).all() and (w[:, 5:] == 0).all()
    # a uniform table repeats one row
    rc, packed = _pack(np.full(4, inv_t[1]), np.full(4, 50), np.full(4, 0.9), np.full(4, 0.1), V=V, dtype=dtype)
    w = packed[:4 * ROW_BYTES].reshape(4, ROW_BYTES)
    assert rc == OK and all(w[i].tobytes() == w[0].tobytes() for i in range(4))
