"""generate(repetition_penalty=, presence_penalty=, frequency_penalty=) on CPU (serving/stages.py, PENALTIES): every bad value
raises ValueError with the keyword's name before any ops call, from the stage and through the pipeline, and neutral values --
1.0 / 0.0 / 0.0, sequences of them, None -- make exactly the ops calls of the call without the keywords."""
import numpy as np
import pytest

import asd_amd
from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
from asd_amd.serving.stage_args import check_frequency_penalty, check_presence_penalty, check_repetition_penalty
from asd_amd.serving.stages import StageManager
from tests.logit_edit_ref import SEEDS
from tests.oracle_backend import OracleBackend
from tests.penalty_ref import PenaltyOracleOps
from tests.stage_scenario import NAMES, PROMPTS, TEMPERATURE, LogprobPredictor, stage_configs

N = len(PROMPTS)
NAN = float("nan")


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def _manager(**kw):
    ops = PenaltyOracleOps()
    return StageManager(stage_configs(**kw), ops=ops), ops


def _bad(name, lo, hi, open_lo):
    out = [True, False, NAN, "1.0", b"1", {}, object(), hi + 0.001, lo - 0.001, float("inf"), float("-inf"), 1 + 2j,
           [hi] * (N - 1), [hi] * (N + 1), [], [hi, None, hi, hi, hi], [hi, hi, NAN, hi, hi], [hi, hi, hi, hi, True],
           [hi, hi, hi, "x", hi], [hi, hi, hi, hi, lo - 1], [[hi]] * N, np.array([hi] * (N - 1))]
    if open_lo:
        out += [lo, [hi, hi, lo, hi, hi]]                 # the open end of (0, 2]
    return [{name: v} for v in out]


BAD = _bad("repetition_penalty", 0.0, 2.0, True) + _bad("presence_penalty", -2.0, 2.0, False) + \
    _bad("frequency_penalty", -2.0, 2.0, False)


@pytest.mark.parametrize("name", [NAMES[0], NAMES[2]])
def test_bad_values_raise_before_any_launch(name):
    sm, ops = _manager()
    stage = sm.get_stage(name)
    encoded = []
    stage.encode_prompts = lambda *a: encoded.append(a) or 1 / 0              # the checks come first
    stage._encode = lambda *a: encoded.append(a) or 1 / 0
    for kw in BAD:
        for temperature in (TEMPERATURE, 0.0):
            with pytest.raises(ValueError, match=next(iter(kw))):
                stage.generate(prompts=PROMPTS, max_tokens=2, temperature=temperature, **kw)
    assert ops.trace == [] and not ops.calls and not encoded, (ops.trace, ops.calls)


def test_bad_values_raise_through_the_pipeline_before_any_launch():
    sm, ops = _manager()
    pipe = AdaptiveSpeculativePipeline(sm, LogprobPredictor(), object(), PipelineConfig(lambda_value=30.0, stage_names=NAMES))
    for kw in BAD:
        with pytest.raises(ValueError, match=next(iter(kw))):
            pipe.batch_process(PROMPTS, max_tokens=2, temperature=TEMPERATURE, **kw)
        v = next(iter(kw.values()))
        if not isinstance(v, (list, np.ndarray)):
            with pytest.raises(ValueError, match=next(iter(kw))):
                pipe.process_request(PROMPTS[0], max_tokens=2, temperature=TEMPERATURE, **kw)
    pipe.shutdown()
    assert ops.trace == [] and not ops.calls, (ops.trace, ops.calls)


def test_the_checks_return_one_float_per_prompt():
    assert check_repetition_penalty(1, 3) == [1.0] * 3 and check_repetition_penalty(np.float32(2.0), 2) == [2.0] * 2
    assert check_repetition_penalty([0.001, 2, np.float64(1.5)], 3) == [0.001, 2.0, 1.5]
    assert check_presence_penalty(-2, 2) == [-2.0] * 2 and check_presence_penalty(np.array([2.0, -0.5]), 2) == [2.0, -0.5]
    assert check_frequency_penalty(0, 1) == [0.0] and check_frequency_penalty((1, np.int64(-2)), 2) == [1.0, -2.0]
    with pytest.raises(ValueError, match=r"repetition_penalty must be a number in \(0, 2\]"):
        check_repetition_penalty(0.0, 2)
    with pytest.raises(ValueError, match=r"presence_penalty must be a number in \[-2, 2\]"):
        check_presence_penalty(2.5, 2)
    with pytest.raises(ValueError, match="2 frequency_penalty values for 3"):
        check_frequency_penalty([0.0, 0.0], 3)


NEUTRAL = [dict(repetition_penalty=1.0), dict(presence_penalty=0.0, frequency_penalty=0), dict(repetition_penalty=[1.0] * N),
           dict(repetition_penalty=1, presence_penalty=[0.0] * N, frequency_penalty=np.zeros(N)),
           dict(repetition_penalty=None, presence_penalty=None, frequency_penalty=None)]


@pytest.mark.parametrize("temperature", [TEMPERATURE, 0.0])
@pytest.mark.parametrize("name", NAMES)
def test_neutral_values_make_exactly_the_calls_made_before(name, temperature):
    sm, ops = _manager()
    stage = sm.get_stage(name)

    def run(**kw):
        stage.gen.manual_seed(int(stage.config.seed))
        ops.trace.clear()
        ops.calls.clear()
        out = stage.generate(prompts=PROMPTS, max_tokens=4, temperature=temperature, seed=SEEDS, stop_token_ids=(3, 4),
                             logit_bias={5: 1.0}, **kw)
        return out, list(ops.trace), dict(ops.calls)
    plain, trace, calls = run()
    names = [n for n, _ in trace]
    assert "logit_edit_rows" in names and not [n for n in names if "penalt" in n]
    for kw in NEUTRAL:
        same, t2, c2 = run(**kw)
        assert t2 == trace and c2 == calls, kw
        assert same[0] == plain[0] and all(a.tobytes() == b.tobytes() for a, b in zip(same[1], plain[1]))
    # one non-neutral value anywhere: one upload, one penalty call immediately behind every edit call, one commit per step
    _, t3, _ = run(frequency_penalty=[0.0] * (N - 1) + [0.5])
    names = [n for n, _ in t3]
    steps = stage.last_steps
    assert names.count("pack_penalties") == 1 and names.count("penalty_commit") == steps
    assert names.count("penalty_rows") == names.count("logit_edit_rows") == \
        (steps if name == NAMES[0] else steps * (stage.config.draft_len + 1))
    assert all(names[i - 1] == "logit_edit_rows" for i, n in enumerate(names) if n == "penalty_rows")


def test_neutral_values_through_the_pipeline_make_the_calls_made_before():
    out = []
    for kw in ({}, dict(repetition_penalty=1.0, presence_penalty=[0.0] * N, frequency_penalty=0.0)):
        sm, ops = _manager()
        pipe = AdaptiveSpeculativePipeline(sm, LogprobPredictor(), object(), PipelineConfig(lambda_value=30.0, stage_names=NAMES))
        res = pipe.batch_process(PROMPTS, max_tokens=4, temperature=TEMPERATURE, seeds=SEEDS, **kw)
        pipe.shutdown()
        out.append(([r.output for r in res], list(ops.trace)))
    assert out[0] == out[1] and out[0][1]
