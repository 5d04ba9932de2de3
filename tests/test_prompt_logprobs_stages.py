"""prompt_logprobs in Stage.generate and the pipeline, on CPU: the three tiny stages of tests/stage_scenario.py at vocabulary 64
on the oracle twin of tests/prompt_logprobs_ref.py, whose prompt_logprobs is the numpy reference of asd_prompt_logprobs.  The
scenarios are those tests/test_gpu_prompt_logprobs_stages.py runs on the kernel."""
import pytest

import asd_amd
from asd_amd.serving.stages import StageManager
from tests.oracle_backend import OracleBackend
from tests.prompt_logprobs_ref import (VOCAB, PromptOracleOps, scenario_call_trace, scenario_composition, scenario_pipeline,
                                       scenario_same_bits, scenario_values)
from tests.stage_scenario import NAMES, PROMPTS, stage_configs


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def _manager(**kw):
    ops = PromptOracleOps()
    return StageManager(stage_configs(vocab=VOCAB, **kw), ops=ops), ops


@pytest.mark.parametrize("n", [0, 1, 8])
@pytest.mark.parametrize("name", NAMES)
def test_stats_hold_the_reference_numbers_of_the_kept_prefill(name, n):
    sm, _ = _manager()
    scenario_values(sm.get_stage(name), n)


@pytest.mark.parametrize("name", NAMES)
def test_greedy_calls_score_the_prompt_too(name):
    sm, _ = _manager()
    scenario_values(sm.get_stage(name), 2, temperature=0.0)


@pytest.mark.parametrize("name", NAMES)
def test_generated_tokens_keep_their_bits(name):
    sm, _ = _manager()
    scenario_same_bits(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_call_trace_gains_exactly_one_call(name):
    sm, ops = _manager()
    stage = sm.get_stage(name)
    scenario_call_trace(stage)
    # the configuration's value is the default, None at the call takes it, and 0 is ON
    sm2, ops2 = _manager(prompt_logprobs=0)
    _, _, stats = sm2.get_stage(name).generate(prompts=PROMPTS, max_tokens=2, temperature=0.0)
    assert [n for n, _ in ops2.trace].count("prompt_logprobs") == 1
    assert "prompt_ranks" in stats and "prompt_top_logprobs" not in stats


@pytest.mark.parametrize("name", NAMES)
def test_masks_edits_and_penalties_leave_the_prompt_numbers_alone(name):
    sm, _ = _manager()
    scenario_composition(sm.get_stage(name))


def test_pipeline_carries_the_entries():
    sm, ops = _manager()
    scenario_pipeline(sm)
    assert "prompt_logprobs" in [n for n, _ in ops.trace]
