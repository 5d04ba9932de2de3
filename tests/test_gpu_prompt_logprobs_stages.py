"""prompt_logprobs in Stage.generate on distributed.HipOps (serving/stages.py, PROMPT LOG-PROBS): the scenarios of
tests/test_prompt_logprobs_stages.py (tests/prompt_logprobs_ref.py) through asd_prompt_logprobs and the real samplers, on the
three tiny float32 stages of tests/stage_scenario.py at vocabulary 64; and one two-stage run at the full vocabulary."""
import pytest
import torch

from tests.logit_edit_ref import SEEDS, run_kept
from tests.prompt_logprobs_ref import (VOCAB, check_stats, check_values, scenario_call_trace, scenario_composition, scenario_pipeline,
                                       scenario_same_bits, scenario_values)
from tests.stage_scenario import NAMES, PROMPTS, TEMPERATURE, stage_configs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs(vocab=VOCAB, dtype=torch.float32))


@pytest.mark.parametrize("n", [0, 1, 8])
@pytest.mark.parametrize("name", NAMES)
def test_stats_hold_the_reference_numbers_of_the_kept_prefill(manager, name, n):
    scenario_values(manager.get_stage(name), n)
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_greedy_calls_score_the_prompt_too(manager, name):
    scenario_values(manager.get_stage(name), 2, temperature=0.0)
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_generated_tokens_keep_their_bits(manager, name):
    scenario_same_bits(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_call_trace_gains_exactly_one_call(manager, name):
    scenario_call_trace(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_masks_edits_and_penalties_leave_the_prompt_numbers_alone(manager, name):
    scenario_composition(manager.get_stage(name))
    manager.ops.check_status()


def test_pipeline_carries_the_entries(manager):
    scenario_pipeline(manager)
    manager.ops.check_status()


def test_full_vocabulary_two_stage_run():
    """tiny(vocab=152064), B = 4, 8 tokens, two bf16 stages: the verifying stage's prompt log-probs, ranks and tables against f64 on
    the kept prefill logits (ids and ranks exact, log-probs within LP_ATOL), and stage 0's likewise."""
    from asd_amd.serving.stages import StageManager
    cfgs = stage_configs(vocab=152064)[:2]
    cfgs[1].model_seed = 1
    assert cfgs[1].dtype == torch.bfloat16
    sm = StageManager(cfgs)
    for name in NAMES[:2]:
        stage = sm.get_stage(name)
        _, _, stats = run_kept(stage, prompts=PROMPTS[:4], max_tokens=8, temperature=TEMPERATURE, seed=SEEDS[:4], prompt_logprobs=5)
        assert stage.prompt_inputs["logits"].dtype == torch.bfloat16 and stage.prompt_inputs["logits"].shape[2] == 152064
        check_stats(stage, stats, 5, PROMPTS[:4])
        check_values(stage, stats, 5, PROMPTS[:4])
    sm.ops.check_status()
