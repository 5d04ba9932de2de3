"""Guided decoding in Stage.generate on distributed.HipOps (serving/stages.py, GUIDED DECODING): the scenarios of
tests/test_fsm_stages.py (tests/fsm_ref.py) through asd_fsm_mask_rows / asd_fsm_advance / asd_fsm_commit and the real samplers,
on the three tiny stages of tests/stage_scenario.py; and one two-stage run at the full vocabulary."""
import pytest

from tests.fsm_ref import (CHOICES, OTHER_CHOICES, STOP, RefAutomaton, check_choice_rows, check_kept_masks, run_kept_recorded, scenario_call_trace,
                           scenario_choices, scenario_composition, scenario_kept_steps, scenario_logprobs, scenario_rows_independent)
from tests.logit_edit_ref import SEEDS
from tests.stage_scenario import MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, stage_configs

pytestmark = pytest.mark.gpu

LP_BAR = 2e-5      # tests/test_gpu_stages.py's bar for a kernel lp against the f64 value at its row


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs())


@pytest.mark.parametrize("greedy", [True, False], ids=["greedy", "sampled"])
@pytest.mark.parametrize("name", NAMES)
def test_every_row_is_one_choice_and_one_stop_id(manager, name, greedy):
    scenario_choices(manager.get_stage(name), greedy)
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_an_unguided_row_is_the_call_without_guidance(manager, name):
    scenario_rows_independent(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_every_kept_step_is_masked_by_the_replayed_state(manager, name):
    scenario_kept_steps(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_returned_logprobs_match_the_f64_restricted_distribution(manager, name):
    scenario_logprobs(manager.get_stage(name), LP_BAR)
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_composes_with_allow_list_bias_penalties_bad_words_and_top_n(manager, name):
    scenario_composition(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_call_trace(manager, name):
    scenario_call_trace(manager.get_stage(name))
    manager.ops.check_status()


def test_full_vocabulary_two_stage_run():
    """tiny(vocab=152064), B = 4, two stages, a draft that differs from its target (rejected proposals as well): one list of
    choices per row, one row free, under the replay of tests/fsm_ref.py::check_kept_masks, draft proposals' logits included."""
    from asd_amd.serving.stages import StageManager
    V = 152064
    cfgs = stage_configs(vocab=V)[:2]
    cfgs[1].model_seed = 1
    sm = StageManager(cfgs)
    stage = sm.get_stage(NAMES[1])
    big = [(V - 1, 4096, 131072), (V - 1, 4095), (151000, 0, 65536, 31, 32)]
    rows = [big, CHOICES, None, OTHER_CHOICES]
    (texts, _, stats), calls = run_kept_recorded(stage, prompts=PROMPTS[:4], max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS[:4],
                                                 stop_token_ids=[STOP], guided_choice_per_prompt=rows)
    check_choice_rows(texts, stats, rows)
    autos = [None if r is None else RefAutomaton.of_choices(r, [STOP], V) for r in rows]
    assert check_kept_masks(stage, texts, autos, PROMPTS[:4], calls) >= 3 * 2 * 2
    sm.ops.check_status()
