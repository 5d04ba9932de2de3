"""no_repeat_ngram_size in Stage.generate on distributed.HipOps (serving/stages.py, NO REPEAT N-GRAM): the scenarios of
tests/test_no_repeat_ngram_stages.py (tests/ngram_ref.py) through asd_no_repeat_ngram_rows and the real samplers, on the three
tiny float32 stages of tests/stage_scenario.py at vocabulary 64; and one two-stage run at the full vocabulary."""
import pytest
import torch

from tests.logit_edit_ref import SEEDS, run_kept
from tests.ngram_ref import (VOCAB, check_kept_bans, check_no_repeat, real_ids, scenario_call_trace, scenario_composition,
                             scenario_greedy, scenario_per_prompt, scenario_pipeline, scenario_prompt_counts, scenario_sampled)
from tests.stage_scenario import NAMES, PROMPTS, TEMPERATURE, stage_configs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs(vocab=VOCAB, dtype=torch.float32))


@pytest.mark.parametrize("n", [2, 3, 1])
@pytest.mark.parametrize("name", NAMES)
def test_greedy_rows_leave_the_plain_run_at_its_first_repeat_and_repeat_nothing(manager, name, n):
    scenario_greedy(manager.get_stage(name), n)
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_sampled_rows_repeat_nothing_and_every_kept_step_has_the_reference_bans(manager, name):
    scenario_sampled(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_row_b_is_the_call_that_gives_every_row_its_n(manager, name):
    scenario_per_prompt(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_the_prompt_counts_and_the_padding_does_not(manager, name):
    scenario_prompt_counts(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_composes_with_allow_list_bias_penalties_bad_words_top_n_and_a_stop_id(manager, name):
    scenario_composition(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_call_trace(manager, name):
    scenario_call_trace(manager.get_stage(name))
    manager.ops.check_status()


def test_pipeline_on_the_stages_repeats_nothing(manager):
    scenario_pipeline(manager)
    manager.ops.check_status()


def test_full_vocabulary_two_stage_run():
    """tiny(vocab=152064), B = 4, 8 tokens, two stages, a draft that differs from its target (rejected proposals as well), n = 1:
    no row takes a token of its prompt or one it has produced, under the replay of tests/ngram_ref.py::check_kept_bans."""
    from asd_amd.serving.stages import StageManager
    cfgs = stage_configs(vocab=152064)[:2]
    cfgs[1].model_seed = 1
    sm = StageManager(cfgs)
    stage = sm.get_stage(NAMES[1])
    kw = dict(prompts=PROMPTS[:4], max_tokens=8, temperature=TEMPERATURE, seed=SEEDS[:4])
    texts, _, _ = run_kept(stage, no_repeat_ngram_size=1, **kw)
    check_no_repeat(real_ids(stage, PROMPTS[:4])[0], texts, [1] * 4)
    assert check_kept_bans(stage, texts, [1] * 4, PROMPTS[:4]) > 0
    sm.ops.check_status()
