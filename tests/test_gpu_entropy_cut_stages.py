"""typical_p / epsilon_cutoff / eta_cutoff in Stage.generate on distributed.HipOps (serving/stages.py, ENTROPY CUTS): the
scenarios of tests/test_entropy_cut_stages.py (tests/entropy_cut_ref.py) through asd_entropy_cut_rows and the real samplers, on
the three tiny float32 stages of tests/stage_scenario.py at vocabulary 64."""
import pytest
import torch

from tests.entropy_cut_ref import (ROW_TEMPERATURES, VOCAB, scenario_allow_list, scenario_configured, scenario_greedy, scenario_mode,
                                   scenario_per_prompt, scenario_tables_and_stats, scenario_top_p_behind)
from tests.stage_scenario import NAMES, stage_configs

pytestmark = pytest.mark.gpu

MODES = [("typical_p", 0.5), ("epsilon_cutoff", 0.03), ("eta_cutoff", 0.05)]


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs(vocab=VOCAB, dtype=torch.float32))


@pytest.mark.parametrize("key,value", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_each_mode_on_its_own(manager, name, key, value):
    scenario_mode(manager.get_stage(name), key, value)
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_per_prompt_values_with_one_row_off(manager, name):
    scenario_per_prompt(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_top_p_acts_on_the_survivors(manager, name):
    scenario_top_p_behind(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_tables_and_statistics_describe_the_cut_row(manager, name):
    scenario_tables_and_stats(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_allow_list_in_front_of_the_cut(manager, name):
    scenario_allow_list(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("key,value", MODES[:2])
def test_configured_cut_is_the_draft_side_of_a_verifying_stage(key, value):
    from asd_amd.serving.stages import StageManager
    sm = StageManager(stage_configs(vocab=VOCAB, dtype=torch.float32, **{key: value}))
    for name in NAMES:
        scenario_configured(sm.get_stage(name), key, value)
    sm.ops.check_status()


def test_configured_draft_cut_takes_per_row_temperatures():
    from asd_amd.serving.stages import StageManager
    sm = StageManager(stage_configs(vocab=VOCAB, dtype=torch.float32, typical_p=0.5))
    for name in NAMES:
        scenario_configured(sm.get_stage(name), "typical_p", 0.5, temperature=ROW_TEMPERATURES)
    sm.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_greedy_makes_no_call(manager, name):
    scenario_greedy(manager.get_stage(name))
    manager.ops.check_status()
