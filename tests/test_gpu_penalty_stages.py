"""Repetition, presence and frequency penalties in Stage.generate on distributed.HipOps (serving/stages.py, PENALTIES): the
scenarios of tests/test_penalty_stages.py (tests/penalty_ref.py) through asd_penalty_rows / asd_penalty_commit and the real
samplers, on the three tiny stages of tests/stage_scenario.py, at the replay bars of tests/test_gpu_stages.py (2e-5) and
tests/greedy_ref.py (1e-5); and one two-stage run at the full vocabulary."""
import pytest
import torch

from tests.logit_edit_ref import SEEDS
from tests.penalty_ref import scenario_greedy, scenario_replay, scenario_rows_independent, scenario_signs_and_stops
from tests.stage_scenario import NAMES, PROMPTS, stage_configs

pytestmark = pytest.mark.gpu

ATOL = 2e-5        # tests/test_gpu_stages.py's bar for a kernel lp against the f64 value at its row


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs())


@pytest.fixture(scope="module")
def manager_f32():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs(dtype=torch.float32))      # (tests/penalty_ref.py, GREEDY: why float32)


@pytest.mark.parametrize("name", NAMES)
def test_edit_bits_arguments_state_and_replay(manager, name):
    worst = scenario_replay(manager.get_stage(name), atol=ATOL)
    print(f"[penalties] stage {name}: max |lp_drawn - f64| on the penalised rows = {worst:.3e}")
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_other_signs_and_a_row_that_ends_early(manager, name):
    scenario_signs_and_stops(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_row_b_is_the_call_that_gives_every_row_its_values(manager, name):
    scenario_rows_independent(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_greedy_text_is_the_teacher_forced_penalised_arg_max(manager_f32, name):
    share = scenario_greedy(manager_f32.get_stage(name))
    print(f"[penalties] stage {name}: {share:.3f} of the teacher-forced positions kept")
    manager_f32.ops.check_status()


def test_full_vocabulary_two_stage_run():
    """tiny(vocab=152064), B = 4, 8 tokens, two stages: all three penalties (one row neutral), seeds and a stop id, under the
    checks (a)-(c) of tests/penalty_ref.py::check_recorded; a row is cut into slices here."""
    from asd_amd.serving.stages import StageManager
    cfgs = stage_configs(vocab=152064)[:2]
    cfgs[1].model_seed = 1                              # a draft that differs from its target: rejected proposals as well
    sm = StageManager(cfgs)
    penalties = dict(repetition_penalty=[1.3, 1.0, 0.8, 1.1], presence_penalty=[0.5, 0.0, -1.0, 0.0],
                     frequency_penalty=[0.25, 0.0, 0.5, -0.5])
    stats = scenario_signs_and_stops(sm.get_stage(NAMES[1]), PROMPTS[:4], 8, SEEDS[:4], penalties)
    assert len(stats["n_tokens"]) == 4
    sm.ops.check_status()
