"""generate(token_stats=True) against the f64 teacher-forced reference of tests/teacher_forced_token_stats.py, on CPU: the three
tiny float32 stages of tests/stage_scenario.py on the oracle twin of tests/token_stats_ref.py, and two negative controls: defects
of the plumbing that leave the loop's own record self-consistent."""
import pytest
import torch

import asd_amd
from asd_amd.serving.stages import StageManager
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import NAMES, stage_configs
from tests.teacher_forced_ref import TeacherForcedError
from tests.teacher_forced_token_stats import check_token_stats, run_scenario, scenarios
from tests.token_stats_ref import TokenStatsOracleOps

LP_BAR = 1e-6      # the twin's figures are the f64 values at their rows rounded to f32
H_BAR = lambda H: 1e-6      # noqa: E731


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


@pytest.fixture(scope="module")
def manager():
    return StageManager(stage_configs(dtype=torch.float32), ops=TokenStatsOracleOps())


@pytest.mark.parametrize("which", sorted(scenarios(8)))
@pytest.mark.parametrize("name", NAMES)
def test_scenarios(manager, name, which):
    run_scenario(manager.get_stage(name), which, LP_BAR, H_BAR)


@pytest.mark.parametrize("name", NAMES[1:])
def test_control_statistics_of_the_row_in_front(manager, name):
    """The pass is handed the step's rows shifted by one (row j holds row j - 1's logits): the record stays self-consistent, and
    the figures are those of another position."""
    stage = manager.get_stage(name)
    kw = scenarios(stage.shape.vocab)["plain"]
    orig = stage.ops.token_stats
    stage.ops.token_stats = lambda logits, *a, **k: orig(torch.roll(logits, 1, 1) if logits.dim() == 3 else logits, *a, **k)
    try:
        out = stage.generate(**kw)
    finally:
        del stage.ops.token_stats
    with pytest.raises(TeacherForcedError, match=r"entropy|rank|top-N"):
        check_token_stats(stage, kw, out, LP_BAR, H_BAR, "control")


@pytest.mark.parametrize("name", NAMES)
def test_control_statistics_at_temperature_one(manager, name):
    stage = manager.get_stage(name)
    kw = scenarios(stage.shape.vocab)["plain"]
    orig = stage.ops.token_stats
    stage.ops.token_stats = lambda *a, **k: orig(*a, **dict(k, inv_temperature=1.0))
    try:
        out = stage.generate(**kw)
    finally:
        del stage.ops.token_stats
    with pytest.raises(TeacherForcedError, match=r"entropy"):
        check_token_stats(stage, kw, out, LP_BAR, H_BAR, "control")
