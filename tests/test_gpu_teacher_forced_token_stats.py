"""generate(token_stats=True) on distributed.HipOps against the f64 teacher-forced reference of
tests/teacher_forced_token_stats.py: the scenarios of tests/test_teacher_forced_token_stats.py through asd_token_stats and the
real samplers, on the three tiny float32 stages of tests/stage_scenario.py."""
import pytest
import torch

from tests.stage_scenario import NAMES, stage_configs
from tests.teacher_forced_token_stats import run_scenario, scenarios

pytestmark = pytest.mark.gpu

LP_BAR = 2e-5                               # tests/test_gpu_stages.py's bar for a kernel lp against the f64 value at its row
H_BAR = lambda H: 1e-4 + 1e-5 * H           # noqa: E731  (tests/test_gpu_token_stats.py's bar for the kernel's entropy)


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs(dtype=torch.float32))


@pytest.mark.parametrize("which", sorted(scenarios(8)))
@pytest.mark.parametrize("name", NAMES)
def test_scenarios(manager, name, which):
    run_scenario(manager.get_stage(name), which, LP_BAR, H_BAR)
    manager.ops.check_status()
