"""generate(typical_p= / eta_cutoff=) on distributed.HipOps against the f64 teacher-forced reference of
tests/teacher_forced_entropy_cut.py: the scenarios of tests/test_teacher_forced_entropy_cut.py through asd_entropy_cut_rows and
the real samplers, on the tiny float32 stages of tests/stage_scenario.py."""
import pytest
import torch

from tests.stage_scenario import stage_configs
from tests.teacher_forced_entropy_cut import run_scenario, scenarios

pytestmark = pytest.mark.gpu

LP_BAR = 2e-5      # the project's bar for a kernel log-prob against f64 at its own row
# typical-p at stage 0 and eta at the verifying stages; the per-prompt scenario runs on the twin, and on the GPU at the step level
# (tests/test_gpu_entropy_cut_stages.py)
CASES = [(which, name) for which in ("typical", "eta") for name in scenarios()[which][0]]


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs(dtype=torch.float32))


@pytest.mark.parametrize("which,name", CASES)
def test_scenarios(manager, which, name):
    run_scenario(manager.get_stage(name), which, LP_BAR)
    manager.ops.check_status()
