"""DRY in Stage.generate on distributed.HipOps (serving/stages.py, DRY): the scenarios of tests/test_dry_stages.py
(tests/dry_ref.py) through asd_dry_rows and the real samplers, on the three tiny float32 stages at vocabulary 64."""
import pytest
import torch

from tests.dry_ref import VOCAB
from tests.stage_scenario import NAMES, stage_configs
from tests.test_dry_stages import SCENARIOS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs(vocab=VOCAB, dtype=torch.float32))


@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__)
@pytest.mark.parametrize("name", NAMES)
def test_scenario(manager, name, scenario):
    scenario(manager.get_stage(name))
    manager.ops.check_status()
