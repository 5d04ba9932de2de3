"""Mirostat v2 in Stage.generate on distributed.HipOps (serving/stages.py, MIROSTAT): the scenarios of
tests/test_mirostat_stages.py (tests/mirostat_ref.py) through asd_mirostat_rows, asd_mirostat_commit and the real samplers, on
the three tiny float32 stages at vocabulary 64."""
import pytest
import torch

from tests.mirostat_ref import CONFIG, VOCAB
from tests.stage_scenario import NAMES, stage_configs
from tests.test_mirostat_stages import SCENARIOS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs(vocab=VOCAB, dtype=torch.float32, **CONFIG))


@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__)
@pytest.mark.parametrize("name", NAMES)
def test_scenario(manager, name, scenario):
    scenario(manager.get_stage(name))
    manager.ops.check_status()
