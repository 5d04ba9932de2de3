"""Mirostat v2 in Stage.generate on CPU: the scenarios of tests/mirostat_ref.py on the three tiny stages of
tests/stage_scenario.py at vocabulary 64, on the oracle twin whose mirostat_rows is the f64 reference of asd_mirostat_rows.  The
scenarios are those tests/test_gpu_mirostat_stages.py runs on the kernels."""
import pytest

import asd_amd
from asd_amd.serving.stages import StageManager
from tests.mirostat_ref import CONFIG, VOCAB, MirostatOracleOps, scenario_configured, scenario_greedy, scenario_per_prompt
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import NAMES, stage_configs

SCENARIOS = [scenario_configured, scenario_per_prompt, scenario_greedy]


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__)
@pytest.mark.parametrize("name", NAMES)
def test_scenario(name, scenario):
    scenario(StageManager(stage_configs(vocab=VOCAB, **CONFIG), ops=MirostatOracleOps()).get_stage(name))
