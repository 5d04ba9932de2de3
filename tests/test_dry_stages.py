"""DRY in Stage.generate on CPU: the four scenarios of tests/dry_ref.py on the three tiny stages of tests/stage_scenario.py at
vocabulary 64, on the oracle twin whose dry_rows is the plain reference of asd_dry_rows; and check_dry's ValueErrors.  The
scenarios are those tests/test_gpu_dry_stages.py runs on the kernel."""
import pytest

import asd_amd
from asd_amd.minimal_adaptive_decoder import SimpleTokenizer
from asd_amd.serving.stage_args import check_dry
from asd_amd.serving.stages import StageManager
from tests.dry_ref import (VOCAB, DryOracleOps, scenario_breaker, scenario_multiplier_zero, scenario_per_prompt,
                           scenario_strict_is_bigram_ban)
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import NAMES, stage_configs

SCENARIOS = [scenario_strict_is_bigram_ban, scenario_per_prompt, scenario_multiplier_zero, scenario_breaker]


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__)
@pytest.mark.parametrize("name", NAMES)
def test_scenario(name, scenario):
    scenario(StageManager(stage_configs(vocab=VOCAB), ops=DryOracleOps()).get_stage(name))


GOOD = dict(multiplier=0.8, base=1.75, allowed_length=2, dry_range=0, breakers=None)


@pytest.mark.parametrize("bad", [
    dict(multiplier=True), dict(multiplier=float("nan")), dict(multiplier=-0.1), dict(multiplier=float("inf")), dict(multiplier="1"),
    dict(multiplier=[0.8, 0.8]), dict(base=True), dict(base=float("nan")), dict(base=0.99), dict(base=float("inf")),
    dict(allowed_length=0), dict(allowed_length=65), dict(allowed_length=2.0), dict(allowed_length=True), dict(dry_range=-1),
    dict(dry_range=1.5), dict(dry_range=[0, 0, 0, 0]), dict(breakers=list(range(33))), dict(breakers=[VOCAB]), dict(breakers=[-1]),
    dict(breakers=["two words"]), dict(breakers=[""]), dict(breakers=3), dict(breakers=[1.0])], ids=str)
def test_check_dry_raises(bad):
    with pytest.raises(ValueError):
        check_dry(**{**GOOD, **bad}, n=3, vocab=VOCAB, tokenizer=SimpleTokenizer())

