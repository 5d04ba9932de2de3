"""token_stats' argument checks (serving/stage_args.py::_check_token_stats, Stage.generate): anything but None or a bool raises
ValueError before the prompts are encoded and before any ops call; None takes the configuration's value."""
import pytest

import asd_amd
from asd_amd.serving.stage_args import _check_token_stats
from asd_amd.serving.stages import StageManager
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import NAMES, PROMPTS, stage_configs
from tests.token_stats_ref import KEYS, VOCAB, TokenStatsOracleOps

BAD = [1, 0, "yes", "", [True], (False,), 1.0, {"on": True}]


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def test_check_token_stats():
    assert _check_token_stats(None) is None and _check_token_stats(True) is True and _check_token_stats(False) is False
    for v in BAD:
        with pytest.raises(ValueError, match="token_stats"):
            _check_token_stats(v)


@pytest.mark.parametrize("name", NAMES)
def test_generate_refuses_before_encoding(name):
    ops = TokenStatsOracleOps()
    stage = StageManager(stage_configs(vocab=VOCAB), ops=ops).get_stage(name)
    encoded = []
    stage._encode = lambda prompts, _orig=stage._encode: (encoded.append(1), _orig(prompts))[1]
    for v in BAD:
        with pytest.raises(ValueError, match="token_stats"):
            stage.generate(prompts=PROMPTS, max_tokens=2, temperature=0.0, token_stats=v)
    assert not encoded and not ops.trace
    stage.generate(prompts=PROMPTS, max_tokens=2, temperature=0.0, token_stats=True)
    assert encoded


def test_none_takes_the_configuration_value():
    for value in (False, True):
        stage = StageManager(stage_configs(vocab=VOCAB, token_stats=value), ops=TokenStatsOracleOps()).get_stage(NAMES[1])
        stats = stage.generate(prompts=PROMPTS, max_tokens=2, temperature=0.0, token_stats=None)[2]
        assert all((k in stats) == value for k in KEYS)
        stats = stage.generate(prompts=PROMPTS, max_tokens=2, temperature=0.0, token_stats=not value)[2]
        assert all((k in stats) == (not value) for k in KEYS)
    with pytest.raises(ValueError, match="token_stats"):                            # a bad configuration value is refused too
        StageManager(stage_configs(vocab=VOCAB, token_stats=1), ops=TokenStatsOracleOps()).get_stage(NAMES[0]).generate(
            prompts=PROMPTS, max_tokens=2, temperature=0.0)
