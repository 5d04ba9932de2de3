"""The watermark on CPU: check_watermark's and Stage.generate's ValueErrors (before the prompts are encoded and before any ops
call), the records pack_watermark would upload, and the stage scenario of tests/watermark_ref.py on the oracle twin -- the one
tests/test_gpu_watermark.py runs on the kernels."""
import numpy as np
import pytest

import asd_amd
from asd_amd import kernels as K
from asd_amd.serving.stages import StageManager
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import NAMES, PROMPTS, stage_configs
from tests.watermark_ref import WatermarkOracleOps, scenario_every_token_green

VOCAB, N = 64, len(PROMPTS)


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


@pytest.mark.parametrize("kw", [
    dict(watermark_key=True), dict(watermark_key=-1), dict(watermark_key=2 ** 64), dict(watermark_key=1.0), dict(watermark_key="7"),
    dict(watermark_key=[1] * (N - 1)), dict(watermark_delta=1.0), dict(watermark_gamma=0.5), dict(watermark_context=2),
    dict(watermark_key=[None] * N, watermark_delta=1.0), dict(watermark_key=1, watermark_delta=0.0),
    dict(watermark_key=1, watermark_delta=100.5), dict(watermark_key=1, watermark_delta=float("nan")),
    dict(watermark_key=1, watermark_delta=True), dict(watermark_key=1, watermark_delta=[2.0] * (N + 1)),
    dict(watermark_key=1, watermark_gamma=0.0), dict(watermark_key=1, watermark_gamma=1.0), dict(watermark_key=1, watermark_gamma="0.5"),
    dict(watermark_key=1, watermark_context=0), dict(watermark_key=1, watermark_context=4), dict(watermark_key=1, watermark_context=1.0)], ids=str)
def test_generate_refuses_before_encoding(kw):
    ops = WatermarkOracleOps()
    stage = StageManager(stage_configs(vocab=VOCAB), ops=ops).get_stage(NAMES[1])
    stage._encode = None                                                         # (reaching it would raise TypeError)
    for temperature in (0.7, 0.0):
        with pytest.raises(ValueError, match="watermark"):
            stage.generate(prompts=PROMPTS, max_tokens=2, temperature=temperature, **kw)
    assert not ops.trace
    with pytest.raises(ValueError, match="watermark_gamma"):                     # a bad configuration: when the stage is built
        StageManager(stage_configs(vocab=VOCAB, watermark_gamma=1.5), ops=ops)


def test_the_records():
    rec, first = K.check_watermark_rows([2 ** 64 - 2, None, 5], [2.0, 9.0, 0.5], [0.25, 0.5, 1e-9], [1, 2, 3], [3, 0, 1], 3)
    assert rec.tolist() == [(0xFFFFFFFE, 0xFFFFFFFF, 2.0, 16384 | 1 << 16), (0, 0, 0.0, 0), (5, 0, 0.5, 1 | 3 << 16)] and first == [0, 3, 2]
    assert K.watermark_threshold(0.99999999) == 65535
    for bad in ([1], [np.inf], [0.5], [1], [0]), ([1], [2.0], [0.5], [4], [0]), ([1], [2.0], [0.5], [1], [4]), ([1, 2], [2.0], [0.5], [1], [0]):
        with pytest.raises(ValueError):
            K.check_watermark_rows(*bad, 3)


@pytest.mark.parametrize("greedy", [False, True], ids=["sampled", "greedy"])
@pytest.mark.parametrize("name", NAMES[:2])
def test_scenario_on_the_twin(name, greedy):
    scenario_every_token_green(StageManager(stage_configs(vocab=VOCAB), ops=WatermarkOracleOps()).get_stage(name), greedy)
