"""Shaping's argument checks, all without a GPU: check_logit_shapes, the records pack_logit_shape would upload, and
Stage.generate, which refuses before the prompts are encoded and before any ops call.  (The launcher's status codes run in
tools/asan_host_args.cpp.)"""
import numpy as np
import pytest

import asd_amd
from asd_amd import kernels as K
from asd_amd.serving.stage_args import check_logit_shapes
from asd_amd.serving.stages import StageManager
from tests.mirostat_ref import VOCAB, MirostatOracleOps
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import NAMES, PROMPTS, stage_configs

NAN, INF = float("nan"), float("inf")


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def test_check_logit_shapes_and_the_records():
    assert check_logit_shapes(0, 1, 0, 1, 2) == [(0, 0.0, 0.0)] * 2
    assert check_logit_shapes([0.3, 0, 0], 2.0, [0, 0.5, 0], [1, 3, 1], 3, True, True) == [(1, float(np.float32(0.3)), 2.0), (2, 0.5, 3.0), (0, 0.0, 0.0)]
    rec = K.check_logit_shape_rows([0.7, 0.7, 0.7], [1, 2, 0], [0.3, 0.1, 9.0], [0.1, 1.1, 9.0])
    assert rec.tolist() == [(1, np.float32(0.7), np.float32(0.3), np.float32(0.1)), (2, 0.0, np.float32(0.1), np.float32(1.1)),
                            (0, 0.0, 0.0, 0.0)]                                  # the f32-rounded values; an off row holds zeros
    for bad in ([0.7], [1], [0.7], [1.0]), ([0.7], [3], [0.3], [1.0]), ([0.7], [2], [0.3], [3.5]), ([NAN], [1], [0.3], [1.0]):
        with pytest.raises(ValueError):
            K.check_logit_shape_rows(*bad)
    with pytest.raises(ValueError, match="smoothing_curve"):                     # a bad configuration: when the stage is built
        StageManager(stage_configs(vocab=VOCAB, target_smoothing_curve=4.0), ops=MirostatOracleOps())


@pytest.mark.parametrize("name", NAMES)
def test_generate_refuses_before_encoding(name):
    ops = MirostatOracleOps()
    stage = StageManager(stage_configs(vocab=VOCAB, top_p=1.0), ops=ops).get_stage(name)
    encoded = []
    stage._encode = lambda prompts, _orig=stage._encode: (encoded.append(1), _orig(prompts))[1]
    n = len(PROMPTS)
    for kw, match in ((dict(dynatemp_range=0.3, smoothing_factor=0.5), "not built"), (dict(dynatemp_range=0.3, mirostat_tau=5.0), "Mirostat"),
                      (dict(smoothing_factor=0.5, mirostat_tau=5.0), "Mirostat"), (dict(dynatemp_exponent=2.0), "dynatemp_exponent"),
                      (dict(smoothing_curve=2.0), "smoothing_curve"), (dict(smoothing_factor=0.5, dynatemp_exponent=2.0), "dynatemp_exponent"),
                      (dict(dynatemp_range=True), "dynatemp_range"), (dict(smoothing_factor=NAN), "smoothing_factor"),
                      (dict(dynatemp_range=-0.1), "dynatemp_range"), (dict(dynatemp_range=INF), "dynatemp_range"),
                      (dict(dynatemp_range="0.3"), "dynatemp_range"), (dict(dynatemp_range=0.3, dynatemp_exponent=0.0), "dynatemp_exponent"),
                      (dict(smoothing_factor=0.5, smoothing_curve=0.5), "smoothing_curve"),
                      (dict(smoothing_factor=0.5, smoothing_curve=3.5), "smoothing_curve"),
                      (dict(dynatemp_range=[0.3] * (n - 1)), "dynatemp_range")):
        for temperature in (0.7, 0.0):                                       # greedy ignores the values, not their errors
            with pytest.raises(ValueError, match=match):
                stage.generate(prompts=PROMPTS, max_tokens=2, temperature=temperature, **kw)
    for kw in (dict(temperature=0.7, dynatemp_range=0.7), dict(temperature=[0.7] * (n - 1) + [0.2], dynatemp_range=0.25)):
        with pytest.raises(ValueError, match="strictly below"):              # a range that reaches the row's temperature
            stage.generate(prompts=PROMPTS, max_tokens=2, **kw)
    assert not encoded and not ops.trace
