"""generate(typical_p= / eta_cutoff=) against the f64 teacher-forced reference of tests/teacher_forced_entropy_cut.py, on CPU: the
tiny float32 stages of tests/stage_scenario.py on the oracle twin of tests/entropy_cut_ref.py -- typical-p at stage 0, eta at the
verifying stages, per-prompt values with per-prompt temperatures -- and the negative control: the checker is handed another
typical_p than the call was made with and must fail."""
import pytest
import torch

import asd_amd
from asd_amd.serving.stages import StageManager
from tests.entropy_cut_ref import EntropyCutOracleOps
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import stage_configs
from tests.teacher_forced_entropy_cut import check_cut, run_scenario, scenarios
from tests.teacher_forced_ref import TeacherForcedError

LP_BAR = 1e-6      # the twin's log-probs are the f64 values at their rows rounded to f32
CASES = [(which, name) for which, (names, _) in sorted(scenarios().items()) for name in names]


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


@pytest.fixture(scope="module")
def manager():
    return StageManager(stage_configs(dtype=torch.float32), ops=EntropyCutOracleOps())


@pytest.mark.parametrize("which,name", CASES)
def test_scenarios(manager, which, name):
    run_scenario(manager.get_stage(name), which, LP_BAR)


@pytest.mark.parametrize("name,wrong", [("8b", 0.95), ("8b", 0.3), ("13b", 0.95)])
def test_control_the_checker_is_given_the_wrong_typical_p(manager, name, wrong):
    stage = manager.get_stage(name)
    kw = scenarios()["typical"][1]
    out = stage.generate(**kw)
    check_cut(stage, kw, out, LP_BAR, "right value")                         # the call itself is in order ...
    with pytest.raises(TeacherForcedError, match=r"removed by the row's cut|teacher-forced value lies in"):
        check_cut(stage, kw, out, LP_BAR, "control", cut_kw=dict(typical_p=wrong))


def test_control_a_cut_that_is_not_applied_fails(manager):
    """The loop's cut call is dropped: texts and log-probs are those of the uncut distribution."""
    stage = manager.get_stage("13b")
    kw = scenarios()["eta"][1]
    stage.ops.entropy_cut_rows = lambda logits, cut: logits
    try:
        out = stage.generate(**kw)
    finally:
        del stage.ops.entropy_cut_rows
    with pytest.raises(TeacherForcedError):
        check_cut(stage, kw, out, LP_BAR, "control")
