"""typical_p / epsilon_cutoff / eta_cutoff in Stage.generate, on CPU: the three tiny stages of tests/stage_scenario.py at
vocabulary 64 on the oracle twin of tests/entropy_cut_ref.py, whose entropy_cut_rows is the numpy reference of
asd_entropy_cut_rows.  The scenarios are those tests/test_gpu_entropy_cut_stages.py runs on the kernel."""
import pytest

import asd_amd
from asd_amd.serving.stages import StageManager
from tests.entropy_cut_ref import (ROW_TEMPERATURES, VOCAB, EntropyCutOracleOps, scenario_allow_list, scenario_configured, scenario_greedy,
                                   scenario_mode, scenario_per_prompt, scenario_tables_and_stats, scenario_top_p_behind)
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import NAMES, PROMPTS, stage_configs

MODES = [("typical_p", 0.5), ("epsilon_cutoff", 0.03), ("eta_cutoff", 0.05)]


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def _manager(**kw):
    ops = EntropyCutOracleOps()
    return StageManager(stage_configs(vocab=VOCAB, **kw), ops=ops), ops


@pytest.mark.parametrize("key,value", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_each_mode_on_its_own(name, key, value):
    sm, _ = _manager()
    scenario_mode(sm.get_stage(name), key, value)


@pytest.mark.parametrize("name", NAMES)
def test_per_prompt_values_with_one_row_off(name):
    sm, _ = _manager()
    scenario_per_prompt(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_top_p_acts_on_the_survivors(name):
    sm, _ = _manager()
    scenario_top_p_behind(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_tables_and_statistics_describe_the_cut_row(name):
    sm, _ = _manager()
    scenario_tables_and_stats(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_allow_list_in_front_of_the_cut(name):
    sm, _ = _manager()
    scenario_allow_list(sm.get_stage(name))


@pytest.mark.parametrize("key,value", MODES[:2])
@pytest.mark.parametrize("name", NAMES)
def test_configured_cut_is_the_draft_side_of_a_verifying_stage(name, key, value):
    sm, _ = _manager(**{key: value})
    scenario_configured(sm.get_stage(name), key, value)


@pytest.mark.parametrize("name", NAMES)
def test_configured_draft_cut_takes_per_row_temperatures(name):
    sm, _ = _manager(typical_p=0.5)
    scenario_configured(sm.get_stage(name), "typical_p", 0.5, temperature=ROW_TEMPERATURES)


@pytest.mark.parametrize("name", NAMES)
def test_greedy_makes_no_call(name):
    sm, _ = _manager()
    scenario_greedy(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_off_makes_the_calls_made_before(name):
    """None, and the off values 0 / 1, make exactly the default call's ops calls."""
    sm, ops = _manager()
    stage = sm.get_stage(name)
    kw = dict(prompts=PROMPTS, max_tokens=4, temperature=0.7, seed=[1, 2, 3, 4, 5])
    stage.generate(**kw)
    base = [n for n, _ in ops.trace]
    for extra in (dict(typical_p=None), dict(typical_p=1.0), dict(typical_p=0.0, epsilon_cutoff=0.0, eta_cutoff=0.0)):
        del ops.trace[:]
        stage.generate(**extra, **kw)
        assert [n for n, _ in ops.trace] == base and "entropy_cut_rows" not in base


def test_pipeline_config_hands_the_values_on():
    from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
    from tests.stage_scenario import LogprobPredictor
    sm, ops = _manager()
    for cfg_kw in ({}, dict(typical_p=0.5), dict(eta_cutoff=0.05)):
        cfg = PipelineConfig(lambda_value=100.0, stop_rule="full", stage_names=NAMES, **cfg_kw)
        pipe = AdaptiveSpeculativePipeline(sm, LogprobPredictor(), object(), cfg)
        calls = []
        for name in sm.names:
            stage = sm.get_stage(name)

            def wrapped(*a, _orig=stage.generate, **kw):
                calls.append(kw)
                return _orig(*a, **kw)
            stage.generate = wrapped
        try:
            del ops.trace[:]
            pipe.batch_process(PROMPTS, max_tokens=4, temperature=0.7)
        finally:
            for name in sm.names:
                del sm.get_stage(name).generate
            pipe.shutdown()
        assert calls
        for kw in calls:
            for key in ("typical_p", "epsilon_cutoff", "eta_cutoff"):
                assert (key in kw) == (key in cfg_kw) and (key not in kw or kw[key] == cfg_kw[key])
        assert ("entropy_cut_rows" in [n for n, _ in ops.trace]) == bool(cfg_kw)


def test_pipeline_section_keys(tmp_path):
    from asd_amd.serving.pipeline import PipelineConfig
    path = tmp_path / "serving.yaml"
    path.write_text("pipeline:\n  typical_p: 0.9\n  eta_cutoff: 0.001\n")
    cfg = PipelineConfig.from_yaml(str(path))
    assert cfg.typical_p == 0.9 and cfg.eta_cutoff == 0.001 and cfg.epsilon_cutoff is None
