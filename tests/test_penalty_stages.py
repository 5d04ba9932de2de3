"""Repetition, presence and frequency penalties in Stage.generate and the pipeline, on CPU: the three tiny stages of
tests/stage_scenario.py (vocabulary 1000, MAX_TOKENS = 12, DRAFT_LEN = 4, 5 prompts) on the oracle twin of tests/penalty_ref.py,
whose penalty_rows / penalty_commit are the numpy references of asd_penalty_rows / asd_penalty_commit.  The scenarios are those
tests/test_gpu_penalty_stages.py runs on the kernels."""
import pytest

import asd_amd
from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
from asd_amd.serving.stages import StageManager
from tests.logit_edit_ref import SEEDS
from tests.oracle_backend import OracleBackend
from tests.penalty_ref import (DISCOURAGE, PenaltyOracleOps, scenario_greedy, scenario_replay, scenario_rows_independent,
                               scenario_signs_and_stops)
from tests.stage_scenario import MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, LogprobPredictor, stage_configs, text_ids
from tests.test_seeded_stages import SeedRecordingManager, WordPredictor


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def _manager(**kw):
    ops = PenaltyOracleOps()
    return StageManager(stage_configs(**kw), ops=ops), ops


@pytest.mark.parametrize("name", NAMES)
def test_edit_bits_arguments_state_and_replay(name):
    sm, ops = _manager()
    stage = sm.get_stage(name)
    scenario_replay(stage, atol=1e-6)                 # the twin's lp is the f64 value rounded to f32 (tests/test_stages.py)
    names = [n for n, _ in ops.trace]
    # the second (penalised) call: one upload; per step one penalty call per logits tensor, each right behind the edit's, and
    # one commit call
    steps = stage.last_steps
    per_step = 1 if name == NAMES[0] else stage.config.draft_len + 1
    assert names.count("pack_penalties") == 1
    assert names.count("penalty_rows") == steps * per_step and names.count("penalty_commit") == steps
    assert all(names[i - 1] == "logit_edit_rows" for i, n in enumerate(names) if n == "penalty_rows")


@pytest.mark.parametrize("name", NAMES)
def test_other_signs_and_a_row_that_ends_early(name):
    sm, _ = _manager()
    scenario_signs_and_stops(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_row_b_is_the_call_that_gives_every_row_its_values(name):
    sm, _ = _manager()
    scenario_rows_independent(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_greedy_text_is_the_teacher_forced_penalised_arg_max(name):
    import torch
    sm, _ = _manager(dtype=torch.float32)            # (tests/penalty_ref.py, GREEDY: why float32)
    share = scenario_greedy(sm.get_stage(name))
    print(f"[penalties] stage {name}: {share:.3f} of the teacher-forced positions kept")


def test_the_configuration_supplies_the_default():
    from asd_amd.serving.stages import StageConfig
    cfg = StageConfig()
    assert (cfg.repetition_penalty, cfg.presence_penalty, cfg.frequency_penalty) == (1.0, 0.0, 0.0)
    kw = dict(prompts=PROMPTS, max_tokens=4, temperature=TEMPERATURE, seed=SEEDS)
    sm, _ = _manager()
    want = sm.get_stage(NAMES[1]).generate(**kw, repetition_penalty=1.5, frequency_penalty=0.5)
    sm, ops = _manager(repetition_penalty=1.5, frequency_penalty=0.5)
    stage = sm.get_stage(NAMES[1])
    got = stage.generate(**kw)
    assert got[0] == want[0] and all(a.tobytes() == b.tobytes() for a, b in zip(got[1], want[1]))
    assert "penalty_rows" in [n for n, _ in ops.trace]
    ops.trace.clear()
    stage.generate(**kw, repetition_penalty=1.0, frequency_penalty=0.0)          # a keyword that is not None replaces the field
    assert not [n for n, _ in ops.trace if "penalt" in n]


# ------------------------------------------------------------------------------------------ the pipeline
REQS = ["easy a", "hard a", "mid a", "hard b", "easy b", "mid b", "hard c"]
REP = [1.0 + 0.1 * i for i in range(len(REQS))]
FREQ = [0.2 * i - 0.6 for i in range(len(REQS))]
KEYS = ("repetition_penalty", "presence_penalty", "frequency_penalty")


def _owner(prompt):
    owner = [i for i, orig in enumerate(REQS) if prompt == orig or prompt.startswith(orig + " ")]
    assert len(owner) == 1
    return owner[0]


@pytest.mark.parametrize("grouping", ["predicted_stage", "none"])
def test_pipeline_hands_every_request_its_own_values_through(grouping):
    sm = SeedRecordingManager()
    pipe = AdaptiveSpeculativePipeline(sm, WordPredictor(), object(),
                                       PipelineConfig(lambda_value=30.0, stop_rule="full", risk_adjustment=False,
                                                      batch_grouping=grouping))
    calls = lambda: [c for st in sm.stages.values() for c in st.calls]        # noqa: E731
    res = pipe.batch_process(REQS, max_tokens=4, repetition_penalty=REP, frequency_penalty=FREQ, presence_penalty=0.5)
    seen = 0
    for call in calls():
        assert set(call["kw"]) == set(KEYS) and call["kw"]["presence_penalty"] == 0.5
        for j, p in enumerate(call["prompts"]):
            assert (call["kw"]["repetition_penalty"][j], call["kw"]["frequency_penalty"][j]) == (REP[_owner(p)], FREQ[_owner(p)])
            seen += 1
    assert seen == sum(r.stages_run for r in res) > len(REQS)               # later stages saw subsets
    # the keyword is passed only when it is set: the duck-typed stages of the older tests keep working
    for kw, want in ((dict(frequency_penalty=0.25), {"frequency_penalty": 0.25}), ({}, {})):
        for st in sm.stages.values():
            st.calls.clear()
        pipe.batch_process(REQS[:3], max_tokens=4, **kw)
        assert calls() and all(c["kw"] == want for c in calls())
    for st in sm.stages.values():
        st.calls.clear()
    pipe.process_request("hard x", max_tokens=4, repetition_penalty=1.3, presence_penalty=-1.0)
    assert calls() and all(c["kw"] == {"repetition_penalty": 1.3, "presence_penalty": -1.0} for c in calls())
    n = len(calls())
    for bad in (dict(repetition_penalty=[1.1] * 2), dict(frequency_penalty=[0.0] * 4), dict(presence_penalty=[0.1] * 7)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            pipe.batch_process(REQS[:3], max_tokens=4, **bad)
    with pytest.raises(ValueError, match="presence_penalty"):
        pipe.process_request("hard x", max_tokens=4, presence_penalty=[0.5])
    assert len(calls()) == n
    pipe.shutdown()


def test_pipeline_on_the_stages_penalises_every_request_with_its_own_values():
    sm, ops = _manager()
    cfg = PipelineConfig(lambda_value=30.0, stop_rule="full", stage_names=NAMES)
    pipe = AdaptiveSpeculativePipeline(sm, LogprobPredictor(), object(), cfg)
    res = pipe.batch_process(PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seeds=SEEDS, **DISCOURAGE)
    plain = pipe.batch_process(PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seeds=SEEDS)
    pipe.shutdown()
    assert max(r.stages_run for r in res) > 1 and "penalty_commit" in [n for n, _ in ops.trace]
    assert all(len(text_ids(r.output)) == MAX_TOKENS for r in res)
    assert [r.output for r in res] != [r.output for r in plain]
