"""Guided decoding in Stage.generate and the pipeline, on CPU: the three tiny stages of tests/stage_scenario.py (vocabulary 1000,
MAX_TOKENS = 12, DRAFT_LEN = 4, 5 prompts) on the oracle twin of tests/fsm_ref.py, whose fsm_mask_rows / fsm_advance / fsm_commit
are the numpy references of the kernels.  The scenarios are those tests/test_gpu_fsm_stages.py runs on the kernels."""
import pytest

import asd_amd
from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
from asd_amd.serving.stages import StageManager
from tests.fsm_ref import (CHOICES, OTHER_CHOICES, STOP, FsmOracleOps, check_choice_rows, scenario_call_trace, scenario_choices,
                           scenario_composition, scenario_kept_steps, scenario_logprobs, scenario_rows_independent)
from tests.logit_edit_ref import SEEDS
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import DRAFT_LEN, MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, LogprobPredictor, stage_configs
from tests.test_seeded_stages import SeedRecordingManager, WordPredictor

LP_BAR = 1e-6      # the twin's lp is the f64 value at its row rounded to f32 (tests/test_teacher_forced_stages.py)


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def _manager(**kw):
    ops = FsmOracleOps()
    return StageManager(stage_configs(**kw), ops=ops), ops


@pytest.mark.parametrize("greedy", [True, False], ids=["greedy", "sampled"])
@pytest.mark.parametrize("name", NAMES)
def test_every_row_is_one_choice_and_one_stop_id(name, greedy):
    sm, _ = _manager()
    scenario_choices(sm.get_stage(name), greedy)


@pytest.mark.parametrize("name", NAMES)
def test_an_unguided_row_is_the_call_without_guidance(name):
    sm, _ = _manager()
    scenario_rows_independent(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_every_kept_step_is_masked_by_the_replayed_state(name):
    sm, _ = _manager()
    scenario_kept_steps(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_returned_logprobs_match_the_f64_restricted_distribution(name):
    sm, _ = _manager()
    scenario_logprobs(sm.get_stage(name), LP_BAR)


@pytest.mark.parametrize("name", NAMES)
def test_composes_with_allow_list_bias_penalties_bad_words_and_top_n(name):
    sm, _ = _manager()
    scenario_composition(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_call_trace(name):
    sm, ops = _manager()
    stage = sm.get_stage(name)
    scenario_call_trace(stage)
    # the twin's own trace of one call: the tables are uploaded once; the proposal buffer is there for the automaton alone
    ops.trace.clear()
    stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, stop_token_ids=[STOP], guided_choice=CHOICES)
    names = [n for n, _ in ops.trace]
    steps, spec = stage.last_steps, stage.draft is not None
    assert names.count("pack_fsm") == 1 and names.count("fsm_commit") == steps
    assert names.count("fsm_mask_rows") == steps * (DRAFT_LEN + 1 if spec else 1)
    assert names.count("fsm_advance") == (steps * DRAFT_LEN if spec else 0)
    assert not [n for n in names if n in ("logit_mask_rows", "bad_words_rows", "logit_edit_rows", "penalty_rows")]
    # the configuration's value is the keyword's default
    sm2, ops2 = _manager(guided_choice=CHOICES, stop_token_ids=(STOP,))
    texts, _, stats = sm2.get_stage(name).generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0)
    check_choice_rows(texts, stats, [CHOICES] * len(PROMPTS))


# ------------------------------------------------------------------------------------------ the pipeline
REQS = ["easy a", "hard a", "mid a", "hard b", "easy b", "mid b", "hard c"]
LISTS = [[(i, i + 1), f"w{i}"] for i in range(len(REQS))]
LISTS[2] = None


def _owner(prompt):
    owner = [i for i, orig in enumerate(REQS) if prompt == orig or prompt.startswith(orig + " ")]
    assert len(owner) == 1
    return owner[0]


@pytest.mark.parametrize("grouping", ["predicted_stage", "none"])
def test_pipeline_hands_every_request_its_own_choices_through(grouping):
    sm = SeedRecordingManager()
    pipe = AdaptiveSpeculativePipeline(sm, WordPredictor(), object(),
                                       PipelineConfig(lambda_value=30.0, stop_rule="full", risk_adjustment=False,
                                                      batch_grouping=grouping))
    calls = lambda: [c for st in sm.stages.values() for c in st.calls]        # noqa: E731
    res = pipe.batch_process(REQS, max_tokens=4, guided_choice=LISTS)
    seen = 0
    for call in calls():
        assert set(call["kw"]) == {"guided_choice_per_prompt"}
        for j, p in enumerate(call["prompts"]):
            assert call["kw"]["guided_choice_per_prompt"][j] == LISTS[_owner(p)]
            seen += 1
    assert seen == sum(r.stages_run for r in res) > len(REQS)               # later stages saw subsets
    # one list for the batch is the stages' `guided_choice`; the keyword is passed only when it is set
    for kw, want in ((dict(guided_choice=[(3, 4), "x"]), {"guided_choice": ((3, 4), "x")}), ({}, {})):
        for st in sm.stages.values():
            st.calls.clear()
        pipe.batch_process(REQS[:3], max_tokens=4, **kw)
        assert calls() and all(c["kw"] == want for c in calls())
    for st in sm.stages.values():
        st.calls.clear()
    pipe.process_request("hard x", max_tokens=4, guided_choice=[[7, 8, 9]])
    assert calls() and all(c["kw"] == {"guided_choice": ([7, 8, 9],)} for c in calls())
    n = len(calls())
    for bad in (dict(guided_choice=LISTS[:2]), dict(guided_choice="abc"), dict(guided_choice=[(1, 2), [(3, 4)]])):
        with pytest.raises(ValueError, match="guided_choice"):
            pipe.batch_process(REQS[:3], max_tokens=4, **bad)
    with pytest.raises(ValueError, match="guided_choice"):
        pipe.process_request("hard x", max_tokens=4, guided_choice=[[(1, 2)]])
    assert len(calls()) == n
    pipe.shutdown()


def test_pipeline_on_the_stages_returns_one_choice_per_request():
    sm, ops = _manager(stop_token_ids=(STOP,))
    cfg = PipelineConfig(lambda_value=30.0, stop_rule="full", stage_names=NAMES)
    pipe = AdaptiveSpeculativePipeline(sm, LogprobPredictor(), object(), cfg)
    rows = [CHOICES, OTHER_CHOICES, CHOICES, OTHER_CHOICES, CHOICES]
    res = pipe.batch_process(PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seeds=SEEDS, guided_choice=rows)
    pipe.shutdown()
    assert "fsm_mask_rows" in [n for n, _ in ops.trace]
    from tests.stage_scenario import text_ids
    for r, choices in zip(res, rows):
        g = text_ids(r.output)
        assert tuple(g[:-1]) in set(choices) and g[-1] == STOP, g
