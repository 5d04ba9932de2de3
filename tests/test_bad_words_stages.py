"""Multi-token bad words in Stage.generate and the pipeline, on CPU: the three tiny stages of tests/stage_scenario.py (vocabulary
1000, MAX_TOKENS = 12, DRAFT_LEN = 4, 5 prompts) on the oracle twin of tests/bad_words_ref.py, whose bad_words_rows is the numpy
reference of asd_bad_words_rows.  The scenarios are those tests/test_gpu_bad_words_stages.py runs on the kernel."""
import pytest

import asd_amd
from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
from asd_amd.serving.stages import StageManager
from tests.bad_words_ref import (BadWordsOracleOps, check_no_word, scenario_call_trace, scenario_composition, scenario_greedy_replay,
                                 scenario_rows_independent, scenario_sampled)
from tests.logit_edit_ref import SEEDS
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, LogprobPredictor, stage_configs, text_ids
from tests.test_seeded_stages import SeedRecordingManager, WordPredictor


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def _manager(**kw):
    ops = BadWordsOracleOps()
    return StageManager(stage_configs(**kw), ops=ops), ops


@pytest.mark.parametrize("name", NAMES)
def test_greedy_replay_changes_the_token_that_would_complete_the_word(name):
    sm, _ = _manager()
    scenario_greedy_replay(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_sampled_rows_hold_no_word_and_every_kept_step_has_the_reference_bans(name):
    sm, _ = _manager()
    scenario_sampled(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_row_b_is_the_call_that_gives_every_row_its_list(name):
    sm, _ = _manager()
    scenario_rows_independent(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_composes_with_allow_list_bias_penalties_top_n_and_a_stop_id(name):
    sm, _ = _manager()
    scenario_composition(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_call_trace(name):
    sm, ops = _manager()
    stage = sm.get_stage(name)
    scenario_call_trace(stage)
    # the twin's own trace of one call: the word tables are uploaded once, and the proposal buffer is one buffer of the call
    ops.trace.clear()
    stage.generate(prompts=PROMPTS, max_tokens=4, temperature=TEMPERATURE, seed=SEEDS, bad_words=[(2, 4)], presence_penalty=0.5)
    names = [n for n, _ in ops.trace]
    assert names.count("pack_bad_words") == 1 and names.count("bad_words_rows") == names.count("penalty_rows") > 0
    assert "logit_edit_rows" not in names


# ------------------------------------------------------------------------------------------ the pipeline
REQS = ["easy a", "hard a", "mid a", "hard b", "easy b", "mid b", "hard c"]
WORDS = [[(i, i + 1), f"w{i}"] for i in range(len(REQS))]
WORDS[2] = None


def _owner(prompt):
    owner = [i for i, orig in enumerate(REQS) if prompt == orig or prompt.startswith(orig + " ")]
    assert len(owner) == 1
    return owner[0]


@pytest.mark.parametrize("grouping", ["predicted_stage", "none"])
def test_pipeline_hands_every_request_its_own_list_through(grouping):
    sm = SeedRecordingManager()
    pipe = AdaptiveSpeculativePipeline(sm, WordPredictor(), object(),
                                       PipelineConfig(lambda_value=30.0, stop_rule="full", risk_adjustment=False,
                                                      batch_grouping=grouping))
    calls = lambda: [c for st in sm.stages.values() for c in st.calls]        # noqa: E731
    res = pipe.batch_process(REQS, max_tokens=4, bad_words=WORDS)
    seen = 0
    for call in calls():
        assert set(call["kw"]) == {"bad_words_per_prompt"}
        for j, p in enumerate(call["prompts"]):
            assert call["kw"]["bad_words_per_prompt"][j] == (WORDS[_owner(p)] or [])
            seen += 1
    assert seen == sum(r.stages_run for r in res) > len(REQS)               # later stages saw subsets
    # one list for the batch is the stages' common list; the keyword is passed only when it is set
    for kw, want in ((dict(bad_words=[(3, 4), "x"]), {"bad_words": ((3, 4), "x")}), ({}, {})):
        for st in sm.stages.values():
            st.calls.clear()
        pipe.batch_process(REQS[:3], max_tokens=4, **kw)
        assert calls() and all(c["kw"] == want for c in calls())
    for st in sm.stages.values():
        st.calls.clear()
    pipe.process_request("hard x", max_tokens=4, bad_words=[[7, 8, 9]])
    assert calls() and all(c["kw"] == {"bad_words": ([7, 8, 9],)} for c in calls())
    n = len(calls())
    for bad in (dict(bad_words=WORDS[:2]), dict(bad_words="abc"), dict(bad_words=[(1, 2), [(3, 4)]])):
        with pytest.raises(ValueError, match="bad_words"):
            pipe.batch_process(REQS[:3], max_tokens=4, **bad)
    with pytest.raises(ValueError, match="bad_words"):
        pipe.process_request("hard x", max_tokens=4, bad_words=[[(1, 2)]])
    assert len(calls()) == n
    pipe.shutdown()


def test_pipeline_on_the_stages_keeps_every_request_clear_of_its_words():
    sm, ops = _manager()
    cfg = PipelineConfig(lambda_value=30.0, stop_rule="full", stage_names=NAMES)
    pipe = AdaptiveSpeculativePipeline(sm, LogprobPredictor(), object(), cfg)
    plain = pipe.batch_process(PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seeds=SEEDS)
    rows = [[(t[2],), tuple(t[0:2])] for t in (text_ids(r.output) for r in plain)]
    res = pipe.batch_process(PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seeds=SEEDS, bad_words=rows)
    pipe.shutdown()
    assert max(r.stages_run for r in res) > 1 and "bad_words_rows" in [n for n, _ in ops.trace]
    assert all(len(text_ids(r.output)) == MAX_TOKENS for r in res)
    check_no_word([r.output for r in res], rows)
    assert [r.output for r in res] != [r.output for r in plain]
