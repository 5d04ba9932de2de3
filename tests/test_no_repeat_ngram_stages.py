"""no_repeat_ngram_size in Stage.generate and the pipeline, on CPU: the three tiny stages of tests/stage_scenario.py at vocabulary
64 with 32 tokens per row (DRAFT_LEN = 4, 5 prompts) on the oracle twin of tests/ngram_ref.py, whose no_repeat_ngram_rows is the
numpy reference of asd_no_repeat_ngram_rows.  The scenarios are those tests/test_gpu_no_repeat_ngram_stages.py runs on the kernel."""
import pytest

import asd_amd
from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
from asd_amd.serving.stages import StageManager
from tests.logit_edit_ref import SEEDS
from tests.ngram_ref import (VOCAB, NgramOracleOps, scenario_call_trace, scenario_composition, scenario_greedy, scenario_per_prompt,
                             scenario_pipeline, scenario_prompt_counts, scenario_sampled)
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import NAMES, PROMPTS, TEMPERATURE, stage_configs
from tests.test_seeded_stages import SeedRecordingManager, WordPredictor


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def _manager(**kw):
    ops = NgramOracleOps()
    return StageManager(stage_configs(vocab=VOCAB, **kw), ops=ops), ops


@pytest.mark.parametrize("n", [2, 3, 1])
@pytest.mark.parametrize("name", NAMES)
def test_greedy_rows_leave_the_plain_run_at_its_first_repeat_and_repeat_nothing(name, n):
    sm, _ = _manager()
    scenario_greedy(sm.get_stage(name), n)


@pytest.mark.parametrize("name", NAMES)
def test_sampled_rows_repeat_nothing_and_every_kept_step_has_the_reference_bans(name):
    sm, _ = _manager()
    scenario_sampled(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_row_b_is_the_call_that_gives_every_row_its_n(name):
    sm, _ = _manager()
    scenario_per_prompt(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_the_prompt_counts_and_the_padding_does_not(name):
    sm, _ = _manager()
    scenario_prompt_counts(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_composes_with_allow_list_bias_penalties_bad_words_top_n_and_a_stop_id(name):
    sm, _ = _manager()
    scenario_composition(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_call_trace(name):
    sm, ops = _manager()
    stage = sm.get_stage(name)
    scenario_call_trace(stage)
    # the twin's own trace of one call with nothing else on: one upload, and the proposal buffer exists for this feature alone
    ops.trace.clear()
    stage.generate(prompts=PROMPTS, max_tokens=4, temperature=TEMPERATURE, seed=SEEDS, no_repeat_ngram_size=2)
    names = [n for n, _ in ops.trace]
    per_step = 1 if stage.draft is None else stage.config.draft_len + 1
    assert names.count("pack_no_repeat_ngram") == 1 and names.count("no_repeat_ngram_rows") == stage.last_steps * per_step
    assert not {"bad_words_rows", "logit_edit_rows", "penalty_rows", "logit_mask_rows"} & set(names)
    # the configuration's value is the default, and the keyword replaces it
    sm2, ops2 = _manager(no_repeat_ngram_size=3)
    sm2.get_stage(name).generate(prompts=PROMPTS, max_tokens=4, temperature=0.0)
    assert "no_repeat_ngram_rows" in [n for n, _ in ops2.trace]
    ops2.trace.clear()
    sm2.get_stage(name).generate(prompts=PROMPTS, max_tokens=4, temperature=0.0, no_repeat_ngram_size=0)
    assert not [n for n, _ in ops2.trace if "ngram" in n]


# ------------------------------------------------------------------------------------------ the pipeline
REQS = ["easy a", "hard a", "mid a", "hard b", "easy b", "mid b", "hard c"]
SIZES = [2, 0, 3, 8, 1, 0, 4]


def _owner(prompt):
    owner = [i for i, orig in enumerate(REQS) if prompt == orig or prompt.startswith(orig + " ")]
    assert len(owner) == 1
    return owner[0]


@pytest.mark.parametrize("grouping", ["predicted_stage", "none"])
def test_pipeline_hands_every_request_its_own_n_through(grouping):
    sm = SeedRecordingManager()
    pipe = AdaptiveSpeculativePipeline(sm, WordPredictor(), object(),
                                       PipelineConfig(lambda_value=30.0, stop_rule="full", risk_adjustment=False,
                                                      batch_grouping=grouping))
    calls = lambda: [c for st in sm.stages.values() for c in st.calls]        # noqa: E731
    res = pipe.batch_process(REQS, max_tokens=4, no_repeat_ngram_size=SIZES)
    seen = 0
    for call in calls():
        assert set(call["kw"]) == {"no_repeat_ngram_size"}
        for j, p in enumerate(call["prompts"]):
            assert call["kw"]["no_repeat_ngram_size"][j] == SIZES[_owner(p)]
            seen += 1
    assert seen == sum(r.stages_run for r in res) > len(REQS)               # later stages saw subsets
    # one value for the batch reaches the stages as it is; the keyword is passed only when it is set
    for kw, want in ((dict(no_repeat_ngram_size=3), {"no_repeat_ngram_size": 3}), ({}, {})):
        for st in sm.stages.values():
            st.calls.clear()
        pipe.batch_process(REQS[:3], max_tokens=4, **kw)
        assert calls() and all(c["kw"] == want for c in calls())
    for st in sm.stages.values():
        st.calls.clear()
    pipe.process_request("hard x", max_tokens=4, no_repeat_ngram_size=2)
    assert calls() and all(c["kw"] == {"no_repeat_ngram_size": 2} for c in calls())
    n = len(calls())
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        pipe.batch_process(REQS[:3], max_tokens=4, no_repeat_ngram_size=SIZES[:2])
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        pipe.process_request("hard x", max_tokens=4, no_repeat_ngram_size=[2])
    assert len(calls()) == n
    pipe.shutdown()
    # the configuration's value is handed on when the call names none, and the call's own value replaces it
    sm = SeedRecordingManager()
    pipe = AdaptiveSpeculativePipeline(sm, WordPredictor(), object(),
                                       PipelineConfig(lambda_value=30.0, stop_rule="full", risk_adjustment=False,
                                                      no_repeat_ngram_size=4))
    pipe.batch_process(REQS[:3], max_tokens=4)
    assert calls() and all(c["kw"] == {"no_repeat_ngram_size": 4} for c in calls())
    for st in sm.stages.values():
        st.calls.clear()
    pipe.batch_process(REQS[:3], max_tokens=4, no_repeat_ngram_size=[1, 2, 3])
    assert calls() and all(c["kw"]["no_repeat_ngram_size"] == [[1, 2, 3][_owner(p)] for p in c["prompts"]] for c in calls())
    pipe.shutdown()


def test_pipeline_on_the_stages_repeats_nothing():
    sm, ops = _manager()
    scenario_pipeline(sm)
    assert "no_repeat_ngram_rows" in [n for n, _ in ops.trace]
