"""Allow-lists in Stage.generate and the pipeline, on CPU: the three tiny stages of tests/stage_scenario.py (vocabulary 1000,
MAX_TOKENS = 12, DRAFT_LEN = 4) on the oracle twin of tests/token_mask_ref.py, whose logit_mask_rows is the torch reference of
asd_logit_mask_rows.  The scenarios are those tests/test_gpu_token_mask_stages.py runs on the kernels."""
import pytest

import asd_amd
from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
from asd_amd.serving.stages import StageManager
from tests.logit_edit_ref import SEEDS
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, LogprobPredictor, stage_configs, text_ids
from tests.test_seeded_stages import SeedRecordingManager, WordPredictor
from tests.token_mask_ref import (MaskOracleOps, per_prompt_lists, scenario_greedy, scenario_restrict, scenario_rows_independent,
                                  scenario_single, scenario_top_n, scenario_with_edits)


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def _manager(**kw):
    ops = MaskOracleOps()
    return StageManager(stage_configs(**kw), ops=ops), ops


@pytest.mark.parametrize("name", NAMES)
def test_only_listed_tokens_are_proposed_accepted_or_drawn(name):
    sm, ops = _manager()
    stage = sm.get_stage(name)
    scenario_restrict(stage, atol=1e-6)               # the twin's lp is the f64 value rounded to f32 (tests/test_stages.py)
    names = [n for n, _ in ops.trace]
    # two calls, each: one upload, one mask per logits tensor -- K proposals and the target's output at a verifying stage
    assert names.count("pack_token_masks") == 2 and "logit_edit_rows" not in names
    per_step = 1 if name == NAMES[0] else stage.config.draft_len + 1
    assert names.count("logit_mask_rows") % per_step == 0 and names.count("logit_mask_rows") >= 2 * per_step


@pytest.mark.parametrize("name", NAMES)
def test_a_one_id_list_commits_that_id(name):
    sm, _ = _manager()
    scenario_single(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_greedy_takes_the_arg_max_inside_the_list(name):
    sm, _ = _manager()
    scenario_greedy(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_row_b_is_the_call_that_gives_every_row_list_b(name):
    sm, _ = _manager()
    scenario_rows_independent(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_the_list_is_the_ban_of_its_complement(name):
    sm, _ = _manager()
    scenario_with_edits(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_top_n_slots_beyond_the_list_are_empty(name):
    sm, _ = _manager()
    scenario_top_n(sm.get_stage(name))


# ------------------------------------------------------------------------------------------ the pipeline
REQS = ["easy a", "hard a", "mid a", "hard b", "easy b", "mid b", "hard c"]
ALLOW = [None if i == 2 else [i, 10 + i, 20 + i] for i in range(len(REQS))]


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
    res = pipe.batch_process(REQS, max_tokens=4, allowed_token_ids=ALLOW)
    seen = 0
    for call in calls():
        assert set(call["kw"]) == {"allowed_token_ids"}
        for j, p in enumerate(call["prompts"]):
            assert call["kw"]["allowed_token_ids"][j] == ALLOW[_owner(p)]
            seen += 1
    assert seen == sum(r.stages_run for r in res) > len(REQS)               # later stages saw subsets
    # together with the sparse edits, each request keeps all of its own
    for st in sm.stages.values():
        st.calls.clear()
    bans = [[100 + i] for i in range(len(REQS))]
    pipe.batch_process(REQS, max_tokens=4, allowed_token_ids=ALLOW, banned_token_ids=bans)
    for call in calls():
        for j, p in enumerate(call["prompts"]):
            assert (call["kw"]["allowed_token_ids"][j], call["kw"]["banned_token_ids"][j]) == (ALLOW[_owner(p)], bans[_owner(p)])
    # one list for the batch stays one value; the keyword is passed only when it is set
    for kw, want in ((dict(allowed_token_ids=[4, 5]), {"allowed_token_ids": (4, 5)}), ({}, {})):
        for st in sm.stages.values():
            st.calls.clear()
        pipe.batch_process(REQS[:3], max_tokens=4, **kw)
        assert calls() and all(c["kw"] == want for c in calls())
    for st in sm.stages.values():
        st.calls.clear()
    pipe.process_request("hard x", max_tokens=4, allowed_token_ids=[4, 5])
    assert calls() and all(c["kw"] == {"allowed_token_ids": (4, 5)} for c in calls())
    n = len(calls())
    for bad in (dict(allowed_token_ids=[[1]] * 2), dict(allowed_token_ids=[None] * 4), dict(allowed_token_ids=5)):
        with pytest.raises(ValueError):
            pipe.batch_process(REQS[:3], max_tokens=4, **bad)
    assert len(calls()) == n
    pipe.shutdown()


def test_pipeline_on_the_stages_keeps_every_request_inside_its_list():
    sm, _ = _manager()
    cfg = PipelineConfig(lambda_value=30.0, stop_rule="full", stage_names=NAMES)
    pipe = AdaptiveSpeculativePipeline(sm, LogprobPredictor(), object(), cfg)
    lists = per_prompt_lists(1000)
    res = pipe.batch_process(PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seeds=SEEDS, allowed_token_ids=lists)
    pipe.shutdown()
    assert max(r.stages_run for r in res) > 1
    for r, ids in zip(res, lists):
        assert len(text_ids(r.output)) == MAX_TOKENS and (ids is None or set(text_ids(r.output)) <= set(ids))
