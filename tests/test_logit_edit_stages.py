"""Logit bias, banned tokens and min_tokens in Stage.generate and the pipeline, on CPU: the three tiny stages of
tests/stage_scenario.py (vocabulary 1000, MAX_TOKENS = 12, DRAFT_LEN = 4) on the oracle twin of tests/logit_edit_ref.py, whose
logit_edit_rows is the torch reference of asd_logit_edit_rows.  The scenarios are those tests/test_gpu_logit_edit_stages.py runs
on the kernels."""
import numpy as np
import pytest

import asd_amd
from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
from asd_amd.serving.stages import StageManager
from tests.logit_edit_ref import (SEEDS, EditOracleOps, scenario_ban, scenario_force, scenario_min_tokens,
                                  scenario_rows_independent)
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, LogprobPredictor, stage_configs, text_ids
from tests.test_seeded_stages import SeedRecordingManager, WordPredictor


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def _manager(**kw):
    ops = EditOracleOps()
    return StageManager(stage_configs(**kw), ops=ops), ops


@pytest.mark.parametrize("name", NAMES)
def test_banned_tokens_are_never_proposed_accepted_or_drawn(name):
    sm, ops = _manager()
    stage = sm.get_stage(name)
    scenario_ban(stage, atol=1e-6)                    # the twin's lp is the f64 value rounded to f32 (tests/test_stages.py)
    names = [n for n, _ in ops.trace]
    # the edited call (the baseline made none): one upload, one edit per logits tensor -- K proposals and the target's output at a verifying stage
    per_step = 1 if name == NAMES[0] else stage.config.draft_len + 1
    assert names.count("logit_edit_rows") == stage.last_steps * per_step and names.count("pack_logit_edits") == 1


@pytest.mark.parametrize("name", NAMES)
def test_a_bias_of_100_forces_the_token(name):
    sm, _ = _manager()
    scenario_force(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_min_tokens_keeps_the_stop_ids_away(name):
    sm, _ = _manager()
    scenario_min_tokens(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_row_b_is_the_call_that_gives_every_row_bs_edit(name):
    sm, _ = _manager()
    scenario_rows_independent(sm.get_stage(name))


def test_the_top_n_table_never_lists_a_banned_token():
    sm, _ = _manager()
    stage = sm.get_stage(NAMES[2])
    base, _, stats = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, logprobs=3)
    banned = [sorted({int(i) for i in ids[:, 0]}) for ids in stats["top_token_ids"]]       # every row's most likely tokens
    texts, lps, stats = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, logprobs=3,
                                       banned_token_ids=banned)
    for b, ids in enumerate(stats["top_token_ids"]):
        assert ids.shape == (MAX_TOKENS, 3) and (ids >= 0).all() and not set(ids.ravel().tolist()) & set(banned[b])
        assert np.isfinite(stats["top_logprobs"][b]).all() and not set(text_ids(texts[b])) & set(banned[b])


# ------------------------------------------------------------------------------------------ the pipeline
REQS = ["easy a", "hard a", "mid a", "hard b", "easy b", "mid b", "hard c"]
BANS = [[i, 10 + i] for i in range(len(REQS))]
BIAS = [None if i % 2 else {i: 1.0 + i} for i in range(len(REQS))]
MINS = [i % 3 for i in range(len(REQS))]


def _owner(prompt):
    owner = [i for i, orig in enumerate(REQS) if prompt == orig or prompt.startswith(orig + " ")]
    assert len(owner) == 1
    return owner[0]


@pytest.mark.parametrize("grouping", ["predicted_stage", "none"])
def test_pipeline_hands_every_request_its_own_edits_through(grouping):
    sm = SeedRecordingManager()
    pipe = AdaptiveSpeculativePipeline(sm, WordPredictor(), object(),
                                       PipelineConfig(lambda_value=30.0, stop_rule="full", risk_adjustment=False,
                                                      batch_grouping=grouping))
    calls = lambda: [c for st in sm.stages.values() for c in st.calls]        # noqa: E731
    res = pipe.batch_process(REQS, max_tokens=4, banned_token_ids=BANS, logit_bias=BIAS, min_tokens=MINS)
    seen = 0
    for call in calls():
        assert set(call["kw"]) == {"banned_token_ids", "logit_bias", "min_tokens"}
        for j, p in enumerate(call["prompts"]):
            i = _owner(p)
            assert (call["kw"]["banned_token_ids"][j], call["kw"]["logit_bias"][j], call["kw"]["min_tokens"][j]) == \
                (BANS[i], BIAS[i], MINS[i])
            seen += 1
    assert seen == sum(r.stages_run for r in res) > len(REQS)               # later stages saw subsets
    # one value for the batch stays one value; a keyword is passed only when it is set
    for kw, want in ((dict(banned_token_ids=[4, 5]), {"banned_token_ids": (4, 5)}), (dict(logit_bias={3: -2.0}), {"logit_bias": {3: -2.0}}),
                     (dict(min_tokens=2), {"min_tokens": 2}), ({}, {})):
        for st in sm.stages.values():
            st.calls.clear()
        pipe.batch_process(REQS[:3], max_tokens=4, **kw)
        assert calls() and all(c["kw"] == want for c in calls())
    for st in sm.stages.values():
        st.calls.clear()
    pipe.process_request("hard x", max_tokens=4, banned_token_ids=[4, 5], logit_bias={3: 1.0}, min_tokens=1)
    assert calls() and all(c["kw"] == {"banned_token_ids": (4, 5), "logit_bias": {3: 1.0}, "min_tokens": 1} for c in calls())
    n = len(calls())
    for bad in (dict(banned_token_ids=[[1]] * 2), dict(logit_bias=[{}] * 4), dict(min_tokens=[1, 2]), dict(banned_token_ids=5)):
        with pytest.raises(ValueError):
            pipe.batch_process(REQS[:3], max_tokens=4, **bad)
    assert len(calls()) == n
    pipe.shutdown()


def test_pipeline_on_the_stages_keeps_banned_tokens_out():
    sm, _ = _manager()
    cfg = PipelineConfig(lambda_value=30.0, stop_rule="full", stage_names=NAMES)
    pipe = AdaptiveSpeculativePipeline(sm, LogprobPredictor(), object(), cfg)
    free = pipe.batch_process(PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seeds=SEEDS)
    bans = [sorted(set(text_ids(r.output))) for r in free]
    res = pipe.batch_process(PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seeds=SEEDS, banned_token_ids=bans)
    pipe.shutdown()
    for r, ban in zip(res, bans):
        assert len(text_ids(r.output)) == MAX_TOKENS and not set(text_ids(r.output)) & set(ban)
