"""Stop tokens (EOS) in Stage.generate and the pipeline, on CPU tensors with the ops twin of tests/stop_scenario.py: a run with a
stop set returns the free run's rows up to and including the first stop id (tokens and log-prob bytes), says why every row
ended, and leaves the loop as soon as the device-side counter says all rows have; without a stop set the parent's path runs."""
import numpy as np
import pytest

import asd_amd
from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
from asd_amd.serving.stages import StageManager
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import (MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, LogprobPredictor, expected_results, record_generate,
                                  stage_configs)
from tests.stop_scenario import StopOracleOps, assert_prefix_property, free_run, pick_stop_ids


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def fresh_manager(**kw):
    return StageManager(stage_configs(**kw), ops=StopOracleOps())


@pytest.fixture(scope="module")
def free():
    """The free run of every stage: each on its first generate call of one manager (the seeds of `stage_configs`)."""
    asd_amd.set_backend(OracleBackend())
    sm = fresh_manager()
    out = {n: free_run(sm.get_stage(n)) for n in NAMES}
    assert sm.ops.calls["commit_step_stop"] == 0 and sm.ops.calls["commit_step_lp"] > 0
    return out


def test_a_stop_set_returns_the_free_runs_prefix(free):
    sm = fresh_manager()
    seen = set()
    for name in NAMES:
        ids = pick_stop_ids(free[name])
        assert 1 <= len(ids) <= 8
        before = sm.ops.calls["commit_step_lp"]
        texts, lps, stats = sm.get_stage(name).generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE,
                                                        stop_token_ids=ids)
        want = assert_prefix_property(free[name], ids, texts, lps, stats)
        assert sm.ops.calls["commit_step_lp"] == before and stats["steps"] <= free[name]["stats"]["steps"]
        seen |= {how for _, _, how in want}
    assert sm.ops.calls["commit_step_stop"] > 0
    # over the three stages: a stop on the first token, on an accepted draft token, on a drawn token, and a row that runs on
    assert seen >= {"first", "accepted", "drawn", None}, seen


def test_all_rows_stopping_in_step_one_ends_the_loop_at_the_first_read(free):
    sm = fresh_manager()
    for name in NAMES:
        ids = sorted({row[0] for row in free[name]["tokens"]})
        stage = sm.get_stage(name)
        texts, lps, stats = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, stop_token_ids=ids)
        assert_prefix_property(free[name], ids, texts, lps, stats)
        assert stats["n_tokens"] == [1] * len(PROMPTS) and stats["finish_reasons"] == ["stop"] * len(PROMPTS)
        assert stats["steps"] <= stage.config.sync_every


@pytest.mark.parametrize("how", ["argument_none", "argument_empty", "config_set_argument_empty"])
def test_without_a_stop_set_the_parents_path_runs(free, how):
    sm = fresh_manager(stop_token_ids=(free["8b"]["tokens"][0][0],)) if how == "config_set_argument_empty" else fresh_manager()
    kw = {} if how == "argument_none" else {"stop_token_ids": []}
    for name in NAMES:
        texts, lps, stats = sm.get_stage(name).generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, **kw)
        assert_prefix_property(free[name], (), texts, lps, stats)             # all of it, bit for bit
        assert stats["finish_reasons"] == ["length"] * len(PROMPTS) and stats["steps"] == free[name]["stats"]["steps"]
    assert sm.ops.calls["commit_step_stop"] == 0


def test_the_configs_stop_set_is_the_default(free):
    ids = pick_stop_ids(free["13b"])
    sm = fresh_manager(stop_token_ids=tuple(ids))
    texts, lps, stats = sm.get_stage("13b").generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE)
    assert_prefix_property(free["13b"], ids, texts, lps, stats)
    assert "stop" in stats["finish_reasons"]


@pytest.mark.parametrize("ids", [[1000], [-1], [3, 3], list(range(9))])
def test_bad_stop_sets_raise_before_any_launch(ids):
    sm = fresh_manager()
    with pytest.raises(ValueError):
        sm.get_stage("13b").generate(prompts=PROMPTS, max_tokens=4, temperature=TEMPERATURE, stop_token_ids=ids)
    with pytest.raises(ValueError):
        fresh_manager(stop_token_ids=tuple(ids)).get_stage("8b").generate(prompts=PROMPTS, max_tokens=4)
    assert not sm.ops.calls


def test_pipeline_passes_the_stop_set_and_scores_the_ragged_logprobs(free):
    ids = pick_stop_ids(free["8b"]) + pick_stop_ids(free["13b"])[:2]
    ids = list(dict.fromkeys(ids))[:8]
    ops = StopOracleOps()
    sm = StageManager(stage_configs(), ops=ops)
    stats_log = []
    for name in NAMES:                                       # keep every call's stats (record_generate keeps texts and log-probs)
        stage = sm.get_stage(name)

        def keeping(*a, _orig=stage.generate, **kw):
            assert tuple(kw["stop_token_ids"]) == tuple(ids)
            out = _orig(*a, **kw)
            stats_log.append(out[2])
            return out
        stage.generate = keeping
    log = record_generate(sm, lambda: ops.calls["verify"])
    lam = 30.0
    pipe = AdaptiveSpeculativePipeline(sm, LogprobPredictor(), object(),
                                       PipelineConfig(lambda_value=lam, stop_rule="full", stage_names=NAMES, stop_token_ids=ids))
    res = pipe.batch_process(PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE)
    pipe.shutdown()
    want = expected_results(log, PROMPTS, lam, "full")
    ragged = 0
    for p, r, (probs, k) in zip(PROMPTS, res, want):
        assert r.stage_probabilities == probs and r.stopped_at_stage == k
        n_call = next(i for i, c in enumerate(log) if c["stage"] == NAMES[k] and any(q.startswith(p) for q in c["prompts"]))
        call = log[n_call]
        j = next(j for j, q in enumerate(call["prompts"]) if q.startswith(p) and call["texts"][j] == r.output)
        n = stats_log[n_call]["n_tokens"][j]
        assert len(r.output.split()) == n == len(call["logprobs"][j])
        ragged += n < MAX_TOKENS
    assert ragged >= 1, "the scenario must end at least one returned output at a stop token"
    assert ops.calls["commit_step_stop"] > 0 and ops.calls["commit_step_lp"] == 0


def test_pipeline_without_the_option_passes_no_keyword():
    calls = []

    class OldStage:                                          # the signature of the duck-typed stages of the older tests
        cost_per_token = 1.0

        def generate(self, prompts, max_tokens, temperature, return_logprobs=True):
            calls.append(list(prompts))
            return ["t1 t2" for _ in prompts], [np.array([-0.1, -0.2], np.float32) for _ in prompts], {"generation_time_ms": 1.0}

    class Manager:
        def get_stage(self, name):
            return OldStage()

    pipe = AdaptiveSpeculativePipeline(Manager(), LogprobPredictor(), object(), PipelineConfig(lambda_value=1.0, stage_names=NAMES))
    res = pipe.batch_process(PROMPTS[:2], max_tokens=2, temperature=TEMPERATURE)
    pipe.shutdown()
    assert calls and all(r.output == "t1 t2" for r in res)
    assert PipelineConfig().stop_token_ids is None
