"""serving/stages.py on CPU tensors with the oracle ops twin (tests/stage_scenario.py): Stage.generate's contract (token and
log-prob counts, text round trip), every committed log-prob against the verify's lp_t / the f64 value at its row, and the
pipeline driving real stages (Bayes + DP on the returned log-probs; the verify step runs for the stages above 0 only)."""
import numpy as np
import pytest
import torch

import asd_amd
from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
from asd_amd.serving.stages import Stage, StageConfig, StageManager
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import (DRAFT_LEN, MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, LogprobPredictor, StageOracleOps,
                                  check_generation, expected_results, record_generate, stage_configs, text_ids)


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


@pytest.fixture(scope="module")
def manager():
    ops = StageOracleOps()
    return StageManager(stage_configs(), {"8b": [0]}, ops=ops)


def test_stage_manager_builds_the_hierarchy(manager):
    assert manager.names == NAMES
    s0, s1, s2 = (manager.get_stage(n) for n in NAMES)
    assert s0.draft is None and s1.draft is s0 and s2.draft is s1
    assert [s.cost_per_token for s in (s0, s1, s2)] == [1.0, 4.5, 10.0]
    info = s2.get_model_info()
    assert info["draft"] == "13b" and info["vocab"] == 1000 and info["parameters"] == s2.shape.param_count()
    assert manager.get_model_info()["8b"]["gpus"] == [0]
    with pytest.raises(KeyError):
        manager.get_stage("70b")
    with pytest.raises(ValueError):
        StageManager([StageConfig(model_size="1b")], ops=StageOracleOps())      # no shape for that label


def test_prompts_are_left_padded_to_the_longest(manager):
    s0 = manager.get_stage("8b")
    ids = s0.encode_prompts(PROMPTS)
    lens = [len(s0.tokenizer.encode(p, return_tensors=None)) for p in PROMPTS]
    assert ids.shape == (5, max(lens)) and ids.dtype == torch.int64 and int(ids.max()) < 1000
    for b, n in enumerate(lens):
        assert (ids[b, :ids.shape[1] - n] == 0).all()
        assert ids[b, ids.shape[1] - n:].tolist() == [i % 1000 for i in s0.tokenizer.encode(PROMPTS[b], return_tensors=None)]
    assert s0.encode_prompts(["x"]).shape == (1, 2)                             # at least two positions


@pytest.mark.parametrize("name", NAMES)
def test_generate_returns_max_tokens_with_their_logprobs(manager, name):
    stage, ops = manager.get_stage(name), manager.ops
    stage.keep_inputs = True
    before = dict(ops.calls)
    try:
        texts, lps, stats = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, return_logprobs=True)
    finally:
        stage.keep_inputs = False
    assert len(texts) == len(lps) == len(PROMPTS) and stats["generation_time_ms"] > 0
    for t, lp in zip(texts, lps):
        assert len(t.split()) == MAX_TOKENS == len(lp) and Stage.decode_tokens(text_ids(t)) == t
    inv_t = float(np.float32(1 / TEMPERATURE))
    check_generation(stage, texts, lps, inv_t, atol=1e-6)     # the twin's lp is the f64 value rounded to f32
    assert ops.calls["check_status"] == before.get("check_status", 0) + 1
    verifies = ops.calls["verify"] - before.get("verify", 0)
    if name == "8b":
        assert verifies == 0 and len(stage.step_inputs) == MAX_TOKENS
    else:
        assert verifies == len(stage.step_inputs) >= -(-MAX_TOKENS // (DRAFT_LEN + 1))
        n_acc = np.concatenate([s["n_acc"].numpy() for s in stage.step_inputs])
        if name == "13b":                       # the draft model IS the target (its nucleus aside): whole blocks pass, bonus draws
            assert (n_acc == DRAFT_LEN).any()
        else:
            assert (n_acc < DRAFT_LEN).any()    # rejections: residual draws
    assert stage.generate([], max_tokens=4) == ([], [], {"generation_time_ms": 0.0})
    assert stage.generate(["p"], max_tokens=3, return_logprobs=False)[1] is None


@pytest.mark.parametrize("stop_rule,lam", [("full", 30.0), ("full", 3.0), ("prefix", 30.0)])
def test_pipeline_drives_real_stages(stop_rule, lam):
    ops = StageOracleOps()
    sm = StageManager(stage_configs(), ops=ops)
    log = record_generate(sm, lambda: ops.calls["verify"])
    pipe = AdaptiveSpeculativePipeline(sm, LogprobPredictor(), object(),
                                       PipelineConfig(lambda_value=lam, stop_rule=stop_rule, stage_names=NAMES))
    res = pipe.batch_process(PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE)
    pipe.shutdown()
    want = expected_results(log, PROMPTS, lam, stop_rule)
    for r, (probs, k) in zip(res, want):
        assert r.stage_probabilities == probs and r.stopped_at_stage == k
        assert r.total_tokens == MAX_TOKENS * r.stages_run and len(r.output.split()) == MAX_TOKENS
    for call in log:                            # ONE generate call per executed stage; the verify runs above stage 0 only
        assert (call["verifies"] == 0) if call["stage"] == "8b" else (call["verifies"] >= 1)
    assert [c["stage"] for c in log] == list(NAMES[:len(log)]) and len(log[0]["prompts"]) == len(PROMPTS)
    if stop_rule == "prefix":
        assert all(r.stopped_at_stage == 0 for r in res) and len(log) == 1 and ops.calls["verify"] == 0
    elif lam == 30.0:
        assert max(r.stages_run for r in res) > 1, "the scenario must escalate at least one request"
