"""Top-N log-probs per committed token (`Stage.generate(logprobs=N)`, `PipelineConfig.logprobs`) on CPU tensors with the oracle
ops twin (tests/top_logprobs_ref.py): shapes and dtypes, replay from the kept steps, slot 0 at greedy positions, the same
tokens and log-probs with and without the table, no extra launch without it, invalid values, and the pipeline handing the
[n, 5] table to the predictor and to FeatureExtractor.extract."""
import numpy as np
import pytest

import asd_amd
from asd_amd.serving.components import FeatureExtractor
from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
from asd_amd.serving.stages import StageManager
from tests import top_logprobs_ref as T
from tests.greedy_ref import pick_mid_stop
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, stage_configs, text_ids


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def _stage(name, **kw):
    """A fresh manager per run: a sampled run moves the stage's generator, and the runs below must start from the same state."""
    ops = T.TopOracleOps()
    return StageManager(stage_configs(**kw), ops=ops).get_stage(name), ops


def _inv_t(temperature):
    return 1.0 if temperature == 0.0 else float(np.float32(1.0 / temperature))


@pytest.mark.parametrize("with_stop", [False, True], ids=["free", "stop"])
@pytest.mark.parametrize("temperature", [TEMPERATURE, 0.0], ids=["sampled", "greedy"])
@pytest.mark.parametrize("name", NAMES[:2])              # stage 0 and a verifying stage
def test_generate_with_logprobs(name, temperature, with_stop):
    stage, ops = _stage(name)
    kw = {}
    if with_stop:
        free = T.run(stage, temperature)[0]
        b0, i0, stop_id = pick_mid_stop(free)
        kw["stop_token_ids"] = (stop_id,)
        stage, ops = _stage(name)
    # without the table: today's launches, nothing else
    texts, lps, stats = T.run(stage, temperature, **kw)
    assert ops.calls["top_logprobs"] == 0 and ops.calls["commit_top_logprobs"] == 0
    assert "top_logprobs" not in stats and "top_token_ids" not in stats
    # with it: the same tokens and log-probs, bit for bit, and the generator where the other run left it
    other, ops2 = _stage(name)
    t2, lp2, st2 = T.run(other, temperature, T.N_TOP, keep=True, **kw)
    assert t2 == texts and all(a.tobytes() == b.tobytes() for a, b in zip(lp2, lps))
    assert st2["n_tokens"] == stats["n_tokens"] and st2["finish_reasons"] == stats["finish_reasons"]
    assert np.array_equal(other.gen.get_state().numpy(), stage.gen.get_state().numpy())
    assert ops2.calls["top_logprobs"] == ops2.calls["commit_top_logprobs"] == st2["steps"] == len(other.step_inputs)
    for k in ("verify", "verify_greedy", "draft_sample", "residual_sample_lp", "commit_step_lp", "commit_step_stop"):
        assert ops2.calls[k] == ops.calls[k], k              # one call per step is all that was added
    if with_stop:
        assert st2["finish_reasons"][b0] == "stop" and st2["n_tokens"][b0] == i0 + 1 < MAX_TOKENS
    else:
        assert st2["n_tokens"] == [MAX_TOKENS] * len(PROMPTS)
    for s in other.step_inputs:
        assert s["top_id"].shape == s["top_lp"].shape == (len(PROMPTS), 1 if name == NAMES[0] else stage.config.draft_len + 1, T.N_TOP)
    T.check_tables(other.step_inputs, t2, lp2, st2, T.N_TOP, _inv_t(temperature), greedy=temperature == 0.0)


def test_untruncated_table_entry_is_the_returned_logprob():
    """With truncation off the committed token's log-prob and its table entry are the same f64 number (the twin computes both in
    f64 and rounds once); and every committed token of these runs is among its row's 5 most likely often enough to matter."""
    for name in NAMES[:2]:
        stage, _ = _stage(name, top_p=1.0)
        texts, lps, stats = T.run(stage, TEMPERATURE, T.N_TOP)
        worst, found = T.pair_gap(texts, lps, stats)
        assert found >= len(PROMPTS) * MAX_TOKENS // 4 and worst <= T.PAIR_ATOL, (name, worst, found)


def test_config_value_and_call_value():
    stage, ops = _stage(NAMES[0], logprobs=3)
    _, _, stats = T.run(stage, 0.0)
    assert stats["top_logprobs"][0].shape == (MAX_TOKENS, 3)
    _, _, stats = T.run(stage, 0.0, 8)
    assert stats["top_token_ids"][0].shape == (MAX_TOKENS, 8)
    before = ops.calls["top_logprobs"]
    _, _, stats = T.run(stage, 0.0, 0)                      # 0 turns the config value off
    assert "top_logprobs" not in stats and ops.calls["top_logprobs"] == before


@pytest.mark.parametrize("bad", [9, -1, 2.5, "5", True])
def test_invalid_logprobs_raise(bad):
    stage, _ = _stage(NAMES[0])
    with pytest.raises(ValueError):
        stage.generate(["p"], max_tokens=2, logprobs=bad)
    with pytest.raises(ValueError):
        StageManager(stage_configs(logprobs=bad), ops=T.TopOracleOps()).get_stage(NAMES[0]).generate(["p"], max_tokens=2)


class _RecordingPredictor:
    def __init__(self):
        self.seen = []

    def predict(self, prompt, draft_output, draft_logprobs, stage_id, feature_extractor):
        self.seen.append((prompt, draft_output, draft_logprobs, stage_id))
        feats = feature_extractor.extract(prompt, draft_output, draft_logprobs, stage_id)
        return float(np.clip(np.exp(feats[3]) + 0.15 * stage_id, 0.01, 0.99))


class _RecordingCache:
    def __init__(self):
        self.entries = []

    def get_cache(self, request_id, stage):
        return None

    def allocate(self, request_id, stage, entry):
        self.entries.append((stage, entry))

    def cleanup_request(self, request_id):
        pass

    def truncate_at_stage(self, request_id, stage):
        pass

    def get_stats(self):
        return {}


def test_pipeline_hands_the_table_to_the_predictor():
    sm = StageManager(stage_configs(), ops=T.TopOracleOps())
    pred, cache, fx = _RecordingPredictor(), _RecordingCache(), FeatureExtractor()
    pipe = AdaptiveSpeculativePipeline(sm, pred, fx, PipelineConfig(lambda_value=30.0, stage_names=NAMES, logprobs=T.N_TOP),
                                       cache_manager=cache)
    try:
        results = pipe.batch_process(PROMPTS, max_tokens=8, temperature=TEMPERATURE)
    finally:
        pipe.shutdown()
    assert len(results) == len(PROMPTS) and len(pred.seen) >= len(PROMPTS)
    for prompt, output, table, stage_id in pred.seen:
        n = len(output.split())
        assert isinstance(table, np.ndarray) and table.shape == (n, T.N_TOP) and table.dtype == np.float32 and n == 8
        # the specification's features (RESEARCH_PROTOCOL.md:378-385), by hand
        t64 = table.astype(np.float64)
        f0 = -np.mean([(np.exp(row) * row).sum() for row in t64[-32:]])
        f3 = np.mean([row.max() for row in t64])
        feats = fx.extract(prompt, output, table, stage_id)
        assert feats[0] == f0 > 0.0 and feats[3] == f3 < 0.0
        assert feats[3] == t64[:, 0].mean()                  # the per-token maximum is slot 0
    assert cache.entries and all("top_logprobs" in e and e["top_logprobs"].shape == (8, T.N_TOP) and e["logprobs"].shape == (8,)
                                 for _, e in cache.entries)


def test_pipeline_without_logprobs_is_unchanged():
    sm = StageManager(stage_configs(), ops=T.TopOracleOps())
    pred, cache = _RecordingPredictor(), _RecordingCache()
    pipe = AdaptiveSpeculativePipeline(sm, pred, FeatureExtractor(), PipelineConfig(lambda_value=30.0, stage_names=NAMES),
                                       cache_manager=cache)
    try:
        pipe.batch_process(PROMPTS[:2], max_tokens=8, temperature=TEMPERATURE)
    finally:
        pipe.shutdown()
    assert all(table.shape == (8,) for _, _, table, _ in pred.seen)
    assert all("top_logprobs" not in e for _, e in cache.entries) and sm.ops.calls["top_logprobs"] == 0


def test_from_yaml_reads_logprobs(tmp_path):
    path = tmp_path / "serving.yaml"
    path.write_text("pipeline:\n  lambda_value: 2.0\n  logprobs: 5\n")
    assert PipelineConfig.from_yaml(str(path)).logprobs == 5
    path.write_text("pipeline:\n  lambda_value: 2.0\n")
    assert PipelineConfig.from_yaml(str(path)).logprobs is None
