"""Greedy decoding (temperature 0) in serving/stages.py on CPU tensors with the oracle ops twin (tests/greedy_ref.py): the
stage-level checks -- shapes, replay from the kept rows, seed independence, ignored truncation, losslessness (teacher-forced),
the draft is used, stop tokens, the pipeline passes temperature 0 through."""
import numpy as np
import pytest

import asd_amd
from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
from asd_amd.serving.stages import StageManager
from tests import greedy_ref as G
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import DRAFT_LEN, MAX_TOKENS, NAMES, PROMPTS, LogprobPredictor


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


@pytest.fixture(scope="module")
def manager():
    return StageManager(G.greedy_configs(), ops=G.GreedyOracleOps())


@pytest.fixture(scope="module")
def runs(manager):
    """One greedy run per stage with its step inputs kept: name -> (texts, lps, stats, step_inputs)."""
    out = {}
    for name in NAMES:
        stage = manager.get_stage(name)
        texts, lps, stats = G.run_greedy(stage, keep=True)
        out[name] = (texts, lps, stats, list(stage.step_inputs))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_greedy_generate_shapes_and_replay(manager, runs, name):
    stage = manager.get_stage(name)
    texts, lps, stats, steps = runs[name]
    G.check_shapes(texts, lps)
    stage.step_inputs = steps
    G.check_replay(stage, texts, lps, atol=1e-5)
    for s in steps:                                         # what a greedy step keeps
        assert set(s) == {"logits", "tok", "n_acc", "argmax", "lp_argmax", "lp_t", "drawn", "lp_drawn", "seq_len"}
        assert s["logits"].dim() == (2 if name == "8b" else 3)
    if name == "8b":
        assert len(steps) == MAX_TOKENS == stats["steps"]
    else:
        assert steps[0]["logits"].shape[1] == DRAFT_LEN + 1


def test_negative_temperature_still_raises(manager):
    for t in (-0.5, float("nan")):
        with pytest.raises(ValueError):
            manager.get_stage("8b").generate(["p"], max_tokens=2, temperature=t)


@pytest.mark.parametrize("name", NAMES)
def test_greedy_does_not_depend_on_the_seed_or_the_truncation(runs, name):
    texts, lps, _, _ = runs[name]
    for kw in (dict(), dict(top_p=0.5, top_k=3, target_top_p=0.5, target_top_k=3)):
        cfgs = G.greedy_configs(**kw)
        for c in cfgs:
            c.seed += 1000
        other = StageManager(cfgs, ops=G.GreedyOracleOps()).get_stage(name)
        t2, lp2, _ = G.run_greedy(other)
        assert t2 == texts and all(a.tobytes() == b.tobytes() for a, b in zip(lp2, lps))
    # ... nor on the per-call nucleus; and the generator is left where it was
    stage = StageManager(G.greedy_configs(), ops=G.GreedyOracleOps()).get_stage(name)
    before = stage.gen.get_state().clone()
    t3, lp3, _ = G.run_greedy(stage, top_p=0.5)
    assert t3 == texts and all(a.tobytes() == b.tobytes() for a, b in zip(lp3, lps))
    assert np.array_equal(stage.gen.get_state().numpy(), before.numpy())


@pytest.mark.parametrize("name", NAMES[1:])
def test_greedy_speculation_is_lossless(manager, runs, name):
    G.check_lossless(manager.get_stage(name), runs[name][0])


def test_the_draft_is_used(runs):
    assert runs["13b"][2]["steps"] < MAX_TOKENS               # stage 1 shares stage 0's weights: whole blocks pass
    n_acc = np.concatenate([s["n_acc"].numpy() for s in runs["13b"][3]])
    assert (n_acc == DRAFT_LEN).any()


@pytest.mark.parametrize("name", NAMES)
def test_greedy_stop_tokens(manager, runs, name):
    G.check_stop(manager.get_stage(name), runs[name][0], runs[name][1])


def test_pipeline_passes_temperature_zero_through():
    sm = StageManager(G.greedy_configs(), ops=G.GreedyOracleOps())
    pipe = AdaptiveSpeculativePipeline(sm, LogprobPredictor(), object(), PipelineConfig(lambda_value=30.0, stage_names=NAMES))
    try:
        r = pipe.process_request(PROMPTS[0], max_tokens=8, temperature=0.0)
        again = pipe.batch_process([PROMPTS[0]], max_tokens=8, temperature=0.0)
    finally:
        pipe.shutdown()
    assert len(r.output.split()) == 8 and r.stages_run >= 1
    assert again[0].output == r.output and again[0].stage_probabilities == r.stage_probabilities     # reproducible
