"""Greedy decoding (temperature 0) in serving/stages.py on HipOps: the stage-level checks of tests/test_greedy_stages.py through
asd_verify_greedy -- tiny shapes, vocabulary 1000, 12 tokens."""
import numpy as np
import pytest

from tests import greedy_ref as G
from tests.stage_scenario import DRAFT_LEN, MAX_TOKENS, NAMES, PROMPTS, LogprobPredictor

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def hip_backend():
    import asd_amd
    asd_amd.set_backend(None)
    yield


def _manager(ops=None, **kw):
    from asd_amd.distributed import HipOps
    from asd_amd.serving.stages import StageManager
    return StageManager(G.greedy_configs(**kw), ops=ops or HipOps())


@pytest.fixture(scope="module")
def hip_manager():
    return _manager()


@pytest.fixture(scope="module")
def runs(hip_manager):
    out = {}
    for name in NAMES:
        stage = hip_manager.get_stage(name)
        texts, lps, stats = G.run_greedy(stage, keep=True)
        out[name] = (texts, lps, stats, list(stage.step_inputs))
    hip_manager.ops.check_status()
    return out


@pytest.mark.parametrize("name", NAMES)
def test_greedy_generate_shapes_and_replay(hip_manager, runs, name):
    stage = hip_manager.get_stage(name)
    texts, lps, _, steps = runs[name]
    G.check_shapes(texts, lps)
    stage.step_inputs = steps
    worst = G.check_replay(stage, texts, lps, atol=1e-5)
    print(f"stage {name}: max |lp - f64| = {worst:.3g} over {len(steps)} steps")


@pytest.mark.parametrize("name", NAMES)
def test_greedy_does_not_depend_on_the_seed_or_the_truncation(hip_manager, runs, name):
    texts, lps, _, _ = runs[name]
    cfgs = G.greedy_configs(top_p=0.5, top_k=3, target_top_p=0.5, target_top_k=3)
    for c in cfgs:
        c.seed += 1000
    from asd_amd.serving.stages import StageManager
    other = StageManager(cfgs, ops=hip_manager.ops).get_stage(name)
    for kw in (dict(), dict(top_p=0.5)):
        t2, lp2, _ = G.run_greedy(other, **kw)
        assert t2 == texts and all(a.tobytes() == b.tobytes() for a, b in zip(lp2, lps))


@pytest.mark.parametrize("name", NAMES[1:])
def test_greedy_speculation_is_lossless(hip_manager, runs, name):
    kept = G.check_lossless(hip_manager.get_stage(name), runs[name][0])
    print(f"stage {name}: {kept:.0%} of the positions have a top-2 gap above {G.LOSSLESS_GAP}")


def test_the_draft_is_used(runs):
    assert runs["13b"][2]["steps"] < MAX_TOKENS
    n_acc = np.concatenate([s["n_acc"].cpu().numpy() for s in runs["13b"][3]])
    assert (n_acc == DRAFT_LEN).any()


@pytest.mark.parametrize("name", NAMES)
def test_greedy_stop_tokens(hip_manager, runs, name):
    G.check_stop(hip_manager.get_stage(name), runs[name][0], runs[name][1])
    hip_manager.ops.check_status()


def test_pipeline_passes_temperature_zero_through(hip_manager):
    from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
    pipe = AdaptiveSpeculativePipeline(_manager(ops=hip_manager.ops), LogprobPredictor(), object(),
                                       PipelineConfig(lambda_value=30.0, stage_names=NAMES))
    try:
        r = pipe.process_request(PROMPTS[0], max_tokens=8, temperature=0.0)
        again = pipe.batch_process([PROMPTS[0]], max_tokens=8, temperature=0.0)
    finally:
        pipe.shutdown()
    assert len(r.output.split()) == 8 and r.stages_run >= 1
    assert again[0].output == r.output and again[0].stage_probabilities == r.stage_probabilities
