"""serving/stages.py on HipOps: the scenario of tests/test_stages.py through the real kernels.  Every drawn token's log-prob is
within 2e-5 (the project's bound for lp_t) of the f64 value on the kept bf16 logits; every accepted token's
is the verify's lp_t, bit for bit; the pipeline's Bayes + DP on the returned log-probs is bit-equal to the oracle's."""
import numpy as np
import pytest

from tests.stage_scenario import (MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, LogprobPredictor, check_generation, expected_results,
                                  record_generate, stage_configs)

pytestmark = pytest.mark.gpu

LP_ATOL = 2e-5


@pytest.fixture(scope="module")
def hip_manager():
    from asd_amd.distributed import HipOps
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs(), ops=HipOps())


@pytest.fixture(autouse=True)
def hip_backend():
    import asd_amd
    asd_amd.set_backend(None)
    yield


@pytest.mark.parametrize("name", NAMES)
def test_stage_generate_on_the_gpu(hip_manager, name):
    stage = hip_manager.get_stage(name)
    stage.keep_inputs = True
    try:
        texts, lps, _ = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, return_logprobs=True)
    finally:
        stage.keep_inputs = False
    worst = check_generation(stage, texts, lps, float(np.float32(1 / TEMPERATURE)), atol=LP_ATOL)
    print(f"stage {name}: max |lp_drawn - f64| = {worst:.3g} over {len(stage.step_inputs)} steps")
    hip_manager.ops.check_status()                     # clean status words (raises otherwise)


@pytest.mark.parametrize("stop_rule,lam", [("full", 30.0), ("prefix", 30.0)])
def test_pipeline_on_real_stages_matches_the_oracle(hip_manager, stop_rule, lam):
    from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
    from asd_amd.serving.stages import StageManager
    sm = StageManager(stage_configs(), ops=hip_manager.ops)
    log = record_generate(sm)
    pipe = AdaptiveSpeculativePipeline(sm, LogprobPredictor(), object(),
                                       PipelineConfig(lambda_value=lam, stop_rule=stop_rule, stage_names=NAMES))
    res = pipe.batch_process(PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE)
    pipe.shutdown()
    want = expected_results(log, PROMPTS, lam, stop_rule)
    for r, (probs, k) in zip(res, want):
        assert r.stage_probabilities == probs and r.stopped_at_stage == k      # bit-equal to the oracle's Bayes + DP
        assert len(r.output.split()) == MAX_TOKENS
    if stop_rule == "prefix":
        assert all(r.stopped_at_stage == 0 for r in res) and [c["stage"] for c in log] == ["8b"]
    sm.ops.check_status()


def test_full_vocabulary_stage_with_a_truncated_target():
    """tiny(vocab=152064), B = 4, target top-k 50 / top-p 0.9: the full vocabulary and the truncated route through Stage once."""
    import torch
    from asd_amd.distributed import HipOps
    from asd_amd.serving.stages import StageManager
    ops = HipOps()
    cfgs = stage_configs(vocab=152064, target_top_k=50, target_top_p=0.9)[:2]
    cfgs[1].model_seed = 1                              # a draft that differs from its target: residual draws as well
    sm = StageManager(cfgs, ops=ops)
    stage = sm.get_stage("13b")
    stage.keep_inputs = True
    texts, lps, _ = stage.generate(prompts=PROMPTS[:4], max_tokens=10, temperature=TEMPERATURE)
    inv_t = float(np.float32(1 / TEMPERATURE))

    def thr_of_bonus(bonus):                            # the bonus rows' threshold: the draft sampler's select on those rows
        r = torch.zeros((bonus.shape[0],), device="cuda")
        return ops.draft_sample_top_k(bonus.cuda().contiguous(), r, inv_t, top_k=50, top_p=0.9)[2].cpu().numpy()

    worst = check_generation(stage, texts, lps, inv_t, atol=LP_ATOL, thr_of_bonus=thr_of_bonus, max_tokens=10)
    print(f"full vocabulary, truncated target: max |lp_drawn - f64| = {worst:.3g}")
    n_acc = np.concatenate([s["n_acc"].cpu().numpy() for s in stage.step_inputs])
    assert all(s["t_thr"] is not None for s in stage.step_inputs) and len(n_acc) > 0
    ops.check_status()
