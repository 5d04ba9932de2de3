"""Stage.generate with min-p on distributed.HipOps: the three tiny stages of tests/stage_scenario.py with min_p = target_min_p =
0.05, every step kept through keep_inputs and replayed against the oracle twin's arithmetic (the method of
tests/test_gpu_stages.py: check_generation with the bonus rows' thresholds), a run with a stop set and logprobs = 3, and one
full-vocabulary two-stage run."""
import numpy as np
import pytest
import torch

from tests.min_p_ref import min_p_delta, min_p_thresholds
from tests.stage_scenario import MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, check_generation, stage_configs, text_ids

pytestmark = pytest.mark.gpu

MIN_P = 0.05
INV_T = float(np.float32(1 / TEMPERATURE))
ATOL = 2e-5        # tests/test_gpu_stages.py's bar for a kernel lp against the f64 value at its row


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs(min_p=MIN_P, target_min_p=MIN_P))


def _thr_of_bonus(cfg):
    return lambda bonus: min_p_thresholds(bonus.cpu(), INV_T, cfg.target_top_k, cfg.target_top_p, MIN_P)


def _check_kept_sets(stage, B):
    """Every committed draw lies in its row's kept set, and every threshold is at least x_max + delta."""
    delta = min_p_delta(MIN_P, INV_T)
    for s in stage.step_inputs:
        drawn = s["drawn"].cpu().numpy()
        if "tok" in s:
            x, thr = s["logits"].float().cpu().numpy(), s["t_thr"].cpu().numpy()
            assert thr.tobytes() == min_p_thresholds(s["logits"].cpu(), INV_T, stage.config.target_top_k,
                                                     stage.config.target_top_p, MIN_P).reshape(thr.shape).tobytes()
            n_acc, Kd = s["n_acc"].cpu().numpy(), s["tok"].shape[1]
            for b in range(B):
                if n_acc[b] < Kd:
                    assert x[b, n_acc[b], drawn[b]] >= thr[b, n_acc[b]]
        else:
            x, thr = s["logits"].float().cpu().numpy(), s["thr"].cpu().numpy()
            assert (thr >= x.max(-1) + delta).all() and (x[np.arange(B), drawn] >= thr).all()


@pytest.mark.parametrize("name", NAMES)
def test_stage_generation_replays_against_the_twin(manager, name):
    stage = manager.get_stage(name)
    stage.keep_inputs = True
    try:
        texts, lps, _ = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE)
    finally:
        stage.keep_inputs = False
    check_generation(stage, texts, lps, INV_T, atol=ATOL, thr_of_bonus=_thr_of_bonus(stage.config))
    _check_kept_sets(stage, len(PROMPTS))
    manager.ops.check_status()


def test_stop_set_and_top_logprobs_with_min_p(manager):
    stage = manager.get_stage("34b")
    plain, _, _ = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE)
    stop = sorted({text_ids(t)[3] for t in plain})[:8]             # ids the run is known to commit
    stage.gen.manual_seed(int(stage.config.seed))
    stage.keep_inputs = True
    try:
        texts, lps, stats = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, stop_token_ids=stop,
                                           logprobs=3, min_p=MIN_P)
    finally:
        stage.keep_inputs = False
    assert "stop" in stats["finish_reasons"]
    for t, lp, n, why, ids, tlp in zip(texts, lps, stats["n_tokens"], stats["finish_reasons"], stats["top_token_ids"],
                                       stats["top_logprobs"]):
        tk = text_ids(t)
        assert len(tk) == n == len(lp) and ids.shape == (n, 3) and tlp.shape == (n, 3)
        assert (why == "stop") == (tk[-1] in stop) and not any(i in stop for i in tk[:-1])
        assert np.isfinite(lp).all() and (np.diff(tlp, axis=1) <= 0).all()
        # the table is the UNTRUNCATED distribution: the committed token's renormalised log-prob is not below its entry
        for i in range(n):
            hit = np.nonzero(ids[i] == tk[i])[0]
            if hit.size:
                assert lp[i] >= tlp[i, hit[0]] - 1e-5
    _check_kept_sets(stage, len(PROMPTS))
    manager.ops.check_status()


def test_full_vocabulary_two_stage_run():
    from asd_amd.serving.stages import StageManager
    sm = StageManager(stage_configs(vocab=152064, min_p=MIN_P, target_min_p=MIN_P)[:2])
    stage = sm.get_stage(NAMES[1])
    stage.keep_inputs = True
    texts, lps, _ = stage.generate(prompts=PROMPTS[:4], max_tokens=10, temperature=TEMPERATURE)
    stage.keep_inputs = False
    check_generation(stage, texts, lps, INV_T, atol=ATOL, thr_of_bonus=_thr_of_bonus(stage.config), max_tokens=10)
    _check_kept_sets(stage, 4)
    sm.ops.check_status()
