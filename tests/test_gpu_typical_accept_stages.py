"""Typical acceptance in Stage.generate on distributed.HipOps (serving/stages.py, TYPICAL ACCEPTANCE), on the tiny float32 stages
of tests/stage_scenario.py at vocabulary 64: through asd_typical_accept and the real draw, at the two verifying stages and under
prompt lookup."""
import numpy as np
import pytest
import torch

from tests.logit_edit_ref import SEEDS, run_kept
from tests.stage_scenario import MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, ref_logprob, stage_configs

pytestmark = pytest.mark.gpu

INV_T = 1.0 / TEMPERATURE
LP_ATOL = 2e-5
LOOKUP = dict(prompt_lookup_num_tokens=3, top_p=1.0)
ROUTES = [(NAMES[1], {}), (NAMES[2], {}), (NAMES[0], LOOKUP)]


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs(vocab=64, dtype=torch.float32))


def _run(stage, extra, **kw):
    """-> (texts, lps, stats, the steps' records on the host) of a seeded call with the inputs kept."""
    out = run_kept(stage, prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, **extra, **kw)
    steps = [{k: v.cpu().numpy() for k, v in s.items() if isinstance(v, torch.Tensor)} for s in stage.step_inputs]
    return (*out, steps)


def _teacher_forced(steps, lps, n_tok):
    """Every committed token's reported log-prob against the f64 log-softmax of the kept processed row it was taken from."""
    B, P = len(lps), int(steps[0]["seq_len"][0])
    want = [[] for _ in range(B)]
    for s in steps:
        K = s["tok"].shape[1]
        rows = np.concatenate([s["logits"], s["bonus"][:, None]], 1)
        for b in range(B):
            n = int(s["n_acc"][b])
            assert np.array_equal(s["commit_row"][b], rows[b, n]) and 0 <= n <= K      # the gathered row is row n_acc
            if int(s["seq_len"][b]) - P == len(want[b]):                                # (a finished row's length stands still)
                want[b] += [ref_logprob(rows[b, k], s["tok"][b, k], INV_T) for k in range(n)]
                want[b].append(ref_logprob(rows[b, n], s["drawn"][b], INV_T))
    for b in range(B):
        assert n_tok[b] == len(lps[b]) <= len(want[b])
        assert np.abs(lps[b].astype(np.float64) - np.array(want[b][:n_tok[b]])).max() <= LP_ATOL, b


@pytest.mark.parametrize("name,extra", ROUTES)
def test_typical_acceptance_through_the_stage(manager, name, extra):
    stage = manager.get_stage(name)
    texts, lps, stats, steps = _run(stage, extra, typical_acceptance_threshold=0.09, typical_acceptance_alpha=0.3)
    _teacher_forced(steps, lps, stats["n_tokens"])
    acc, prop = stats["typical_accepted"], stats["typical_proposed"]
    assert all(0 <= a <= p for a, p in zip(acc, prop)) and min(prop) > 0
    assert (texts, [lp.tobytes() for lp in lps]) == (lambda o: (o[0], [lp.tobytes() for lp in o[1]]))(
        _run(stage, extra, typical_acceptance_alpha=0.3))                                # the default threshold; repeats itself

    # eps = 1e-30, alpha = 100: every proposal with target mass is accepted
    _, lps, stats, steps = _run(stage, extra, typical_acceptance_threshold=1e-30, typical_acceptance_alpha=100)
    _teacher_forced(steps, lps, stats["n_tokens"])
    for s in steps:
        K = s["tok"].shape[1]
        mass = np.array([[0 <= s["tok"][b, k] < 64 and ref_logprob(s["logits"][b, k], s["tok"][b, k], INV_T) > np.log(1e-30) + 1e-3
                          for k in range(K)] for b in range(len(PROMPTS))])
        assert np.array_equal((s["accept_bits"][:, None] >> np.arange(K)) & 1, mass.astype(np.int64))

    # eps = 1, alpha = 100 at 64 tokens (H <= ln 64 < ln 100): the threshold is p > 1, nothing is accepted
    _, lps, stats, steps = _run(stage, extra, typical_acceptance_threshold=1.0, typical_acceptance_alpha=100)
    _teacher_forced(steps, lps, stats["n_tokens"])                                       # ... and every token is row 0's plain draw
    assert all(not s["n_acc"].any() and not s["accept_bits"].any() for s in steps)
    assert stats["typical_accepted"] == [0] * len(PROMPTS) and stats["steps"] >= MAX_TOKENS
    manager.ops.check_status()
