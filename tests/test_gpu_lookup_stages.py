"""Prompt-lookup drafting in Stage.generate on the kernels (HipOps), K = 4, at stage 0 and at a verifying stage of the tiny
scenario: (a) a forced repetition is committed five tokens per step; (b) every returned log-prob and greedy token passes the f64
teacher-forced check of tests/teacher_forced_ref.py; (c) the draft stage's model is never run."""
import math

import pytest
import torch

from tests.stage_scenario import NAMES, stage_configs
from tests.teacher_forced_ref import run_checked

pytestmark = pytest.mark.gpu

K, VOCAB = 4, 64
REPEATING = ["a b c d a b c d a b c d a b", "x y x y x y x y x", "one two three one two three one two"]
SAMPLED = [dict(temperature=0.0), dict(temperature=0.8, seed=1)]


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs(vocab=VOCAB))


@pytest.fixture(scope="module")
def manager_f32():
    """f32 stages, as the other teacher-forced GPU tests use: the reference's own bound (4 x the dtype's noise) is then small
    enough that nearly every greedy position lies outside its arg-max gap."""
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs(dtype=torch.float32))


@pytest.mark.parametrize("how", SAMPLED, ids=["greedy", "sampled"])
@pytest.mark.parametrize("name", NAMES[:2])
def test_a_forced_repetition_commits_five_tokens_a_step(manager, name, how):
    """The first step can only commit one token; every later one proposes t7 four times and commits five.  The same call without
    the keyword takes 33 steps."""
    stage = manager.get_stage(name)
    texts, _, stats = stage.generate(prompts=REPEATING, max_tokens=33, allowed_token_ids=[7], prompt_lookup_num_tokens=K, **how)
    assert texts == [" ".join(["t7"] * 33)] * len(REPEATING)
    sync = stage.config.sync_every
    assert stats["steps"] <= math.ceil((1 + math.ceil(32 / 5)) / sync) * sync
    assert len(stats["lookup_matched_steps"]) == len(REPEATING)


@pytest.mark.parametrize("how", [dict(temperature=0.0), dict(temperature=0.8, seed=1, top_p=0.9, repetition_penalty=1.2)],
                         ids=["greedy", "top-p + repetition penalty"])
@pytest.mark.parametrize("name", NAMES[:2])
def test_b_returned_logprobs_pass_the_teacher_forced_check(manager_f32, name, how):
    stage = manager_f32.get_stage(name)
    (_, _, stats), _ = run_checked(stage, 2e-5, f"{name} lookup", prompts=REPEATING, max_tokens=24, prompt_lookup_num_tokens=K,
                                   prompt_lookup_max_ngram=3, **how)
    assert max(stats["lookup_matched_steps"]) > 0
    assert "lookup_matched_steps" not in stage.generate(prompts=REPEATING, max_tokens=2, **how)[2]


def test_c_the_draft_model_is_not_run(manager):
    stage = manager.get_stage(NAMES[1])
    calls, real = [], stage.draft.model.forward_ragged
    stage.draft.model.forward_ragged = lambda *a, **kw: calls.append(1) or real(*a, **kw)
    try:
        stage.generate(prompts=REPEATING, max_tokens=8, prompt_lookup_num_tokens=K)
    finally:
        del stage.draft.model.forward_ragged
    assert not calls
