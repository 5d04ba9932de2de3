"""Logit bias, banned tokens and min_tokens in Stage.generate on distributed.HipOps (serving/stages.py, LOGIT EDITS): the
scenarios of tests/test_logit_edit_stages.py (tests/logit_edit_ref.py) through asd_logit_edit_rows and the real samplers, on the
three tiny stages of tests/stage_scenario.py, at the replay bar of tests/test_gpu_stages.py; and one two-stage run at the full
vocabulary."""
import numpy as np
import pytest

from tests.logit_edit_ref import (SEEDS, run_kept, scenario_ban, scenario_force, scenario_min_tokens, scenario_rows_independent)
from tests.per_request_ref import inv_t_of
from tests.stage_scenario import NAMES, PROMPTS, TEMPERATURE, check_generation, stage_configs, text_ids

pytestmark = pytest.mark.gpu

ATOL = 2e-5        # tests/test_gpu_stages.py's bar for a kernel lp against the f64 value at its row


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs())


@pytest.mark.parametrize("name", NAMES)
def test_banned_tokens_are_never_proposed_accepted_or_drawn(manager, name):
    worst = scenario_ban(manager.get_stage(name), atol=ATOL)
    print(f"[logit edits] stage {name}: max |lp_drawn - f64| on the edited rows = {worst:.3e}")
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_a_bias_of_100_forces_the_token(manager, name):
    scenario_force(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_min_tokens_keeps_the_stop_ids_away(manager, name):
    scenario_min_tokens(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_row_b_is_the_call_that_gives_every_row_bs_edit(manager, name):
    scenario_rows_independent(manager.get_stage(name))
    manager.ops.check_status()


def test_full_vocabulary_two_stage_run():
    """tiny(vocab=152064), B = 4, 8 tokens: bans, biases and min_tokens together through the verifying stage once."""
    import torch
    from asd_amd.serving.stages import StageManager
    cfgs = stage_configs(vocab=152064)[:2]
    cfgs[1].model_seed = 1                              # a draft that differs from its target: residual draws as well
    sm = StageManager(cfgs)
    stage = sm.get_stage(NAMES[1])
    kw = dict(prompts=PROMPTS[:4], max_tokens=8, temperature=TEMPERATURE, seed=SEEDS[:4])
    base, _, _ = stage.generate(**kw)
    toks = [text_ids(t) for t in base]
    bans = [sorted(set(t)) + [0, 152063] for t in toks]
    bias = [{(t[0] + 1) % 152064: 4.0, 152062: -50.0} for t in toks]
    texts, lps, _ = run_kept(stage, banned_token_ids=bans, logit_bias=bias, **kw)
    for b, t in enumerate(texts):
        assert not set(text_ids(t)) & set(bans[b]) and np.isfinite(lps[b]).all()
    for s in stage.step_inputs:
        for b, ids in enumerate(bans):
            assert torch.isneginf(s["logits"][b][:, ids]).all() and torch.isneginf(s["bonus"][b][ids]).all()
            assert not set(s["tok"][b].tolist()) & set(ids)
    check_generation(stage, texts, lps, inv_t_of(TEMPERATURE), atol=ATOL, max_tokens=8)
    # min_tokens on the same stage: the first tokens of the edited run as stop ids
    stops = sorted({text_ids(t)[0] for t in texts})
    _, _, stats = stage.generate(banned_token_ids=bans, logit_bias=bias, stop_token_ids=stops, **kw)
    assert stats["n_tokens"] == [1] * 4
    t2, _, stats = stage.generate(banned_token_ids=bans, logit_bias=bias, stop_token_ids=stops, min_tokens=[0, 2, 8, 3], **kw)
    assert stats["n_tokens"][0] == 1 and stats["finish_reasons"][2] == "length"
    for t, m in zip(t2, [0, 2, 8, 3]):
        assert not set(text_ids(t)[:m]) & set(stops)
    sm.ops.check_status()
