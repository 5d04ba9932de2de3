"""Allow-lists in Stage.generate on distributed.HipOps (serving/stages.py, ALLOW-LISTS): the scenarios of
tests/test_token_mask_stages.py (tests/token_mask_ref.py) through asd_logit_mask_rows and the real samplers, on the three tiny
stages of tests/stage_scenario.py, at the replay bar of tests/test_gpu_stages.py; and one two-stage run at the full vocabulary."""
import numpy as np
import pytest

from tests.logit_edit_ref import SEEDS, run_kept
from tests.per_request_ref import inv_t_of
from tests.stage_scenario import NAMES, PROMPTS, check_generation, stage_configs, text_ids
from tests.token_mask_ref import (RESTRICT_TEMPERATURE, allow_list, check_restricted, scenario_greedy, scenario_restrict, scenario_rows_independent,
                                  scenario_single, scenario_top_n, scenario_with_edits)

pytestmark = pytest.mark.gpu

ATOL = 2e-5        # tests/test_gpu_stages.py's bar for a kernel lp against the f64 value at its row


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs())


@pytest.mark.parametrize("name", NAMES)
def test_only_listed_tokens_are_proposed_accepted_or_drawn(manager, name):
    worst = scenario_restrict(manager.get_stage(name), atol=ATOL)
    print(f"[allow-lists] stage {name}: max |lp_drawn - f64| on the masked rows = {worst:.3e}")
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_a_one_id_list_commits_that_id(manager, name):
    scenario_single(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_greedy_takes_the_arg_max_inside_the_list(manager, name):
    scenario_greedy(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_row_b_is_the_call_that_gives_every_row_list_b(manager, name):
    scenario_rows_independent(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_the_list_is_the_ban_of_its_complement(manager, name):
    scenario_with_edits(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_top_n_slots_beyond_the_list_are_empty(manager, name):
    scenario_top_n(manager.get_stage(name))
    manager.ops.check_status()


def test_full_vocabulary_two_stage_run():
    """tiny(vocab=152064), B = 4, 4 tokens through the verifying stage once: a list of 4, one of 17, no list, a list of 1000."""
    from asd_amd.serving.stages import StageManager
    V = 152064
    cfgs = stage_configs(vocab=V)[:2]
    cfgs[1].model_seed = 1                              # a draft that differs from its target: residual draws as well
    sm = StageManager(cfgs)
    stage = sm.get_stage(NAMES[1])
    lists = [allow_list(V, 4, 1), allow_list(V, 17, 2), None, allow_list(V, 1000, 3)]
    kw = dict(prompts=PROMPTS[:4], max_tokens=4, temperature=RESTRICT_TEMPERATURE, seed=SEEDS[:4])   # (replayed: see there)
    base, _, _ = stage.generate(**kw)
    texts, lps, _ = run_kept(stage, allowed_token_ids=lists, **kw)
    check_restricted(stage, texts, lps, lists)
    assert texts[2] == base[2] and sum(t != f for t, f in zip(texts, base)) == 3
    check_generation(stage, texts, lps, inv_t_of(RESTRICT_TEMPERATURE), atol=ATOL, max_tokens=4)
    for b, ids in enumerate(lists):
        assert len(text_ids(texts[b])) == 4 and np.isfinite(lps[b]).all()
    sm.ops.check_status()
