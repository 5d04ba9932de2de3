"""token_stats in Stage.generate on distributed.HipOps (serving/stages.py, TOKEN STATS): the scenarios of
tests/test_token_stats_stages.py (tests/token_stats_ref.py) through asd_token_stats and the real samplers, on the three tiny
float32 stages of tests/stage_scenario.py at vocabulary 64; and one two-stage bf16 run at the full vocabulary."""
import pytest
import torch

from tests.logit_edit_ref import SEEDS, run_kept
from tests.per_request_ref import inv_t_of
from tests.stage_scenario import NAMES, PROMPTS, TEMPERATURE, stage_configs
from tests.token_stats_ref import (VOCAB, check_stage_stats, scenario_call_trace, scenario_greedy, scenario_pipeline,
                                   scenario_rows_route, scenario_sampled_ranks, scenario_same_bits, scenario_stops, scenario_values)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs(vocab=VOCAB, dtype=torch.float32))


@pytest.mark.parametrize("n", [0, 3])
@pytest.mark.parametrize("name", NAMES)
def test_values_are_the_reference_numbers_of_the_kept_steps(manager, name, n):
    scenario_values(manager.get_stage(name), n=n)
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_truncated_calls_describe_the_untruncated_distribution(manager, name):
    scenario_values(manager.get_stage(name), n=2, top_k=8, top_p=0.9)
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_greedy_rows_have_rank_one(manager, name):
    scenario_greedy(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_sampled_tokens_can_rank_below_the_arg_max(manager, name):
    scenario_sampled_ranks(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_tokens_logprobs_and_tables_keep_their_bits(manager, name):
    scenario_same_bits(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_call_trace_gains_one_pass_and_one_commit_per_step(manager, name):
    scenario_call_trace(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_rows_route_equals_the_scalar_call_per_row(manager, name):
    scenario_rows_route(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_finished_rows_keep_their_entries(manager, name):
    scenario_stops(manager.get_stage(name))
    manager.ops.check_status()


def test_pipeline_carries_the_entries_and_feeds_the_features(manager):
    scenario_pipeline(manager)
    manager.ops.check_status()


def test_full_vocabulary_two_stage_run():
    """tiny(vocab=152064), B = 4, 8 tokens, two bf16 stages: every kept step's ranks, arg-max ids and tables exactly, log-probs
    within LP_ATOL and entropies within 1e-4 + 1e-5 |H| of f64 on the kept step logits."""
    from asd_amd.serving.stages import StageManager
    cfgs = stage_configs(vocab=152064)[:2]
    cfgs[1].model_seed = 1
    assert cfgs[1].dtype == torch.bfloat16
    sm = StageManager(cfgs)
    for name in NAMES[:2]:
        stage = sm.get_stage(name)
        texts, _, stats = run_kept(stage, prompts=PROMPTS[:4], max_tokens=8, temperature=TEMPERATURE, seed=SEEDS[:4], token_stats=True,
                                   logprobs=5)
        assert stage.step_inputs[0]["logits"].dtype == torch.bfloat16 and stage.step_inputs[0]["logits"].shape[-1] == 152064
        check_stage_stats(stage, texts, stats, inv_t_of(TEMPERATURE), 5, PROMPTS[:4])
    sm.ops.check_status()
