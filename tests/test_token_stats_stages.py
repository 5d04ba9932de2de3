"""token_stats in Stage.generate and the pipeline, on CPU: the three tiny stages of tests/stage_scenario.py at vocabulary 64 on
the oracle twin of tests/token_stats_ref.py, whose token_stats is the numpy reference of asd_token_stats.  The scenarios are
those tests/test_gpu_token_stats_stages.py runs on the kernel."""
import numpy as np
import pytest

import asd_amd
from asd_amd.serving.stages import StageManager
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import NAMES, PROMPTS, stage_configs
from tests.token_stats_ref import (KEYS, VOCAB, TokenStatsOracleOps, ref_token_stats, scenario_call_trace, scenario_greedy,
                                   scenario_pipeline, scenario_rows_route, scenario_sampled_ranks, scenario_same_bits,
                                   scenario_stops, scenario_values)


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def _manager(**kw):
    ops = TokenStatsOracleOps()
    return StageManager(stage_configs(vocab=VOCAB, **kw), ops=ops), ops


def test_reference_on_a_hand_made_step():
    """ref_token_stats itself: live rows, the scored token, the neutral rows, ties by id, a flat row."""
    V = 8
    x = np.zeros((2, 3, V), np.float32)
    x[0, 0] = [0, 3, 3, 1, 0, 0, 0, 0]
    x[1, 1, 5] = -np.inf
    stat_id, stat_val, top_id, top_lp = ref_token_stats(x, [[2, 4], [1, 1]], [1, 7], [6, 3], n=2)
    assert stat_id[0].tolist() == [[2, 1], [7, 0], [0, -1]]             # tok 2 ties with id 1; drawn 6 on a flat row; not live
    assert stat_id[1].tolist() == [[2, 0], [2, 0], [4, 0]]              # n_acc 7 is clamped to 2: tok, tok, drawn
    assert stat_val[0, 2].tolist() == [0.0, 0.0] and top_id[0, 2].tolist() == [-1, -1] and np.isneginf(top_lp[0, 2]).all()
    assert abs(stat_val[0, 1, 0] - np.log(V)) < 1e-12 and abs(stat_val[0, 1, 1] + np.log(V)) < 1e-12
    assert abs(stat_val[1, 1, 0] - np.log(V - 1)) < 1e-12               # a -inf element carries no mass
    assert top_id[0, 0].tolist() == [1, 2] and top_lp[0, 0, 0] == stat_val[0, 0, 1]
    x[1, 2, 0] = np.nan
    x[0, 0] = -np.inf
    stat_id, stat_val, _, _ = ref_token_stats(x, [[2, 4], [1, 1]], [0, 2], [6, 0])
    assert np.isnan(stat_val[1, 2, 0]) and stat_id[1, 2, 0] == 0        # a NaN element, and a NaN target
    assert np.isnan(stat_val[0, 0, 0]) and stat_id[0, 0].tolist() == [7, -1] and np.isneginf(stat_val[0, 0, 1])


@pytest.mark.parametrize("n", [0, 3])
@pytest.mark.parametrize("name", NAMES)
def test_values_are_the_reference_numbers_of_the_kept_steps(name, n):
    sm, _ = _manager()
    scenario_values(sm.get_stage(name), n=n)


@pytest.mark.parametrize("name", NAMES)
def test_truncated_calls_describe_the_untruncated_distribution(name):
    sm, _ = _manager()
    scenario_values(sm.get_stage(name), n=2, top_k=8, top_p=0.9)


@pytest.mark.parametrize("name", NAMES)
def test_greedy_rows_have_rank_one(name):
    sm, _ = _manager()
    scenario_greedy(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_sampled_tokens_can_rank_below_the_arg_max(name):
    sm, _ = _manager()
    scenario_sampled_ranks(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_tokens_logprobs_and_tables_keep_their_bits(name):
    sm, _ = _manager()
    scenario_same_bits(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_call_trace_gains_one_pass_and_one_commit_per_step(name):
    sm, ops = _manager()
    scenario_call_trace(sm.get_stage(name))
    # the configuration's value is the default, and None at the call takes it
    sm2, ops2 = _manager(token_stats=True)
    stage = sm2.get_stage(name)
    _, _, stats = stage.generate(prompts=PROMPTS, max_tokens=2, temperature=0.0)
    assert [n for n, _ in ops2.trace].count("token_stats") == stage.last_steps and all(k in stats for k in KEYS)
    del ops2.trace[:]
    _, _, stats = stage.generate(prompts=PROMPTS, max_tokens=2, temperature=0.0, token_stats=False)
    assert "token_stats" not in [n for n, _ in ops2.trace] and stats.keys().isdisjoint(KEYS)


@pytest.mark.parametrize("name", NAMES)
def test_rows_route_equals_the_scalar_call_per_row(name):
    sm, _ = _manager()
    scenario_rows_route(sm.get_stage(name))


@pytest.mark.parametrize("name", NAMES)
def test_finished_rows_keep_their_entries(name):
    sm, _ = _manager()
    scenario_stops(sm.get_stage(name))


def test_pipeline_carries_the_entries_and_feeds_the_features():
    sm, ops = _manager()
    scenario_pipeline(sm)
    assert "token_stats" in [n for n, _ in ops.trace]


def test_quality_predictor_predict_features_is_one_mlp_call():
    from asd_amd.serving.components import FeatureExtractor, QualityPredictor
    import torch
    torch.manual_seed(0)
    q = QualityPredictor()
    feats = FeatureExtractor.extract_device(torch.tensor([[-0.5, -1.0, 0.0], [-2.0, 0.0, 0.0]]),
                                            torch.tensor([[1.0, 2.0, 0.0], [0.5, 0.0, 0.0]]), [3, 4], [2, 1], 1,
                                            n_valid=torch.tensor([2, 1])).numpy()
    got = q.predict_features(feats)
    assert got.shape == (2,) and ((got > 0) & (got < 1)).all()
    want = q(torch.from_numpy(feats)).reshape(-1).numpy()
    assert np.array_equal(got, want)
