"""Multi-token bad words in Stage.generate on distributed.HipOps (serving/stages.py, BAD WORDS): the scenarios of
tests/test_bad_words_stages.py (tests/bad_words_ref.py) through asd_bad_words_rows and the real samplers, on the three tiny
stages of tests/stage_scenario.py; and one two-stage run at the full vocabulary."""
import pytest

from tests.bad_words_ref import (check_kept_bans, check_no_word, scenario_call_trace, scenario_composition, scenario_greedy_replay,
                                 scenario_rows_independent, scenario_sampled)
from tests.logit_edit_ref import SEEDS, run_kept
from tests.stage_scenario import NAMES, PROMPTS, TEMPERATURE, stage_configs, text_ids

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs())


@pytest.mark.parametrize("name", NAMES)
def test_greedy_replay_changes_the_token_that_would_complete_the_word(manager, name):
    scenario_greedy_replay(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_sampled_rows_hold_no_word_and_every_kept_step_has_the_reference_bans(manager, name):
    scenario_sampled(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_row_b_is_the_call_that_gives_every_row_its_list(manager, name):
    scenario_rows_independent(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_composes_with_allow_list_bias_penalties_top_n_and_a_stop_id(manager, name):
    scenario_composition(manager.get_stage(name))
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES)
def test_call_trace(manager, name):
    scenario_call_trace(manager.get_stage(name))
    manager.ops.check_status()


def test_full_vocabulary_two_stage_run():
    """tiny(vocab=152064), B = 4, 8 tokens, two stages, a draft that differs from its target (rejected proposals as well): a
    one-token word, a bigram and a trigram per row under the replay of tests/bad_words_ref.py::check_kept_bans."""
    from asd_amd.serving.stages import StageManager
    cfgs = stage_configs(vocab=152064)[:2]
    cfgs[1].model_seed = 1
    sm = StageManager(cfgs)
    stage = sm.get_stage(NAMES[1])
    kw = dict(prompts=PROMPTS[:4], max_tokens=8, temperature=TEMPERATURE, seed=SEEDS[:4])
    base = [text_ids(t) for t in stage.generate(**kw)[0]]
    rows = [[(t[-1],), tuple(t[0:2]), tuple(t[2:5])] for t in base]
    texts, _, _ = run_kept(stage, bad_words_per_prompt=rows, **kw)
    check_no_word(texts, rows)
    two, _ = check_kept_bans(stage, texts, rows, PROMPTS[:4])
    assert two > 0
    sm.ops.check_status()
