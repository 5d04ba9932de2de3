"""top_n_sigma / top_a / XTC in Stage.generate on distributed.HipOps (serving/stages.py, RELATIVE CUTS), on the three tiny float32
stages of tests/stage_scenario.py at vocabulary 64: through asd_relative_cut_rows, asd_step_uniforms_ex and the real samplers."""
import pytest
import torch

from tests.logit_edit_ref import SEEDS
from tests.stage_scenario import MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, stage_configs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs(vocab=64, dtype=torch.float32))


def _run(stage, **kw):
    texts, lps, _ = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, **kw)
    return texts, [lp.tobytes() for lp in lps]


@pytest.mark.parametrize("name", NAMES[:2])                                      # stage 0, and a verifying stage's own distribution
def test_a_tiny_top_n_sigma_is_greedy_decoding(manager, name):
    stage = manager.get_stage(name)
    greedy = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0)[0]
    assert _run(stage, top_n_sigma=1e-6)[0] == greedy                            # only the maximum's ties survive the cut
    plain = _run(stage)
    mixed = _run(stage, top_n_sigma=[1e-6, 0] + [1e-6] * (len(PROMPTS) - 2))
    assert mixed[0][0] == greedy[0] and (mixed[0][1], mixed[1][1]) == (plain[0][1], plain[1][1])   # the off row: bit for bit
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES[:2])
def test_xtc_coins_come_from_the_unused_word(manager, name):
    stage = manager.get_stage(name)
    plain = _run(stage)
    assert _run(stage, xtc_probability=1e-9) == plain                            # coins drawn, none under q: no other uniform moved
    on = _run(stage, xtc_probability=1.0, xtc_threshold=0.05)
    assert on == _run(stage, xtc_probability=1.0, xtc_threshold=0.05) and on != plain
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES[:2])
def test_top_a_and_an_unseeded_xtc_call_run(manager, name):
    stage = manager.get_stage(name)
    assert _run(stage, top_a=0.5) != _run(stage)
    texts = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, xtc_probability=0.5)[0]
    assert all(len(t.split()) == MAX_TOKENS for t in texts)
