"""tfs in Stage.generate on distributed.HipOps (serving/stages.py, TAIL-FREE), on the tiny float32 stages of
tests/stage_scenario.py at vocabulary 64: through asd_tail_free_rows and the real samplers."""
import pytest
import torch

from tests.logit_edit_ref import SEEDS, run_kept
from tests.stage_scenario import MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, stage_configs
from tests.tail_free_ref import tfs_row

pytestmark = pytest.mark.gpu

TINY = 1e-6                                      # every row of the scenario keeps one token under it (asserted below)
INV_T = 1.0 / TEMPERATURE


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs(vocab=64, dtype=torch.float32))


def _run(stage, **kw):
    texts, lps, _ = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, **kw)
    return texts, [lp.tobytes() for lp in lps]


@pytest.mark.parametrize("name", NAMES[:2])                                      # stage 0, and a verifying stage's own distribution
def test_a_tiny_tfs_is_greedy_and_tfs_repeats_itself(manager, name):
    stage = manager.get_stage(name)
    greedy = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0)[0]
    texts = run_kept(stage, prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, tfs=TINY)[0]
    rows = [r for s in stage.step_inputs for r in s["tfs_in"].cpu().float().reshape(-1, 64).numpy()]
    assert rows and all(tfs_row(r, (INV_T, TINY)).kept == 1 for r in rows)       # the reference: one token per row
    assert texts == greedy
    plain = _run(stage)
    mixed = _run(stage, tfs=[TINY, 1.0] + [TINY] * (len(PROMPTS) - 2))
    assert mixed[0][0] == greedy[0] and (mixed[0][1], mixed[1][1]) == (plain[0][1], plain[1][1])   # the off row: bit for bit
    on = _run(stage, tfs=0.9)
    assert on == _run(stage, tfs=0.9) and on != plain                            # repeats itself, differs from plain
    manager.ops.check_status()
