"""`Stage.generate(logprobs=5)` on HipOps: the stage-level checks of tests/test_top_logprobs_stages.py through
asd_top_logprobs / asd_commit_top_logprobs -- tiny shapes, vocabulary 1000, 12 tokens; stage 0 and a verifying stage, sampled
and greedy, one stop-token run."""
import numpy as np
import pytest

from tests import top_logprobs_ref as T
from tests.greedy_ref import pick_mid_stop
from tests.stage_scenario import MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, stage_configs

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def hip_backend():
    import asd_amd
    asd_amd.set_backend(None)
    yield


@pytest.fixture(scope="module")
def ops():
    from asd_amd.distributed import HipOps
    return HipOps()


def _stage(ops, name, **kw):
    """A fresh manager per run (the runs compared below must start from the same generator state), one HipOps for all."""
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs(**kw), ops=ops).get_stage(name)


def _inv_t(temperature):
    return 1.0 if temperature == 0.0 else float(np.float32(1.0 / temperature))


@pytest.mark.parametrize("temperature", [TEMPERATURE, 0.0], ids=["sampled", "greedy"])
@pytest.mark.parametrize("name", NAMES[:2])
def test_generate_with_logprobs(ops, name, temperature):
    texts, lps, stats = T.run(_stage(ops, name), temperature)
    assert "top_logprobs" not in stats
    stage = _stage(ops, name)
    t2, lp2, st2 = T.run(stage, temperature, T.N_TOP, keep=True)
    assert t2 == texts and all(a.tobytes() == b.tobytes() for a, b in zip(lp2, lps))
    assert st2["n_tokens"] == [MAX_TOKENS] * len(PROMPTS) and len(stage.step_inputs) == st2["steps"]
    worst = T.check_tables(stage.step_inputs, t2, lp2, st2, T.N_TOP, _inv_t(temperature), greedy=temperature == 0.0)
    print(f"stage {name} T={temperature}: max |top_lp - f64| = {worst:.3g} over {len(stage.step_inputs)} steps")
    ops.check_status()


@pytest.mark.parametrize("name", NAMES[:2])
def test_untruncated_table_entry_is_the_returned_logprob(ops, name):
    """Truncation off (top_p = 1.0): the committed token's log-prob and its table entry come from two kernels, each within 2e-5
    of f64."""
    texts, lps, stats = T.run(_stage(ops, name, top_p=1.0), TEMPERATURE, T.N_TOP)
    worst, found = T.pair_gap(texts, lps, stats)
    print(f"stage {name}: {found} committed tokens found in their rows, max gap {worst:.3g}")
    assert found >= len(PROMPTS) * MAX_TOKENS // 4 and worst <= T.PAIR_ATOL, (worst, found)
    ops.check_status()


def test_stop_token_run(ops):
    name = NAMES[1]
    free = T.run(_stage(ops, name), TEMPERATURE)[0]
    b0, i0, stop_id = pick_mid_stop(free)
    texts, lps, stats = T.run(_stage(ops, name), TEMPERATURE, stop_token_ids=(stop_id,))
    stage = _stage(ops, name)
    t2, lp2, st2 = T.run(stage, TEMPERATURE, T.N_TOP, keep=True, stop_token_ids=(stop_id,))
    assert t2 == texts and all(a.tobytes() == b.tobytes() for a, b in zip(lp2, lps))
    assert st2["finish_reasons"] == stats["finish_reasons"] and st2["finish_reasons"][b0] == "stop"
    assert st2["n_tokens"][b0] == i0 + 1 < MAX_TOKENS
    T.check_tables(stage.step_inputs, t2, lp2, st2, T.N_TOP, _inv_t(TEMPERATURE), greedy=False)
    ops.check_status()
