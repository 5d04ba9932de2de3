"""dynatemp_* / smoothing_* in Stage.generate on distributed.HipOps (serving/stages.py, SHAPING), on the three tiny float32
stages of tests/stage_scenario.py at vocabulary 64: through asd_logit_shape_rows and the real samplers."""
import pytest
import torch

from tests.logit_edit_ref import SEEDS, run_kept
from tests.per_request_ref import inv_t_of
from tests.prompt_logprobs_ref import AllCalls
from tests.stage_scenario import DRAFT_LEN, MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, ref_logprob, stage_configs, text_ids

pytestmark = pytest.mark.gpu

ATOL, N = 2e-5, len(PROMPTS)     # tests/test_gpu_stages.py's bar for a kernel lp against the f64 value at its row


@pytest.fixture(scope="module")
def manager():
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs(vocab=64, dtype=torch.float32))


def _run(stage, **kw):                                                        # -> (texts, log-prob bytes, the ops calls' names)
    calls = AllCalls(stage.ops)
    try:
        texts, lps, _ = stage.generate(**dict(dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS), **kw))
    finally:
        calls.close()
    return texts, [lp.tobytes() for lp in lps], calls.names


@pytest.mark.parametrize("name", NAMES[:2])                                      # stage 0, and a verifying stage's own distribution
def test_every_row_off_is_the_call_as_it_was(manager, name):
    stage = manager.get_stage(name)
    plain = _run(stage)
    assert _run(stage, dynatemp_range=0.0, smoothing_factor=[0.0] * N) == plain
    assert "logit_shape_rows" not in plain[2] and "pack_logit_shape" not in plain[2]
    assert "logit_shape_rows" not in _run(stage, temperature=0.0, dynatemp_range=0.3, smoothing_factor=0.0)[2]    # greedy: no call
    manager.ops.check_status()


@pytest.mark.parametrize("name", NAMES[:2])
@pytest.mark.parametrize("kw", [dict(dynatemp_range=[0, 0, 0.5, 0, 0], dynatemp_exponent=2.0),
                                dict(smoothing_factor=[0, 0, 0.4, 0, 0], smoothing_curve=2.0)], ids=["dynatemp", "quadratic"])
def test_one_shaped_prompt_moves_no_other(manager, name, kw):
    stage = manager.get_stage(name)
    plain, on = _run(stage), _run(stage, **kw)
    for b in range(N):
        assert ((on[0][b], on[1][b]) == (plain[0][b], plain[1][b])) == (b != 2), b
    assert on[2].count("pack_logit_shape") == 1


def test_a_verifying_stage_shapes_both_sides_with_their_own_records():
    from asd_amd.serving.stages import StageManager
    sm = StageManager(stage_configs(vocab=64, dtype=torch.float32, smoothing_factor=0.25))     # the DRAFT side: the configuration's
    stage, seen = sm.get_stage(NAMES[1]), []
    orig = sm.ops.logit_shape_rows
    sm.ops.logit_shape_rows = lambda logits, packed: (seen.append((tuple(logits.shape[1:-1]), set(packed.modes))), orig(logits, packed))[1]
    try:
        stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, dynatemp_range=0.3)
    finally:
        del sm.ops.logit_shape_rows
    step = [((), {2})] * DRAFT_LEN + [((DRAFT_LEN + 1,), {1})]                   # K draft tensors [B, V], then the target's [B, K + 1, V]
    assert seen and len(seen) % len(step) == 0 and seen == step * (len(seen) // len(step))
    sm.ops.check_status()


@pytest.mark.parametrize("kw", [dict(dynatemp_range=0.5, dynatemp_exponent=0.5), dict(smoothing_factor=0.4, smoothing_curve=3.0)],
                         ids=["dynatemp", "quadratic"])
def test_returned_logprobs_describe_the_shaped_distribution(manager, kw):
    """Stage 0 commits one token per step.  (Not check_generation: it asserts lp <= 0, and the plain sampler's f32 log-prob of
    a token with probability 1 to the last bit, which a sharpened row can hold, may round to +3e-8.)"""
    stage = manager.get_stage(NAMES[0])
    texts, lps, _ = run_kept(stage, prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, **kw)
    assert len(stage.step_inputs) == MAX_TOKENS
    for i, s in enumerate(stage.step_inputs):
        assert not torch.equal(s["shape_in"], s["logits"])                       # the draw saw the rewritten rows
        for b, text in enumerate(texts):
            want = ref_logprob(s["logits"][b].float().cpu().numpy(), text_ids(text)[i], inv_t_of(TEMPERATURE), float(s["thr"][b]))
            assert abs(float(lps[b][i]) - want) <= ATOL, (i, b, float(lps[b][i]), want)
