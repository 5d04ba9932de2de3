"""Per-request max_tokens and multi-token stop sequences in Stage.generate on HipOps: the prefix property, the per-row limits, the
combined run and the greedy run of tests/test_finish.py through asd_commit_step_finish and the real sampling / verify kernels,
for the three tiny stages (vocab 1000, max_tokens 12, draft_len 4)."""
import pytest

from tests.finish_scenario import KINDS, assert_finish_prefix, check_combined, check_greedy, pick_stop_sequences
from tests.stage_scenario import MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, stage_configs
from tests.stop_scenario import free_run

pytestmark = pytest.mark.gpu

B = len(PROMPTS)
LIMITS = [1, 12, 5, 12, 7]


@pytest.fixture(autouse=True)
def hip_backend():
    import asd_amd
    asd_amd.set_backend(None)
    yield


@pytest.fixture(scope="module")
def ops():
    from asd_amd.distributed import HipOps
    return HipOps()


def fresh_manager(ops):
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs(), ops=ops)


@pytest.fixture(scope="module")
def free(ops):
    """The free run of every stage: each on its first generate call of one manager (the seeds of `stage_configs`)."""
    sm = fresh_manager(ops)
    return {n: free_run(sm.get_stage(n)) for n in NAMES}


def test_stop_sequences_return_the_free_runs_prefix_on_the_gpu(ops, free):
    sm = fresh_manager(ops)
    seen = set()
    for name in NAMES:
        seqs = pick_stop_sequences(free[name])
        assert 1 <= len(seqs) <= 8
        texts, lps, stats = sm.get_stage(name).generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE,
                                                        stop_sequences=[list(s) for s in seqs])
        want = assert_finish_prefix(free[name], [seqs] * B, texts, lps, stats)
        assert stats["steps"] <= free[name]["stats"]["steps"]
        print(f"stage {name}: sequences {seqs} -> {[(n, kind) for n, _, _, kind in want]} in {int(stats['steps'])} steps")
        seen |= {kind for _, _, _, kind in want}
    # stage "13b" drafts with its own weights, so its steps commit whole blocks: all three kinds of match are on offer
    assert seen >= set(KINDS) | {None}, seen
    ops.check_status()


def test_every_row_keeps_its_own_max_tokens_on_the_gpu(ops, free):
    sm = fresh_manager(ops)
    for name in NAMES:
        texts, lps, stats = sm.get_stage(name).generate(prompts=PROMPTS, max_tokens=LIMITS, temperature=TEMPERATURE)
        assert_finish_prefix(free[name], [[]] * B, texts, lps, stats, LIMITS)
        assert stats["n_tokens"] == LIMITS and stats["finish_reasons"] == ["length"] * B
    ops.check_status()


def test_top_logprobs_seeds_and_a_list_per_prompt_together_on_the_gpu(ops):
    stats = check_combined(fresh_manager(ops).get_stage("13b"))
    print(f"combined: {stats['n_tokens']} {stats['finish_reasons']} {stats['stop_matches']}")
    ops.check_status()


def test_greedy_decoding_on_the_gpu(ops):
    want = check_greedy(fresh_manager(ops).get_stage("13b"), LIMITS[::-1])
    print(f"greedy: {[(n, reason, kind) for n, reason, _, kind in want]}")
    ops.check_status()
