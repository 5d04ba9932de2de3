"""Stop tokens (EOS) in Stage.generate on HipOps: the prefix property and the early exit of tests/test_stop_tokens.py through
asd_commit_step_stop and the real sampling / verify kernels, for the three tiny stages and once at the full vocabulary."""
import pytest

from tests.stage_scenario import MAX_TOKENS, NAMES, PROMPTS, TEMPERATURE, stage_configs
from tests.stop_scenario import assert_prefix_property, free_run, pick_stop_ids

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


def fresh_manager(ops, configs=None):
    from asd_amd.serving.stages import StageManager
    return StageManager(stage_configs() if configs is None else configs, ops=ops)


@pytest.fixture(scope="module")
def free(ops):
    """The free run of every stage: each on its first generate call of one manager (the seeds of `stage_configs`)."""
    sm = fresh_manager(ops)
    return {n: free_run(sm.get_stage(n)) for n in NAMES}


def test_a_stop_set_returns_the_free_runs_prefix_on_the_gpu(ops, free):
    sm = fresh_manager(ops)
    seen = set()
    for name in NAMES:
        ids = pick_stop_ids(free[name])
        assert 1 <= len(ids) <= 8
        texts, lps, stats = sm.get_stage(name).generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE,
                                                        stop_token_ids=ids)
        want = assert_prefix_property(free[name], ids, texts, lps, stats)
        assert stats["steps"] <= free[name]["stats"]["steps"]
        print(f"stage {name}: stop ids {ids} -> {[(n, how) for n, _, how in want]} in {int(stats['steps'])} steps")
        seen |= {how for _, _, how in want}
    assert seen >= {"first", "accepted", "drawn", None}, seen
    ops.check_status()


def test_all_rows_stopping_in_step_one_ends_the_loop_at_the_first_read_on_the_gpu(ops, free):
    sm = fresh_manager(ops)
    for name in NAMES:
        ids = sorted({row[0] for row in free[name]["tokens"]})
        stage = sm.get_stage(name)
        texts, lps, stats = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, stop_token_ids=ids)
        assert_prefix_property(free[name], ids, texts, lps, stats)
        assert stats["n_tokens"] == [1] * len(PROMPTS) and stats["finish_reasons"] == ["stop"] * len(PROMPTS)
        assert stats["steps"] <= stage.config.sync_every
    ops.check_status()


def test_full_vocabulary_stage_with_a_truncated_target_and_a_stop_set(ops):
    """tiny(vocab=152064), B = 4, max_tokens = 10, target top-k 50 / top-p 0.9; the stop set is Qwen2.5's <|im_end|> and
    <|endoftext|> plus one id of the free run, so that a row does stop."""
    def configs():
        cfgs = stage_configs(vocab=152064, target_top_k=50, target_top_p=0.9)[:2]
        cfgs[1].model_seed = 1                          # a draft that differs from its target: residual draws as well
        return cfgs

    free13 = free_run(fresh_manager(ops, configs()).get_stage("13b"), PROMPTS[:4], 10)
    own = pick_stop_ids(free13, max_ids=1)
    ids = [151645, 151643] + [i for i in own if i not in (151645, 151643)]
    assert len(own) == 1 and len(ids) <= 3
    texts, lps, stats = fresh_manager(ops, configs()).get_stage("13b").generate(prompts=PROMPTS[:4], max_tokens=10,
                                                                                temperature=TEMPERATURE, stop_token_ids=ids)
    want = assert_prefix_property(free13, ids, texts, lps, stats)
    assert "stop" in stats["finish_reasons"]
    print(f"full vocabulary: stop ids {ids} -> {[(n, how) for n, _, how in want]}")
    ops.check_status()
