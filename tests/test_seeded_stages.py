"""Per-request seeds on CPU: Stage.generate(seed=...) on the oracle twin that serves asd_step_uniforms from the numpy Philox
reference (tests/philox_ref.py: PhiloxOracleOps), and the seed's way through AdaptiveSpeculativePipeline.

What is checked: which uniform reaches which ops call (bit for bit the reference's slot for its seed, step, slot and stage),
that a seeded call is a function of its arguments alone, that rows do not see each other, that seed=None is the call made
before, the argument rule, and that the pipeline hands every request its own seed whatever it is batched with."""
import asyncio
from dataclasses import replace

import numpy as np
import pytest
import torch

import asd_amd
from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
from asd_amd.serving.stages import StageManager
from tests.oracle_backend import OracleBackend
from tests.philox_ref import PhiloxOracleOps, RecordingOracleOps, as_u64, check_wiring
from tests.stage_scenario import NAMES, PROMPTS, TEMPERATURE, stage_configs, text_ids

MAX_TOKENS = 10
DRAFT_LEN = 3
SEEDS = [0, 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1]                      # one per prompt of PROMPTS
EQ_PROMPTS = ["alpha beta gamma", "delta epsilon zeta", "eta theta iota", "kappa lambda mu"]      # three tokens each
EQ_SEEDS = [42, 123, 456, 789]


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


@pytest.fixture
def no_torch_rand(monkeypatch):
    def boom(*a, **kw):
        raise AssertionError("torch.rand launched inside a seeded call")
    return lambda: monkeypatch.setattr(torch, "rand", boom)


def _manager(ops=None, **kw):
    ops = PhiloxOracleOps() if ops is None else ops
    return StageManager([replace(c, draft_len=DRAFT_LEN, **kw) for c in stage_configs()], ops=ops), ops


def _same(a, b):
    """Two generate results: texts equal, log-probs (and tables) the same bits."""
    assert a[0] == b[0]
    assert len(a[1]) == len(b[1]) and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))
    for key in ("top_token_ids", "top_logprobs"):
        assert (key in a[2]) == (key in b[2])
        if key in a[2]:
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a[2][key], b[2][key]))
    assert a[2]["n_tokens"] == b[2]["n_tokens"] and a[2]["finish_reasons"] == b[2]["finish_reasons"]


# ------------------------------------------------------------------------------------------ 1. wiring
@pytest.mark.parametrize("name", NAMES)
def test_every_uniform_is_the_reference_slot_of_its_seed_step_and_stage(name, no_torch_rand):
    sm, ops = _manager()
    stage = sm.get_stage(name)
    no_torch_rand()
    texts, lps, stats = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS)
    index = NAMES.index(name)
    assert stage.index == index
    steps = check_wiring(ops.log, SEEDS, index, 0 if index == 0 else DRAFT_LEN)
    assert steps == stage.last_steps == ops.names().count("step_uniforms")
    assert all(len(text_ids(t)) == MAX_TOKENS == len(lp) for t, lp in zip(texts, lps))
    if index == 0:
        assert steps == MAX_TOKENS


def test_wiring_with_a_stop_set_and_top_logprobs(no_torch_rand):
    sm, ops = _manager()
    stage = sm.get_stage(NAMES[2])
    free = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS)
    stop = sorted({text_ids(t)[3] for t in free[0]})[:8]             # ids the seeded run is known to commit
    ops.log.clear()
    no_torch_rand()
    texts, lps, stats = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS,
                                       stop_token_ids=stop, logprobs=2)
    steps = check_wiring(ops.log, SEEDS, 2, DRAFT_LEN)
    assert steps == stage.last_steps
    assert "commit_step_stop" in ops.names() and "top_logprobs" in ops.names() and "stop" in stats["finish_reasons"]
    # the seeded run with a stop set is the free seeded run cut behind its first stop id: finished rows keep stepping, so the
    # step index stays every row's own step count
    for b, (t, lp) in enumerate(zip(texts, lps)):
        n = stats["n_tokens"][b]
        assert text_ids(t) == text_ids(free[0][b])[:n] and lp.tobytes() == free[1][b][:n].tobytes()
        assert stats["top_token_ids"][b].shape == (n, 2)


# ------------------------------------------------------------------------------------------ 2. repeat
@pytest.mark.parametrize("name", NAMES[:2])
def test_a_seeded_call_depends_on_its_arguments_alone(name):
    sm, ops = _manager()
    stage = sm.get_stage(name)
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, logprobs=2)
    state = stage.gen.get_state().clone()
    first = stage.generate(seed=SEEDS, **kw)
    assert torch.equal(stage.gen.get_state(), state)                 # the stage's generator is not consumed
    _same(first, stage.generate(seed=SEEDS, **kw))
    # other calls in between: an unseeded one (which does consume the generator) and one with other seeds
    unseeded = stage.generate(**kw)
    assert not torch.equal(stage.gen.get_state(), state)
    other = stage.generate(seed=[s ^ 0x5555 for s in SEEDS], **kw)
    assert other[0] != first[0] and unseeded[0] != first[0]
    _same(first, stage.generate(seed=SEEDS, **kw))
    # another StageConfig.seed (this stage's and the draft's)
    sm2, _ = _manager(seed=987)
    _same(first, sm2.get_stage(name).generate(seed=SEEDS, **kw))


# ------------------------------------------------------------------------------------------ 3. permutation
@pytest.mark.parametrize("name", NAMES[:2])
def test_rows_do_not_see_each_other(name):
    sm, ops = _manager()
    stage = sm.get_stage(name)
    assert {len(stage.tokenizer.encode(p, return_tensors=None)) for p in EQ_PROMPTS} == {3}
    kw = dict(max_tokens=MAX_TOKENS, temperature=TEMPERATURE, logprobs=2)
    base = stage.generate(prompts=EQ_PROMPTS, seed=EQ_SEEDS, **kw)
    perm = [2, 0, 3, 1]
    got = stage.generate(prompts=[EQ_PROMPTS[i] for i in perm], seed=[EQ_SEEDS[i] for i in perm], **kw)
    for j, i in enumerate(perm):
        assert got[0][j] == base[0][i] and got[1][j].tobytes() == base[1][i].tobytes()
        assert got[2]["top_logprobs"][j].tobytes() == base[2]["top_logprobs"][i].tobytes()
    # duplicate prompts: equal seeds give equal rows, different seeds different texts
    p0, p1 = EQ_PROMPTS[:2]
    dup = stage.generate(prompts=[p0, p1, p0, p1], seed=[5, 6, 5, 7], **kw)
    assert dup[0][0] == dup[0][2] and dup[1][0].tobytes() == dup[1][2].tobytes()
    assert dup[0][1] != dup[0][3]
    # ... and a row's text does not depend on what the other rows' seeds are
    swapped = stage.generate(prompts=[p0, p1, p0, p1], seed=[5, 999, 1000, 7], **kw)
    assert swapped[0][0] == dup[0][0] and swapped[0][3] == dup[0][3] and swapped[0][1] != dup[0][1]


# ------------------------------------------------------------------------------------------ 4. default unchanged
@pytest.mark.parametrize("name", NAMES[:2])
def test_seed_none_is_the_call_made_before(name):
    """The twin WITHOUT step_uniforms runs the unseeded call; with it, the same ops-call trace (names and keyword sets) and
    the same outputs."""
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE)
    plain_ops = RecordingOracleOps()
    assert not hasattr(plain_ops, "step_uniforms")
    sm_a, _ = _manager(plain_ops)
    sm_b, ops = _manager()
    a = sm_a.get_stage(name).generate(**kw)
    b = sm_b.get_stage(name).generate(seed=None, **kw)
    _same(a, b)
    assert ops.trace() == plain_ops.trace() and "step_uniforms" not in ops.names()
    assert all(x.tobytes() == y.tobytes() for x, y in zip([e["uniform"] for e in ops.log if e["uniform"] is not None],
                                                          [e["uniform"] for e in plain_ops.log if e["uniform"] is not None]))
    with pytest.raises(AttributeError):                              # a seeded call needs the op: nothing falls back
        sm_a.get_stage(name).generate(seed=1, **kw)


@pytest.mark.parametrize("name", NAMES[:2])
def test_greedy_decoding_ignores_the_seed(name):
    sm, ops = _manager()
    stage = sm.get_stage(name)
    a = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0, seed=SEEDS)
    assert "step_uniforms" not in ops.names() and "verify_greedy" in ops.names()
    _same(a, stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0))


# ------------------------------------------------------------------------------------------ 5. broadcast and validation
def test_an_int_seed_is_broadcast():
    sm, ops = _manager()
    stage = sm.get_stage(NAMES[1])
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE)
    a = stage.generate(seed=2 ** 63 + 5, **kw)
    calls = [e for e in ops.log if e["name"] == "step_uniforms"]
    assert calls and all(e["seeds"].tolist() == [2 ** 63 + 5] * len(PROMPTS) for e in calls)
    _same(a, stage.generate(seed=[2 ** 63 + 5] * len(PROMPTS), **kw))
    _same(a, stage.generate(seed=np.full(len(PROMPTS), 2 ** 63 + 5, np.uint64), **kw))
    _same(a, stage.generate(seed=np.uint64(2 ** 63 + 5), **kw))


@pytest.mark.parametrize("bad", [True, False, 1.0, 1.5, -1, 2 ** 64, "12", [1, 2], [1, 2, 3, 4, 5, 6], [1, 2, None, 4, 5],
                                 [1, 2, 3.0, 4, 5], [1, 2, True, 4, 5], [1, 2, -3, 4, 5], [1, 2, 2 ** 64, 4, 5], [[1, 2, 3, 4, 5]]])
def test_bad_seeds_raise(bad):
    sm, ops = _manager()
    for name in NAMES[:2]:
        with pytest.raises(ValueError, match="seed"):
            sm.get_stage(name).generate(prompts=PROMPTS, max_tokens=2, temperature=TEMPERATURE, seed=bad)
        with pytest.raises(ValueError, match="seed"):                  # greedy ignores a seed, not a malformed one
            sm.get_stage(name).generate(prompts=PROMPTS, max_tokens=2, temperature=0.0, seed=bad)
    assert not ops.log


# ------------------------------------------------------------------------------------------ 6. pipeline
class SeedRecordingStage:
    """The pipeline's stage duck type with the `seed` keyword: logs (prompt, seed) of every row it is handed."""

    def __init__(self, name, cost):
        self.name, self.cost_per_token, self.calls = name, cost, []

    def generate(self, prompts, max_tokens, temperature, return_logprobs=True, **kw):
        self.calls.append(dict(prompts=list(prompts), kw=dict(kw)))
        return [f"{self.name} says" for _ in prompts], [np.array([-0.1, -0.2]) for _ in prompts], {"generation_time_ms": 1.0}


class SeedRecordingManager:
    def __init__(self, names=("8b", "13b", "34b", "70b"), costs=(1.0, 1.6, 4.2, 8.8)):
        self.stages = {n: SeedRecordingStage(n, c) for n, c in zip(names, costs)}

    def get_stage(self, name):
        return self.stages[name]


class WordPredictor:
    def predict(self, prompt, draft_output, draft_logprobs, stage_id, feature_extractor):
        return min(0.99, {"easy": 0.97, "mid": 0.6, "hard": 0.05}.get(prompt.split()[0], 0.5) + 0.2 * stage_id)


def _pipeline(**kw):
    sm = SeedRecordingManager()
    return AdaptiveSpeculativePipeline(sm, WordPredictor(), object(),
                                       PipelineConfig(lambda_value=30.0, stop_rule="full", risk_adjustment=False, **kw)), sm


@pytest.mark.parametrize("grouping", ["predicted_stage", "none"])
def test_pipeline_delivers_each_request_its_own_seed(grouping):
    prompts = ["easy a", "hard a", "mid a", "hard b", "easy b", "mid b", "hard c"]
    seeds = [2 ** 64 - 1, 11, 22, 33, 44, 55, 0]
    pipe, sm = _pipeline(batch_grouping=grouping)
    if grouping == "predicted_stage":
        assert len(set(pipe.predict_stop_stages(prompts).tolist())) >= 2        # the population really splits
    res = pipe.batch_process(prompts, max_tokens=4, seeds=seeds)
    assert len(res) == len(prompts)
    seen = 0
    for stage in sm.stages.values():
        for call in stage.calls:
            assert set(call["kw"]) == {"seed"} and len(call["kw"]["seed"]) == len(call["prompts"])
            for p, s in zip(call["prompts"], call["kw"]["seed"]):
                owner = [i for i, orig in enumerate(prompts) if p == orig or p.startswith(orig + " ")]
                assert len(owner) == 1 and s == seeds[owner[0]], (p, s)
                seen += 1
    assert seen == sum(r.stages_run for r in res) > len(prompts)             # later stages saw subsets
    if grouping == "predicted_stage":
        assert len(sm.stages["8b"].calls) >= 2
    # an int is broadcast; without seeds the keyword is not passed
    for st in sm.stages.values():
        st.calls.clear()
    pipe.batch_process(prompts[:3], max_tokens=4, seeds=9)
    assert all(c["kw"]["seed"] == [9] * len(c["prompts"]) for st in sm.stages.values() for c in st.calls)
    for st in sm.stages.values():
        st.calls.clear()
    pipe.batch_process(prompts[:3], max_tokens=4)
    assert sm.stages["8b"].calls and all(c["kw"] == {} for st in sm.stages.values() for c in st.calls)
    pipe.shutdown()


def test_pipeline_single_requests_and_validation():
    pipe, sm = _pipeline()
    pipe.process_request("hard x", max_tokens=4, seed=77)
    assert sm.stages["8b"].calls[-1]["kw"] == {"seed": [77]} and sm.stages["13b"].calls[-1]["kw"] == {"seed": [77]}
    r = asyncio.run(pipe.process_request_async("hard y", max_tokens=4, request_id="abc", seed=78))
    assert r.request_id == "abc" and sm.stages["8b"].calls[-1]["kw"] == {"seed": [78]}
    pipe.process_request("hard z", max_tokens=4)
    assert sm.stages["8b"].calls[-1]["kw"] == {}
    n = len(sm.stages["8b"].calls)
    for bad in (True, 1.5, -1, 2 ** 64, [5], "5"):
        with pytest.raises(ValueError, match="seed"):
            pipe.process_request("hard x", seed=bad)
    for bad in ([1, 2], [1, None, 3], [1, 2, 3, 4], 1.5, [1, 2, -3], True):
        with pytest.raises(ValueError, match="seed"):
            pipe.batch_process(["easy a", "hard a", "mid a"], seeds=bad)
    assert len(sm.stages["8b"].calls) == n                                     # nothing ran
    pipe.shutdown()


def test_as_u64_wraps_like_the_upload():
    sm, ops = _manager()
    sm.get_stage(NAMES[0]).generate(prompts=PROMPTS, max_tokens=1, temperature=TEMPERATURE, seed=SEEDS)
    assert ops.log[0]["name"] == "step_uniforms" and ops.log[0]["seeds"].tolist() == SEEDS == as_u64(SEEDS).tolist()
