"""generate(logit_bias=, banned_token_ids=, min_tokens=) on CPU (serving/stages.py, LOGIT EDITS): every ValueError is raised
before any ops call, and a call whose merged edit lists are empty makes exactly the ops calls of the call without the
keywords."""
import numpy as np
import pytest

import asd_amd
from asd_amd.serving.stages import MAX_LOGIT_EDITS, StageConfig, StageManager, merge_logit_edits
from tests.logit_edit_ref import SEEDS, EditOracleOps
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import NAMES, PROMPTS, TEMPERATURE, stage_configs

N = len(PROMPTS)
V = 1000


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def _manager(**kw):
    ops = EditOracleOps()
    return StageManager(stage_configs(**kw), ops=ops), ops


BAD = [
    # ---- ids: a bool, a non-integer, outside the vocabulary
    dict(banned_token_ids=[True]), dict(banned_token_ids=[1.5]), dict(banned_token_ids=["7"]), dict(banned_token_ids=[-1]),
    dict(banned_token_ids=[V]), dict(banned_token_ids=7), dict(banned_token_ids=[[1], [2], [3], [4], [V]]),
    dict(banned_token_ids=[[1], 2, [3], [4], [5]]),
    dict(logit_bias={True: 1.0}), dict(logit_bias={1.5: 1.0}), dict(logit_bias={"7": 1.0}), dict(logit_bias={-1: 1.0}),
    dict(logit_bias={V: 1.0}), dict(logit_bias=[{1: 1.0}, None, None, None, {V: 1.0}]),
    # ---- biases: NaN, infinite, out of range, no number
    dict(logit_bias={5: float("nan")}), dict(logit_bias={5: float("inf")}), dict(logit_bias={5: 100.5}), dict(logit_bias={5: -101}),
    dict(logit_bias={5: True}), dict(logit_bias={5: "1"}), dict(logit_bias={5: None}), dict(logit_bias=3.0),
    dict(logit_bias=[{5: 1.0}, 2.0, None, None, None]),
    # ---- min_tokens: negative, non-integer
    dict(min_tokens=-1), dict(min_tokens=1.5), dict(min_tokens=True), dict(min_tokens="3"), dict(min_tokens=[0, 1, 2, 3, -4]),
    dict(min_tokens=[0, 1, 2, 3, 4.0]),
    # ---- sequences of the wrong length
    dict(logit_bias=[{5: 1.0}] * (N - 1)), dict(logit_bias=[]), dict(banned_token_ids=[[1]] * (N + 1)), dict(min_tokens=[1] * (N - 1)),
    dict(min_tokens=[]),
    # (more than 1024 entries in one row after merging needs a larger vocabulary: the next test)
    # ---- a row whose banned ids leave no token
    dict(banned_token_ids=list(range(V))), dict(banned_token_ids=[[1]] * (N - 1) + [list(range(V))]),
]


@pytest.mark.parametrize("name", [NAMES[0], NAMES[2]])
def test_bad_values_raise_before_any_launch(name):
    sm, ops = _manager()
    stage = sm.get_stage(name)
    for kw in BAD:
        for temperature in (TEMPERATURE, 0.0):
            with pytest.raises(ValueError):
                stage.generate(prompts=PROMPTS, max_tokens=2, temperature=temperature, **kw)
    assert ops.trace == [] and not ops.calls, (ops.trace, ops.calls)


def test_too_many_entries_and_an_emptied_vocabulary():
    """More than MAX_LOGIT_EDITS = 1024 entries in one row after merging needs a vocabulary above 1024; V = 1000 reaches the
    other bound first.  Both through Stage.generate on a stage of 2000 tokens, and the merge itself."""
    sm, ops = _manager(vocab=2000)
    stage = sm.get_stage(NAMES[0])
    many = {t: 1.0 for t in range(MAX_LOGIT_EDITS + 1)}
    with pytest.raises(ValueError, match="1024"):
        stage.generate(prompts=PROMPTS, max_tokens=2, temperature=TEMPERATURE, logit_bias=many)
    with pytest.raises(ValueError, match="1024"):                                   # 1000 biases + 25 other banned ids: 1025 after merging
        stage.generate(prompts=PROMPTS, max_tokens=2, temperature=TEMPERATURE, logit_bias={t: 1.0 for t in range(1000)},
                       banned_token_ids=[[]] * (N - 1) + [list(range(1000, 1025))])
    assert ops.trace == []
    # exactly 1024 is fine: 1000 biases, 24 bans, and a ban on a biased id merges into one entry
    rows = merge_logit_edits([{t: 1.0 for t in range(1000)}], [tuple(range(999, 1024))], [0], [[]], 2000)
    assert len(rows[0]) == MAX_LOGIT_EDITS and rows[0][999] == (999, 0.0, 2 ** 31 - 1) and rows[0][998] == (998, 1.0, 0)
    # the stop ids under min_tokens count as banned at the first token
    with pytest.raises(ValueError, match="no token"):
        merge_logit_edits([{}], [tuple(range(1, 8))], [2], [[(0,)]], 8)
    assert merge_logit_edits([{}], [tuple(range(1, 7))], [2], [[(0,)]], 8) == [[(0, 0.0, 2)] + [(t, 0.0, 2 ** 31 - 1) for t in range(1, 7)]]


def test_the_merge():
    # a stop id under min_tokens keeps its bias for afterwards; a banned id wins over a bias; a bias of 0 is no entry
    rows = merge_logit_edits([{5: 2.0, 6: -1.0, 7: 0.0, 9: 4.0}, {}], [(6, 8), ()], [3, 0], [[(5,), (8,), (11,)], [(5,)]], V)
    assert rows == [[(5, 2.0, 3), (6, 0.0, 2 ** 31 - 1), (8, 0.0, 2 ** 31 - 1), (9, 4.0, 0), (11, 0.0, 3)], []]


def test_min_tokens_with_a_multi_token_stop_sequence_raises():
    sm, ops = _manager()
    stage = sm.get_stage(NAMES[1])
    for kw in (dict(stop_sequences=[(3, 4)], min_tokens=1),
               dict(stop_sequences_per_prompt=[[], [], [(3, 4, 5)], [], []], min_tokens=[0, 0, 2, 0, 0])):
        with pytest.raises(ValueError, match="multi-token"):
            stage.generate(prompts=PROMPTS, max_tokens=2, temperature=TEMPERATURE, **kw)
    assert ops.trace == []
    # ... only on the rows that have both
    stage.generate(prompts=PROMPTS, max_tokens=2, temperature=TEMPERATURE,
                   stop_sequences_per_prompt=[[], [], [(3, 4, 5)], [], [(9,)]], min_tokens=[1, 1, 0, 1, 1])
    assert "logit_edit_rows" in [n for n, _ in ops.trace]


@pytest.mark.parametrize("temperature", [TEMPERATURE, 0.0])
@pytest.mark.parametrize("name", NAMES)
def test_empty_edits_make_exactly_the_calls_made_before(name, temperature):
    sm, ops = _manager()
    stage = sm.get_stage(name)

    def run(**kw):
        stage.gen.manual_seed(int(stage.config.seed))
        ops.trace.clear()
        ops.calls.clear()
        out = stage.generate(prompts=PROMPTS, max_tokens=4, temperature=temperature, seed=SEEDS, stop_token_ids=(3, 4), **kw)
        return out, list(ops.trace), dict(ops.calls)
    plain, trace, calls = run()
    assert trace or calls
    for kw in (dict(logit_bias={}), dict(banned_token_ids=[]), dict(min_tokens=0),
               dict(logit_bias={}, banned_token_ids=[], min_tokens=0), dict(logit_bias=[None] * N, banned_token_ids=[[]] * N,
                                                                            min_tokens=np.zeros(N, np.int64)),
               dict(logit_bias={5: 0.0, 6: 0})):
        same, t2, c2 = run(**kw)
        assert t2 == trace and c2 == calls, kw
        assert same[0] == plain[0] and all(a.tobytes() == b.tobytes() for a, b in zip(same[1], plain[1]))
    assert "logit_edit_rows" not in [n for n, _ in trace] and "pack_logit_edits" not in [n for n, _ in trace]
    # one entry anywhere: one upload, and one edit call per logits tensor
    _, t3, _ = run(logit_bias=[None] * (N - 1) + [{5: 1.0}])
    names = [n for n, _ in t3]
    steps = stage.last_steps
    assert names.count("pack_logit_edits") == 1
    assert names.count("logit_edit_rows") == (steps if name == NAMES[0] else steps * (stage.config.draft_len + 1))


def test_the_configuration_supplies_the_defaults():
    assert (StageConfig().logit_bias, StageConfig().banned_token_ids, StageConfig().min_tokens) == (None, (), 0)
    sm, ops = _manager(banned_token_ids=(1, 2), logit_bias={7: 1.5}, min_tokens=2, stop_token_ids=(9,))
    stage = sm.get_stage(NAMES[0])
    packed = []
    orig = ops.pack_logit_edits
    ops.pack_logit_edits = lambda rows, device: packed.append(rows) or orig(rows, device)
    stage.generate(prompts=PROMPTS[:2], max_tokens=2, temperature=TEMPERATURE)
    assert packed[-1] == [[(1, 0.0, 2 ** 31 - 1), (2, 0.0, 2 ** 31 - 1), (7, 1.5, 0), (9, 0.0, 2)]] * 2
    stage.generate(prompts=PROMPTS[:2], max_tokens=2, temperature=TEMPERATURE, banned_token_ids=[], min_tokens=0)
    assert packed[-1] == [[(7, 1.5, 0)]] * 2                                       # a keyword that is not None replaces the field
    n = len(packed)
    stage.generate(prompts=PROMPTS[:2], max_tokens=2, temperature=TEMPERATURE, banned_token_ids=[], min_tokens=0, logit_bias={})
    assert len(packed) == n
