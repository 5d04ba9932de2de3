"""generate(bad_words=, bad_words_per_prompt=) on CPU (serving/stages.py, BAD WORDS): every bad value raises ValueError before
any ops call and before the prompts are encoded, from the stage and through the pipeline; duplicates collapse; a string is
encoded like a stop string; the configuration supplies the default and a keyword that is not None replaces it."""
import numpy as np
import pytest

import asd_amd
from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
from asd_amd.serving.stage_args import (MAX_BAD_WORD_LEN, MAX_BAD_WORDS, _check_stop_sequences, check_bad_words,
                                        check_rows_keep_a_token)
from asd_amd.serving.stages import StageConfig, StageManager
from tests.bad_words_ref import BadWordsOracleOps, check_no_word
from tests.logit_edit_ref import SEEDS
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import NAMES, PROMPTS, TEMPERATURE, LogprobPredictor, stage_configs, text_ids

N = len(PROMPTS)
V = 1000


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def _manager(**kw):
    ops = BadWordsOracleOps()
    return StageManager(stage_configs(**kw), ops=ops), ops


def _last(row):
    """One per-prompt argument whose last prompt holds `row`."""
    return [[] for _ in range(N - 1)] + [row]


MANY = [(i, i + 1) for i in range(MAX_BAD_WORDS + 1)]              # 257 distinct words
BAD = [dict(bad_words=[(1, True)]), dict(bad_words=[(1, 2.0)]), dict(bad_words=[(1, V)]), dict(bad_words=[(-1, 2)]),
       dict(bad_words=[(1, None)]), dict(bad_words=[()]), dict(bad_words=[(1, 2), []]), dict(bad_words=[""]),
       dict(bad_words=[tuple(range(MAX_BAD_WORD_LEN + 1))]), dict(bad_words=["a b c d e f g h i"]), dict(bad_words=MANY),
       dict(bad_words=MANY[:200], bad_words_per_prompt=_last(MANY[200:])),
       dict(bad_words_per_prompt=[[(1, 2)]] * (N - 1)), dict(bad_words_per_prompt=[[(1, 2)]] * (N + 1)), dict(bad_words_per_prompt=[]),
       dict(bad_words_per_prompt="abcde"), dict(bad_words_per_prompt=5), dict(bad_words="abc"), dict(bad_words=5),
       dict(bad_words=[5]), dict(bad_words=[(1, 2), 3]), dict(bad_words_per_prompt=_last("abc")), dict(bad_words_per_prompt=_last([7])),
       dict(bad_words_per_prompt=_last([(1, 2.5)])), dict(bad_words=np.array([[1.0, 2.0]])),
       # a row that would keep no token.  With an allow-list: its ids are all some word's LAST id, whatever the prefix ...
       dict(allowed_token_ids=[3, 4], bad_words=[(9, 3), (4,)]),
       dict(allowed_token_ids=[[3, 4]] + [None] * (N - 1), bad_words_per_prompt=[[(9, 8, 3), (7, 4)]] + [[] for _ in range(N - 1)]),
       dict(allowed_token_ids=[3, 4, 5], banned_token_ids=[5], bad_words=[(9, 3), (1, 4)]),
       # ... and without one: 744 banned ids and the last ids of 256 words cover the vocabulary of 1000
       dict(banned_token_ids=list(range(744)), bad_words=[(0, t) for t in range(744, V)])]


@pytest.mark.parametrize("name", [NAMES[0], NAMES[2]])
def test_bad_values_raise_before_any_launch(name):
    sm, ops = _manager()
    stage = sm.get_stage(name)
    encoded = []
    stage.encode_prompts = lambda *a: encoded.append(a) or 1 / 0              # the checks come first
    stage._encode = lambda *a: encoded.append(a) or 1 / 0
    for kw in BAD:
        for temperature in (TEMPERATURE, 0.0):
            with pytest.raises(ValueError):
                stage.generate(prompts=PROMPTS, max_tokens=2, temperature=temperature, **kw)
    assert ops.trace == [] and not ops.calls and not encoded, (ops.trace, ops.calls)


def test_bad_values_name_what_is_wrong():
    sm, _ = _manager()
    stage = sm.get_stage(NAMES[1])
    for kw, text in ((dict(bad_words=[(1, V)]), "bad_words token ids"), (dict(bad_words=[()]), "1..8 token ids"),
                     (dict(bad_words=MANY), "257 distinct bad_words"), (dict(bad_words="abc"), "bad_words must be a list"),
                     (dict(bad_words_per_prompt=[[]]), r"one list per prompt \(5\)"),
                     (dict(allowed_token_ids=[[3, 4]] + [None] * (N - 1), bad_words=[(9, 3), (4,)]), "prompt 0"),
                     (dict(banned_token_ids=list(range(744)), bad_words_per_prompt=_last([(0, t) for t in range(744, V)])), "prompt 4")):
        with pytest.raises(ValueError, match=text):
            stage.generate(prompts=PROMPTS, max_tokens=2, **kw)


def test_bad_values_raise_through_the_pipeline_before_any_launch():
    sm, ops = _manager()
    pipe = AdaptiveSpeculativePipeline(sm, LogprobPredictor(), object(), PipelineConfig(lambda_value=30.0, stage_names=NAMES))
    for words in ([(1, True)], [(1, V)], [()], [tuple(range(9))], MANY, "abc", 5, [[(1, 2)]] * (N - 1), [(1, 2), [(3, 4)]],
                  _last([(1, 2.5)])):
        with pytest.raises(ValueError):
            pipe.batch_process(PROMPTS, max_tokens=2, temperature=TEMPERATURE, bad_words=words)
    with pytest.raises(ValueError, match="bad_words"):
        pipe.process_request(PROMPTS[0], max_tokens=2, bad_words=[[(1, 2)]])     # one list, not one per request
    pipe.shutdown()
    assert ops.trace == [] and not ops.calls, (ops.trace, ops.calls)


def test_the_row_keeps_a_token_rule_is_conservative():
    rows = [[(0, t) for t in range(50, 300)]]
    edits = [[(t, 0.0, 2 ** 31 - 1) for t in range(50)]]
    with pytest.raises(ValueError, match="prompt 0"):
        check_rows_keep_a_token([None], edits, rows, 300)                          # 50 banned ids + 250 last ids = the vocabulary
    check_rows_keep_a_token([None], edits, [rows[0][1:]], 300)                     # one token left
    check_rows_keep_a_token([None], edits)                                        # the two-argument call still works
    with pytest.raises(ValueError, match="prompt 1"):
        check_rows_keep_a_token([None, (3, 4)], [[], []], [[], [(9, 3), (4,)]], 300)
    check_rows_keep_a_token([None, (3, 4, 5)], [[], []], [[], [(9, 3), (4,)]], 300)
    with pytest.raises(ValueError, match="prompt 1"):                              # a min_tokens ban counts (until > 0)
        check_rows_keep_a_token([None, (3, 4, 5)], [[], [(5, 0.0, 2)]], [[], [(9, 3), (4,)]], 300)


def test_duplicates_collapse_and_a_string_is_encoded_like_a_stop_string():
    sm, _ = _manager()
    tok = sm.get_stage(NAMES[0]).tokenizer
    text = "mid length prompt"
    (ids,) = _check_stop_sequences([text], V, tok)
    assert 1 <= len(ids) <= MAX_BAD_WORD_LEN
    rows = check_bad_words([text, (1, 2), [1, 2], (3,), np.array([1, 2])], [[(3,), (4, 5)], [list(ids)], []], 3, V, tok)
    assert rows == [[ids, (1, 2), (3,), (4, 5)], [ids, (1, 2), (3,)], [ids, (1, 2), (3,)]]
    assert check_bad_words(None, None, 2, V, tok) == [[], []] and check_bad_words((), [None, []], 2, V, tok) == [[], []]
    # 300 entries, 256 distinct: accepted; one more distinct word: refused
    assert len(check_bad_words(MANY[:256] + MANY[:44], None, 1, V, tok)[0]) == MAX_BAD_WORDS
    with pytest.raises(ValueError, match="prompt 0: 257"):
        check_bad_words(MANY[:256] + MANY[:44], [[(900, 901)]], 1, V, tok)


def test_the_configuration_supplies_the_default():
    assert tuple(StageConfig().bad_words) == ()
    kw = dict(prompts=PROMPTS, max_tokens=6, temperature=TEMPERATURE, seed=SEEDS)
    sm, _ = _manager()
    stage = sm.get_stage(NAMES[1])
    base = [text_ids(t) for t in stage.generate(**kw)[0]]
    words = [(t[1],) for t in base] + [tuple(base[0][2:4])]
    want = stage.generate(**kw, bad_words=words)
    sm, ops = _manager(bad_words=words)
    stage = sm.get_stage(NAMES[1])
    got = stage.generate(**kw)
    assert got[0] == want[0] and all(a.tobytes() == b.tobytes() for a, b in zip(got[1], want[1]))
    check_no_word(got[0], [words] * N)
    assert "bad_words_rows" in [n for n, _ in ops.trace]
    # the per-prompt lists come BEHIND the configuration's
    own = [[(text_ids(t)[0],)] for t in got[0]]
    both = stage.generate(**kw, bad_words_per_prompt=own)
    check_no_word(both[0], [words + o for o in own])
    ops.trace.clear()
    plain = stage.generate(**kw, bad_words=[])                                    # a keyword that is not None replaces the field
    assert not [n for n, _ in ops.trace if "bad_words" in n]
    assert [text_ids(t) for t in plain[0]] == base
