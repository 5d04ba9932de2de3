"""no_repeat_ngram_size, host side (serving/stage_args.py, kernels.check_no_repeat_ngram_rows): every ValueError the module
docstring of serving/stages.py names under NO REPEAT N-GRAM, raised before any launch; the rule that a row keeps a token at its
edges; the refusal of a guided row; the packed form."""
import numpy as np
import pytest
import torch

import asd_amd
from asd_amd import kernels as K
from asd_amd.serving.stage_args import MAX_NGRAM, check_ngram_rows_keep_a_token, check_no_repeat_ngram_size
from asd_amd.serving.stages import StageManager
from tests.ngram_ref import NgramOracleOps, real_ids
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import DRAFT_LEN, NAMES, PROMPTS, stage_configs

V = 64


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


class _NoLaunch(NgramOracleOps):
    def _note(self, name, args):
        raise AssertionError(f"{name} was called before the arguments were refused")


@pytest.fixture(scope="module")
def manager():
    return StageManager(stage_configs(vocab=V), ops=_NoLaunch())


def _refused(stage, match, **kw):
    with pytest.raises(ValueError, match=match):
        stage.generate(**{"prompts": PROMPTS, "max_tokens": 8, **kw})


def test_check_no_repeat_ngram_size():
    assert MAX_NGRAM == 8
    assert check_no_repeat_ngram_size(0, 3) == [0, 0, 0] and check_no_repeat_ngram_size(np.int64(8), 2) == [8, 8]
    assert check_no_repeat_ngram_size([2, 0, np.int32(3)], 3) == [2, 0, 3] and check_no_repeat_ngram_size((1, 8), 2) == [1, 8]
    assert check_no_repeat_ngram_size([], 0) == []
    for bad in (True, 2.0, None, "2", -1, 9, [2, 0], [2, 0, 3, 1], [2, None, 3], [2, True, 3], [2, 1.0, 3], [2, 9, 3], [2, -1, 3]):
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            check_no_repeat_ngram_size(bad, 3)


@pytest.mark.parametrize("name", NAMES)
def test_generate_refuses_bad_values_before_any_launch(manager, name):
    stage = manager.get_stage(name)
    for bad in (True, 2.5, "3", -1, 9, [2, 0], [2, 0, 3, 0, None], [2, 0, 3, 0, 9], [2, 0, 3, 0, False]):
        _refused(stage, "no_repeat_ngram_size", no_repeat_ngram_size=bad)


def test_keep_a_token_rule_at_its_edges():
    none, edits, words = [None], [[]], [[]]
    # without an allow-list: |gone| + bound < vocab; bound = 10 + 20 + 4 = 34
    check_ngram_rows_keep_a_token([2], [10], [20], 4, none, edits, words, 35)
    with pytest.raises(ValueError, match="prompt 0.*no_repeat_ngram_size"):
        check_ngram_rows_keep_a_token([2], [10], [20], 4, none, edits, words, 34)
    # ... with gone = a permanent ban, a stop id under min_tokens and a bad word's last id (a bias of 0 until 0 is no ban)
    gone = [[(1, 0.0, 2 ** 31 - 1), (2, 0.0, 3), (3, 1.5, 0)]]
    check_ngram_rows_keep_a_token([2], [10], [20], 4, none, gone, [[(5, 6)]], 38)
    with pytest.raises(ValueError, match="prompt 0"):
        check_ngram_rows_keep_a_token([2], [10], [20], 4, none, gone, [[(5, 6)]], 37)
    check_ngram_rows_keep_a_token([2], [10], [20], 4, none, gone, [[(5, 2)]], 37)                # the word ends in a banned id: one less
    # with an allow-list: |allowed - gone| > bound
    allowed = tuple(range(100, 135))                                                              # 35 ids
    check_ngram_rows_keep_a_token([2], [10], [20], 4, [allowed], edits, words, 1000)
    with pytest.raises(ValueError, match="prompt 0.*allowed_token_ids"):
        check_ngram_rows_keep_a_token([2], [10], [20], 4, [allowed[:-1]], edits, words, 1000)
    with pytest.raises(ValueError, match="prompt 0"):
        check_ngram_rows_keep_a_token([2], [10], [20], 4, [allowed], [[(100, 0.0, 2 ** 31 - 1)]], words, 1000)
    check_ngram_rows_keep_a_token([2], [10], [20], 4, [allowed], [[(99, 0.0, 2 ** 31 - 1)]], words, 1000)     # a ban outside the list
    # rows with n = 0 are not looked at; the refusal names the row
    check_ngram_rows_keep_a_token([0, 0], [10, 10], [20, 20], 4, [None, (1,)], [[], []], [[], []], 2)
    with pytest.raises(ValueError, match="prompt 1"):
        check_ngram_rows_keep_a_token([0, 3], [10, 10], [20, 20], 4, [None, None], [[], []], [[], []], 34)
    # the row's own limit and prompt length count, not the batch's
    check_ngram_rows_keep_a_token([2, 2], [10, 2], [4, 20], 4, [None, None], [[], []], [[], []], 27)
    with pytest.raises(ValueError, match="prompt 1"):
        check_ngram_rows_keep_a_token([2, 2], [10, 2], [4, 20], 4, [None, None], [[], []], [[], []], 26)


@pytest.mark.parametrize("name", NAMES)
def test_generate_applies_the_rule_with_the_prompts_real_lengths(manager, name):
    stage = manager.get_stage(name)
    real, _ = real_ids(stage, PROMPTS)
    longest = max(len(r) for r in real)
    draft = 0 if stage.draft is None else DRAFT_LEN
    room = V - longest - draft                               # bound = longest + max_tokens + draft < V  <=>  max_tokens < room
    assert room > 1
    _refused(stage, f"prompt {[len(r) for r in real].index(longest)}.*no_repeat_ngram_size", no_repeat_ngram_size=2, max_tokens=room)
    ok = StageManager(stage_configs(vocab=V), ops=NgramOracleOps()).get_stage(name)
    assert all(len(t.split()) == room - 1 for t in ok.generate(prompts=PROMPTS, max_tokens=room - 1, temperature=0.0,
                                                               no_repeat_ngram_size=2)[0])
    # per-prompt limits and sizes: only the rows with n > 0 are held to it
    sizes = [0 if len(r) == longest else 2 for r in real]
    limits = [room if len(r) == longest else 4 for r in real]
    assert ok.generate(prompts=PROMPTS, max_tokens=limits, temperature=0.0, no_repeat_ngram_size=sizes)[0]
    # an allow-list must be larger than the bound
    short = [len(r) + 8 + draft for r in real]
    _refused(stage, "allowed_token_ids", no_repeat_ngram_size=2, allowed_token_ids=list(range(max(short))))
    assert ok.generate(prompts=PROMPTS, max_tokens=8, temperature=0.0, no_repeat_ngram_size=2,
                       allowed_token_ids=list(range(max(short) + 1)))[0]


@pytest.mark.parametrize("name", NAMES)
def test_a_guided_row_with_an_n_is_refused(manager, name):
    stage = manager.get_stage(name)
    kw = dict(stop_token_ids=[2], guided_choice_per_prompt=[None, [(5, 6)], None, None, None])
    _refused(stage, "prompt 1.*guided", no_repeat_ngram_size=2, **kw)
    _refused(stage, "prompt 1.*guided", no_repeat_ngram_size=[0, 1, 0, 0, 0], **kw)
    ok = StageManager(stage_configs(vocab=V), ops=NgramOracleOps()).get_stage(name)
    assert ok.generate(prompts=PROMPTS, max_tokens=8, temperature=0.0, no_repeat_ngram_size=[2, 0, 2, 2, 2], **kw)[0]


def test_the_packed_form():
    ns, first = K.check_no_repeat_ngram_rows([2, 0, 8], [3, 0, 5], 5)
    assert ns == [2, 0, 8] and first == [2, 5, 0]                                                 # row_start = P - len(real)
    assert K.check_no_repeat_ngram_rows([], [], 0) == ([], [])
    assert K.check_no_repeat_ngram_rows([np.int32(1)], [np.int64(2)], np.int64(2)) == ([1], [0])
    for bad in (([2, 0], [3], 5), ([9], [3], 5), ([-1], [3], 5), ([True], [3], 5), ([2.0], [3], 5), ([None], [3], 5),
                ([2], [6], 5), ([2], [-1], 5), ([2], [True], 5), ([2], [3.0], 5), ([2], [3], -1), ([2], [3], 2 ** 31), ([2], [3], True)):
        with pytest.raises(ValueError):
            K.check_no_repeat_ngram_rows(*bad)
    with pytest.raises(ValueError):
        K.pack_no_repeat_ngram([9], [3], 5, "cpu")                                               # checked before anything is uploaded
    with pytest.raises(ValueError, match="CUDA"):
        K.no_repeat_ngram_rows(torch.zeros(1, 8), None, None, None, 4)                            # this package has no CPU path
