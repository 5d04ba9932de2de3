"""generate(allowed_token_ids=) on CPU (serving/stages.py, ALLOW-LISTS): every ValueError is raised before any ops call, equal
lists share one mask, kernels.check_token_mask_rows lays the bits out as include/asd_hip.h says, a row that the bans or
min_tokens would leave with nothing is refused, and a call without a list makes exactly the ops calls made before."""
import numpy as np
import pytest

import asd_amd
from asd_amd.serving.stage_args import check_allowed_token_ids, check_rows_keep_a_token, merge_logit_edits
from asd_amd.serving.stages import StageConfig, StageManager
from tests.logit_edit_ref import SEEDS
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import NAMES, PROMPTS, TEMPERATURE, stage_configs
from tests.token_mask_ref import MaskOracleOps, ref_pack_bits

N = len(PROMPTS)
V = 1000


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def _manager(**kw):
    ops = MaskOracleOps()
    return StageManager(stage_configs(**kw), ops=ops), ops


BAD = [
    # ---- ids: a bool, a non-integer, outside the vocabulary; no sequence at all
    dict(allowed_token_ids=[True]), dict(allowed_token_ids=[1.5]), dict(allowed_token_ids=["7"]), dict(allowed_token_ids=[-1]),
    dict(allowed_token_ids=[V]), dict(allowed_token_ids=7), dict(allowed_token_ids="12"),
    dict(allowed_token_ids=[[1], [2], [3], [4], [V]]), dict(allowed_token_ids=[[1], None, [3], [4], [2.0]]),
    # ---- a mix of ids and lists
    dict(allowed_token_ids=[[1], 2, [3], [4], [5]]), dict(allowed_token_ids=[1, None, 3, 4, 5]),
    # ---- a wrong count
    dict(allowed_token_ids=[[1]] * (N - 1)), dict(allowed_token_ids=[[1]] * (N + 1)), dict(allowed_token_ids=[None] * (N + 1)),
    # ---- an EMPTY list: for the call, and for one prompt
    dict(allowed_token_ids=[]), dict(allowed_token_ids=()), dict(allowed_token_ids=[[1], [], [3], [4], [5]]),
    # ---- a row left with nothing: by its bans, by another prompt's own bans, by min_tokens' stop ids
    dict(allowed_token_ids=[4, 5], banned_token_ids=[5, 4, 9]),
    dict(allowed_token_ids=[[4, 5]] * N, banned_token_ids=[[]] * (N - 1) + [[4, 5]]),
    dict(allowed_token_ids=[None] * (N - 1) + [[4, 5]], banned_token_ids=[4, 5]),
    dict(allowed_token_ids=[4, 5], stop_token_ids=[4, 5], min_tokens=1),
    dict(allowed_token_ids=[4, 5], banned_token_ids=[4], stop_token_ids=[5], min_tokens=[0, 0, 0, 0, 2]),
    dict(allowed_token_ids=[4, 5], stop_sequences=[(4,), (5,)], min_tokens=3),
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


def test_the_check_returns_sorted_distinct_tuples_or_none():
    assert check_allowed_token_ids(None, 3, V) == [None] * 3
    assert check_allowed_token_ids([5, 3, 5, np.int64(999)], 2, V) == [(3, 5, 999)] * 2
    assert check_allowed_token_ids(np.array([7, 0]), 2, V) == [(0, 7)] * 2
    assert check_allowed_token_ids([[2, 1], None, (9,)], 3, V) == [(1, 2), None, (9,)]
    assert check_allowed_token_ids([None, None], 2, V) == [None, None]
    with pytest.raises(ValueError, match="at least one"):
        check_allowed_token_ids([[1], []], 2, V)
    with pytest.raises(ValueError, match="mixes"):
        check_allowed_token_ids([[1], 2], 2, V)
    with pytest.raises(ValueError, match="2 allowed_token_ids lists for 3"):
        check_allowed_token_ids([[1], [2]], 3, V)


def test_a_row_left_with_nothing_names_the_prompt():
    # the merged entries with until > 0 are the permanent bans AND the min_tokens bans; a bias (until 0) takes nothing away
    edits = merge_logit_edits([{4: -5.0}, {}, {}], [(5,), (4,), ()], [0, 2, 2], [[(5,)], [(5,)], [(5,), (4,)]], V)
    check_rows_keep_a_token([(4, 5), (4, 5, 6), None], edits)                      # row 0 keeps 4, row 1 keeps 6, row 2 has no list
    with pytest.raises(ValueError, match="prompt 1"):
        check_rows_keep_a_token([(4, 5), (4, 5), None], edits)                     # 4 banned, 5 held back by min_tokens
    with pytest.raises(ValueError, match="prompt 2"):
        check_rows_keep_a_token([(4, 5), (4, 5, 6), (4, 5)], edits)                # both held back by min_tokens
    with pytest.raises(ValueError, match="prompt 0"):
        check_rows_keep_a_token([(5,), None, None], edits)
    # min_tokens that holds nothing back (no stop id in the list) and a ban outside the list are fine
    sm, ops = _manager()
    stage = sm.get_stage(NAMES[1])
    texts, _, _ = stage.generate(prompts=PROMPTS, max_tokens=3, temperature=TEMPERATURE, allowed_token_ids=[4, 5],
                                 banned_token_ids=[6], stop_token_ids=[7], min_tokens=2)
    assert all(set(t.split()) <= {"t4", "t5"} for t in texts)


def test_bit_layout_of_the_packed_masks():
    from asd_amd.kernels import check_token_mask_rows
    for vocab in (V, 1003, 32, 33, 5):
        W = (vocab + 31) // 32
        ids = sorted({0, min(31, vocab - 1), min(32, vocab - 1), vocab - 1})
        bits, mask_row = check_token_mask_rows([tuple(ids)], vocab)
        assert bits.dtype == np.uint32 and bits.shape == (1, W) and mask_row is None
        want = np.zeros(W, dtype=np.uint32)
        want[0] |= 1                                                               # id 0: bit 0 of word 0
        if vocab > 31:
            want[0] |= np.uint32(1 << 31)                                          # id 31: the top bit of word 0
        if vocab > 32:
            want[1] |= 1                                                           # id 32: bit 0 of word 1
        want[(vocab - 1) >> 5] |= np.uint32(1 << ((vocab - 1) & 31))               # id V - 1
        assert np.array_equal(bits[0], want)
        assert int(sum(bin(int(w)).count("1") for w in bits[0])) == len(ids)
        assert np.array_equal(bits, ref_pack_bits([ids], vocab))
    with pytest.raises(ValueError):
        check_token_mask_rows([(0, V)], V)
    with pytest.raises(ValueError):
        check_token_mask_rows([(-1,)], V)


def test_equal_lists_share_one_mask():
    from asd_amd.kernels import check_token_mask_rows
    a, b = (1, 2, 3), (5, 700)
    bits, mask_row = check_token_mask_rows([a, b, None, a, b, a], V)
    assert bits.shape == (2, 32) and mask_row == [0, 1, -1, 0, 1, 0]
    assert np.array_equal(bits, ref_pack_bits([a, b], V))
    bits, mask_row = check_token_mask_rows([a, a, a], V)
    assert bits.shape == (1, 32) and mask_row is None                              # every row uses mask 0: no index array
    bits, mask_row = check_token_mask_rows([a, None], V)
    assert bits.shape == (1, 32) and mask_row == [0, -1]
    bits, mask_row = check_token_mask_rows([None, None], V)
    assert bits.shape == (0, 32) and mask_row == [-1, -1]
    # ... and the stage hands the distinct lists over once per call
    sm, ops = _manager()
    stage = sm.get_stage(NAMES[0])
    packed = []
    orig = ops.pack_token_masks
    ops.pack_token_masks = lambda rows, vocab, device: packed.append((rows, vocab)) or orig(rows, vocab, device)
    stage.generate(prompts=PROMPTS, max_tokens=2, temperature=TEMPERATURE, allowed_token_ids=[[3, 2, 2], None, [2, 3], (9,), None])
    assert packed == [([(2, 3), None, (2, 3), (9,), None], V)]


@pytest.mark.parametrize("temperature", [TEMPERATURE, 0.0])
@pytest.mark.parametrize("name", NAMES)
def test_no_list_makes_exactly_the_calls_made_before(name, temperature):
    sm, ops = _manager()
    stage = sm.get_stage(name)

    def run(**kw):
        stage.gen.manual_seed(int(stage.config.seed))
        ops.trace.clear()
        ops.calls.clear()
        out = stage.generate(prompts=PROMPTS, max_tokens=4, temperature=temperature, seed=SEEDS, stop_token_ids=(3, 4),
                             logit_bias={5: 1.0}, **kw)
        return out, list(ops.trace), dict(ops.calls)
    plain, trace, calls = run()
    names = [n for n, _ in trace]
    assert "logit_edit_rows" in names and "logit_mask_rows" not in names and "pack_token_masks" not in names
    for kw in (dict(allowed_token_ids=None), dict(allowed_token_ids=[None] * N)):
        same, t2, c2 = run(**kw)
        assert t2 == trace and c2 == calls, kw
        assert same[0] == plain[0] and all(a.tobytes() == b.tobytes() for a, b in zip(same[1], plain[1]))
    # one list anywhere: one upload, and one mask call immediately in front of every edit call
    _, t3, _ = run(allowed_token_ids=[None] * (N - 1) + [[5, 6, 7]])
    names = [n for n, _ in t3]
    steps = stage.last_steps
    assert names.count("pack_token_masks") == 1
    assert names.count("logit_mask_rows") == names.count("logit_edit_rows") == \
        (steps if name == NAMES[0] else steps * (stage.config.draft_len + 1))
    assert all(names[i - 1] == "logit_mask_rows" for i, n in enumerate(names) if n == "logit_edit_rows")


def test_the_configuration_supplies_the_default():
    assert StageConfig().allowed_token_ids is None
    sm, ops = _manager(allowed_token_ids=(8, 3))
    stage = sm.get_stage(NAMES[0])
    packed = []
    orig = ops.pack_token_masks
    ops.pack_token_masks = lambda rows, vocab, device: packed.append(rows) or orig(rows, vocab, device)
    texts, _, _ = stage.generate(prompts=PROMPTS[:2], max_tokens=3, temperature=TEMPERATURE)
    assert packed[-1] == [(3, 8)] * 2 and all(set(t.split()) <= {"t3", "t8"} for t in texts)
    stage.generate(prompts=PROMPTS[:2], max_tokens=3, temperature=TEMPERATURE, allowed_token_ids=[[5], None])
    assert packed[-1] == [(5,), None]                                              # a keyword that is not None replaces the field
