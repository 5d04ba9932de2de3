"""The numpy reference of asd_no_repeat_ngram_rows (tests/ngram_ref.py) against transformers' NoRepeatNGramLogitsProcessor, which
HF generate applies for `no_repeat_ngram_size`; then the parts HF has no notion of -- the left-padding, the step's proposals, the
position offset and the clamps -- against expectations written out by hand."""
import numpy as np
import pytest
import torch

from tests.ngram_ref import banned_after, ref_no_repeat_ngram

NINF = float("-inf")


def _banned(x):
    """-> the set of (b, j, v) (or (b, v)) at -inf."""
    return {tuple(i) for i in torch.isneginf(x).nonzero().tolist()}


def test_reference_agrees_with_transformers_no_repeat_ngram_processor():
    transformers = pytest.importorskip("transformers")
    rng = np.random.default_rng(20)
    V, cases, hits = 9, 0, 0
    for n in range(1, 9):
        proc = transformers.NoRepeatNGramLogitsProcessor(n)
        for length in list(range(1, 20)) + [255, 256, 257]:
            for symbols in (3, 7):
                skew = 1.0 / (1.0 + np.arange(symbols))                             # every other history favours the low ids:
                for k in range(10):                                                  # longer repeats than a uniform draw gives
                    H = (rng.choice(symbols, size=length, p=skew / skew.sum()) if k % 2 else
                         rng.integers(0, symbols, size=length)).astype(np.int64)
                    want = proc(torch.from_numpy(H)[None], torch.zeros(1, V))
                    got = ref_no_repeat_ngram(torch.zeros(1, V), [n], H[None].astype(np.int32), [length], [0], length, length)
                    assert torch.equal(got, want), (n, H.tolist())
                    assert _banned(got) == {(0, t) for t in banned_after(H.tolist(), n)}     # the scenarios' helper, too
                    cases += 1
                    hits += bool(torch.isneginf(got).any())
    assert cases == 3520 and 3 * hits >= cases, (cases, hits)


# ------------------------------------------------------------------------------------------ what HF has no notion of
def test_the_padding_in_front_of_row_start_is_not_history():
    # tokens 0 0 7 0 | start 4: with the padding the bigram 0 -> 0 and 0 -> 7 would ban 0 and 7 behind the trailing 0
    tokens = np.array([[0, 0, 7, 0, 9, 9]], dtype=np.int32)
    assert _banned(ref_no_repeat_ngram(torch.zeros(1, 10), [2], tokens, [4], [2], 4, 6)) == set()           # H = 7 0
    assert _banned(ref_no_repeat_ngram(torch.zeros(1, 10), [2], tokens, [4], [1], 4, 6)) == {(0, 7)}       # H = 0 7 0
    assert _banned(ref_no_repeat_ngram(torch.zeros(1, 10), [2], tokens, [4], [0], 4, 6)) == {(0, 0), (0, 7)}
    assert _banned(ref_no_repeat_ngram(torch.zeros(1, 10), [2], tokens, [4], None, 4, 6)) == set()          # no prompt at all
    # the generated part behind `start` always counts: H = [9, 9] with row_start = None
    assert _banned(ref_no_repeat_ngram(torch.zeros(1, 10), [2], tokens, [6], None, 4, 6)) == {(0, 9)}
    # n = 1 bans every token of H, and only of H
    assert _banned(ref_no_repeat_ngram(torch.zeros(1, 10), [1], tokens, [5], [2], 4, 6)) == {(0, 7), (0, 0), (0, 9)}
    assert _banned(ref_no_repeat_ngram(torch.zeros(1, 10), 1, tokens, [4], [3], 4, 6)) == {(0, 0)}         # one n for every row


def test_proposals_are_appended_and_position_j_sees_n_prev_plus_j():
    tokens = np.array([[1, 2, 3, 0, 0]], dtype=np.int32)                            # committed: 1 2 3 (seq_len 3)
    step = np.array([[1, 2, 4, 1]], dtype=np.int32)
    # K1 = 5, n_prev = 0: position j sees step[:j]
    got = ref_no_repeat_ngram(torch.zeros(1, 5, 6), [2], tokens, [3], [0], 0, 5, step, 0)
    assert _banned(got) == {(0, 1, 2),                       # H = 1 2 3 1: 1 -> 2
                            (0, 2, 3),                       # H = 1 2 3 1 2: 2 -> 3
                            (0, 4, 2)}                       # H = 1 2 3 1 2 4 1: 1 -> 2 (twice); positions 0 and 3: 3 and 4 are new
    # K1 = 1 with n_prev = k is row k of the above
    for k in range(5):
        one = ref_no_repeat_ngram(torch.zeros(1, 6), [2], tokens, [3], [0], 0, 5, step, k)
        assert _banned(one) == {(0, v) for b, j, v in _banned(got) if j == k}, k
    # a trigram across the seam: committed ... 2 3 | proposals 1 2 -> behind "1 2" comes 3
    got = ref_no_repeat_ngram(torch.zeros(1, 6), [3], tokens, [3], [0], 0, 5, step, 2)
    assert _banned(got) == {(0, 3)}
    # wholly inside the proposals: 1 2 4 1 | with n_prev = 4 and committed empty, H = 1 2 4 1 -> 2
    got = ref_no_repeat_ngram(torch.zeros(1, 6), [2], tokens, [0], [0], 0, 5, step, 4)
    assert _banned(got) == {(0, 2)}
    # without step_tok no position sees a proposal
    got = ref_no_repeat_ngram(torch.zeros(1, 3, 6), [1], tokens, [2], [0], 0, 5)
    assert _banned(got) == {(0, j, v) for j in range(3) for v in (1, 2)}


def test_the_clamps():
    tokens = np.array([[4, 5, 4, 5, 4, 5]] * 3, dtype=np.int32)
    # seq_len below start counts as start, above max_len as max_len (start 2, max_len 5)
    got = ref_no_repeat_ngram(torch.zeros(3, 8), [2, 2, 2], tokens, [-3, 99, 3], [0, 0, 0], 2, 5)
    assert _banned(got) == {(1, 5), (2, 5)}                  # H = 4 5 (no earlier 5: nothing) | 4 5 4 5 4 -> 5 | 4 5 4 -> 5
    # row_start below 0 counts as 0, above start as start
    got = ref_no_repeat_ngram(torch.zeros(3, 8), [2, 2, 2], tokens, [4, 4, 4], [-7, 99, 2], 2, 6)
    assert _banned(got) == {(0, 4)}                          # rows 1, 2: H = 4 5, nothing; row 0: H = 4 5 4 5 -> 4
    # an n outside 1..8 skips the row; 8 is the largest
    long = np.array([list(range(8)) + list(range(7))] * 4, dtype=np.int32)
    got = ref_no_repeat_ngram(torch.zeros(4, 9), [9, -1, 0, 8], long, [15] * 4, [0] * 4, 0, 15)
    assert _banned(got) == {(3, 7)}
    # a history token outside [0, V) is compared but never written
    odd = np.array([[-1, 8, -1, 3, -1]], dtype=np.int32)
    got = ref_no_repeat_ngram(torch.zeros(1, 8), [2], odd, [5], [0], 0, 5)
    assert _banned(got) == {(0, 3)}                          # -1 -> 8 (outside V = 8: skipped) and -1 -> 3
    # elements that are -inf already stay, everything else keeps its value
    x = torch.full((1, 8), 2.5)
    x[0, 1] = NINF
    got = ref_no_repeat_ngram(x, [2], odd, [5], [0], 0, 5)
    assert got is x and x.tolist() == [[2.5, NINF, 2.5, NINF, 2.5, 2.5, 2.5, 2.5]]
