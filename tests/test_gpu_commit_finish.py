"""asd_commit_step_finish through kernels.commit_step_finish against the numpy reference of tests/finish_scenario.py.  Integer /
bit-copy work, so everything is exact: tokens, log-prob bits, seq_len, n_commit, finished, n_finished, matched; the sentinel stays
everywhere the reference leaves it.  The inputs are CONSTRUCTED: every row of a case is one scenario of `SCENARIOS`, built
together with the outcome it must have (tokens appended, reason, matched index), and the reference is first held to that outcome
-- so the cases the file is about really occur -- before the kernel is held to the reference."""
import numpy as np
import pytest

from tests.finish_scenario import MAX_STOP_SEQS, ref_commit_finish
from tests.stop_scenario import LENGTH, STOP, ref_commit_stop

pytestmark = pytest.mark.gpu

SENT_TOK, SENT_LP, SENT_NC, SENT_MATCH = -123456, np.float32(-7.25), -9, -5
START = 4                                              # the "prompt" of every row: positions 0..3
N_FINISHED_0 = 5                                       # the counter is added to, not set
GRID = ((1, 0), (3, 4), (5, 64), (33, 8))


class Row:
    """One row under construction: random committed stream and candidates; a scenario edits it and says what must happen."""

    def __init__(self, rng, K, T, max_len):
        self.K, self.T, self.max_len = K, T, max_len
        self.rng = rng
        self.len = START + int(rng.integers(8, 12))    # >= 7 generated tokens: a full window of history
        self.stream = rng.integers(100, 151000, T).astype(np.int32)     # [:len] is committed, the rest is overwritten below
        self.tok = rng.integers(100, 151000, K).astype(np.int32)
        self.drawn = np.int32(rng.integers(100, 151000))
        self.n_acc = int(rng.integers(0, K + 1))
        self.seqs, self.seq_n_override = [], {}
        self.row_max_len = max_len + int(rng.integers(0, 3))            # no tighter than max_len unless a scenario says so
        self.finished = 0
        self.want = None                               # (appended, reason, matched or None)

    def cand(self):
        return [int(t) for t in self.tok[:self.n_acc]] + [int(self.drawn)]

    def other(self, m=2):
        return tuple(int(t) for t in self.rng.integers(151000, 152000, m))     # a sequence no token of the row can complete

    def plain(self):
        room = max(min(self.max_len, max(self.row_max_len, 0)) - self.len, 0)
        n = min(self.n_acc + 1, room)
        return (n, LENGTH if n == room else 0, None)


def s_none_owned(r):
    r.want = r.plain()


def s_len1_in_prefix(r):
    if r.K < 2:
        return False
    r.n_acc = r.K
    r.seqs = [r.other(), (int(r.tok[1]),)]
    r.want = (2, STOP, 1)


def s_len2_one_step_accepted(r):
    if r.K < 2:
        return False
    r.n_acc = r.K
    r.seqs = [(int(r.tok[0]), int(r.tok[1]))]
    r.want = (2, STOP, 0)


def s_len2_ends_on_drawn(r):
    if r.K < 1:
        return False
    r.n_acc = min(r.K, 3)
    r.seqs = [r.other(8), (int(r.tok[r.n_acc - 1]), int(r.drawn))]
    r.want = (r.n_acc + 1, STOP, 1)


def s_len8_straddles_na0(r):
    r.n_acc = 0
    r.seqs = [tuple(int(t) for t in r.stream[r.len - 7:r.len]) + (int(r.drawn),)]
    r.want = (1, STOP, 0)


def s_len2_straddles_na1(r):
    if r.K < 1:
        return False
    r.n_acc = 1
    r.seqs = [(int(r.stream[r.len - 1]), int(r.tok[0]))]
    r.want = (1, STOP, 0)


def s_len8_straddles_naK(r):
    if r.K < 4:
        return False
    r.n_acc = r.K
    r.seqs = [tuple(int(t) for t in r.stream[r.len - 5:r.len]) + tuple(int(t) for t in r.tok[:3])]
    r.want = (3, STOP, 0)


def s_k64_drawn_at_64(r):
    if r.K != 64:
        return False
    r.n_acc = 64
    r.seqs = [r.other(), (int(r.tok[63]), int(r.drawn))]
    r.want = (65, STOP, 1)


def s_k64_spans_57_64(r):
    if r.K != 64:
        return False
    r.n_acc = 64
    r.seqs = [tuple(int(t) for t in r.tok[57:64]) + (int(r.drawn),)]
    r.want = (65, STOP, 0)


def s_k64_lane_63(r):
    if r.K != 64:
        return False
    r.n_acc = 64
    r.seqs = [tuple(int(t) for t in r.tok[56:64]), (int(r.drawn),)]
    r.want = (64, STOP, 0)


def s_history_shorter_than_the_sequence(r):
    """Three generated tokens; the 8-token sequence is spelled by the prompt's last tokens, those three and the candidates."""
    r.len = START + 3
    r.n_acc = min(r.K, 2)
    c = r.cand()
    r.seqs = [tuple(int(t) for t in r.stream[r.len - (8 - len(c)):r.len]) + tuple(c)]
    assert len(r.seqs[0]) == 8
    r.want = r.plain()


def s_begins_at_start_minus_1(r):
    r.len = START
    r.n_acc = min(r.K, 1)
    c = r.cand()
    r.seqs = [(int(r.stream[START - 1]),) + tuple(c[:1]), (int(r.stream[START - 1]),) + tuple(c)]
    r.want = r.plain()


def s_begins_at_start(r):
    r.len = START + 1
    r.n_acc = 0
    r.seqs = [(int(r.stream[START - 1]), int(r.stream[START]), int(r.drawn)), (int(r.stream[START]), int(r.drawn))]
    r.want = (1, STOP, 1)


def s_first_generated_token_len1(r):
    r.len = START
    r.n_acc = min(r.K, 2)
    r.seqs = [(r.cand()[0],)]
    r.want = (1, STOP, 0)


def s_two_sequences_end_together(r):
    if r.K < 2:
        return False
    r.n_acc = r.K
    r.seqs = [r.other(), (int(r.tok[0]), int(r.tok[1])), (int(r.tok[1]),)]
    r.want = (2, STOP, 1)


def s_the_later_listed_ends_earlier(r):
    if r.K < 3:
        return False
    r.n_acc = r.K
    r.seqs = [(int(r.tok[2]),), (int(r.tok[0]),)]
    r.want = (1, STOP, 1)


def s_match_on_the_last_free_slot(r):
    r.len = r.max_len - r.n_acc - 1
    r.seqs = [(int(r.drawn),)]
    r.want = (r.n_acc + 1, STOP, 0)


def s_match_cut_by_row_max_len(r):
    r.row_max_len = r.len + r.n_acc                    # the drawn token, the match's last, is cut off
    r.seqs = [((int(r.tok[r.n_acc - 1]),) if r.n_acc else (int(r.stream[r.len - 1]),)) + (int(r.drawn),), (int(r.drawn),)]
    r.want = (r.n_acc, LENGTH, None)


def s_match_cut_by_max_len(r):
    if r.K < 2:
        return False
    r.n_acc = r.K
    r.len = r.max_len - 1                              # only candidate 0 fits
    r.seqs = [(int(r.tok[0]), int(r.tok[1])), (int(r.tok[1]),)]
    r.want = (1, LENGTH, None)


def s_row_limit_reached_without_a_match(r):
    r.row_max_len = r.len + 1
    r.seqs = [r.other()]
    r.want = (1, LENGTH, None)


def s_row_max_len_negative(r):
    r.row_max_len = -3
    r.seqs = [(int(r.drawn),)]
    r.want = (0, LENGTH, None)


def s_enters_stopped(r):
    r.finished = STOP
    r.seqs = [(int(r.drawn),)]
    r.want = (0, STOP, None)


def s_enters_at_length(r):
    r.finished = LENGTH
    r.want = (0, LENGTH, None)


def s_enters_full(r):
    r.len = r.max_len
    r.seqs = [(int(r.drawn),)]
    r.want = (0, LENGTH, None)


def s_only_rejected_tokens_spell_it(r):
    if r.K < 3:
        return False
    r.n_acc = 1
    r.seqs = [(int(r.tok[1]),), (int(r.tok[0]), int(r.tok[1])), (int(r.tok[1]), int(r.drawn)), (int(r.tok[r.K - 1]), int(r.drawn))]
    r.want = r.plain()


def s_sixteen_owned_the_last_matches(r):
    r.seqs = [r.other(1 + i % 8) for i in range(MAX_STOP_SEQS - 1)] + [(int(r.drawn),)]
    r.want = (r.n_acc + 1, STOP, MAX_STOP_SEQS - 1)


def s_lengths_outside_1_to_8_never_match(r):
    r.seqs = [(int(r.drawn),), (int(r.drawn),), (int(r.drawn),)]
    r.seq_n_override = {0: 0, 1: 9, 2: -1}
    r.want = r.plain()


def s_n_acc_out_of_range(r):
    raw = -3 if r.rng.integers(0, 2) else r.K + 5
    r.n_acc = 0 if raw < 0 else r.K
    r.seqs = [r.other()]
    r.want = r.plain()
    r.raw_n_acc = raw


SCENARIOS = [f for n, f in sorted(globals().items()) if n.startswith("s_")]


def _case(B, K, first, shared=False):
    """Rows first, first + 1, ... of the scenario list (those K allows) -> the inputs and, per row, what must happen."""
    rng = np.random.default_rng(B * 10000 + K * 100 + first)
    T = K + 24
    max_len = T - 2                                    # rows are longer than max_len: nothing past max_len may be written
    rows, i = [], first
    while len(rows) < B:
        r = Row(rng, K, T, max_len)
        fn = SCENARIOS[i % len(SCENARIOS)]
        i += 1
        if fn(r) is False:
            continue
        r.name = fn.__name__
        rows.append(r)
    tok = np.stack([r.tok for r in rows]).reshape(B, K)
    lp_tok = (-rng.uniform(0, 20, (B, K))).astype(np.float32)
    if K:
        lp_tok.reshape(-1)[::3] = -np.inf              # bits, not values
        lp_tok.reshape(-1)[1::5] = np.float32(-0.0)
    lp_drawn = (-rng.uniform(0, 20, B)).astype(np.float32)
    lp_drawn[::4] = np.nan
    out_tok = np.full((B, T), SENT_TOK, np.int32)
    for b, r in enumerate(rows):
        out_tok[b, :r.len] = r.stream[:r.len]
    seq_rows, seq_n, row_first = [], [], [0]
    for r in rows:
        for k, s in enumerate(r.seqs):
            seq_rows.append(list(s)[:8] + [SENT_TOK] * (8 - len(s)))    # slots behind a sequence's length are ignored
            seq_n.append(r.seq_n_override.get(k, len(s)))
        row_first.append(len(seq_rows))
    c = dict(tok=tok, lp_tok=lp_tok, n_acc=np.array([getattr(r, "raw_n_acc", r.n_acc) for r in rows], np.int32),
             drawn=np.array([r.drawn for r in rows], np.int32), lp_drawn=lp_drawn,
             seq_len=np.array([r.len for r in rows], np.int32), finished=np.array([r.finished for r in rows], np.int32),
             out_tok=out_tok, out_lp=np.full((B, T), SENT_LP, np.float32), matched=np.full(B, SENT_MATCH, np.int32),
             seq_tok=np.array(seq_rows, np.int32).reshape(-1, 8), seq_n=np.array(seq_n, np.int32),
             row_first=np.array(row_first, np.int32), row_max_len=np.array([r.row_max_len for r in rows], np.int32),
             T=T, max_len=max_len, rows=rows)
    if shared:                                         # every row owns the first 16 sequences of the whole case
        c.update(seq_tok=c["seq_tok"][:MAX_STOP_SEQS], seq_n=c["seq_n"][:MAX_STOP_SEQS], row_first=None)
    return c


def _reference(c, state=None, n_finished=N_FINISHED_0):
    B, K = c["tok"].shape
    seq_len, out_tok, out_lp, finished, matched = state or (c["seq_len"], c["out_tok"], c["out_lp"], c["finished"], c["matched"])
    n_seq = len(c["seq_n"])
    return ref_commit_finish(c["tok"] if K else None, c["lp_tok"] if K else None, c["n_acc"], c["drawn"], c["lp_drawn"], seq_len,
                             out_tok, out_lp, finished, n_finished, matched, c["seq_tok"] if n_seq else None,
                             c["seq_n"] if n_seq else None, c["row_first"], c["row_max_len"], START, c["max_len"])


def _device(c, state=None, n_finished=N_FINISHED_0, with_optional=True):
    """One launch on copies of the inputs (or on `state`, the device tensors an earlier launch left) -> the device tensors in the
    reference's order."""
    import torch
    from asd_amd import kernels as Kn
    B, K = c["tok"].shape
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()            # noqa: E731
    if state is None:
        state = [dev(c[k].copy()) for k in ("seq_len", "out_tok", "out_lp", "finished", "matched")]
        state.append(torch.full((1,), n_finished, dtype=torch.int32, device="cuda"))
    seq_len, out_tok, out_lp, finished, matched, nfin = state
    nc = torch.full((B,), SENT_NC, dtype=torch.int32, device="cuda")
    n_seq = len(c["seq_n"])
    Kn.commit_step_finish(dev(c["tok"]) if K else None, dev(c["lp_tok"]) if K else None, dev(c["n_acc"]), dev(c["drawn"]),
                          dev(c["lp_drawn"]), seq_len, out_tok, out_lp, finished, START,
                          seq_tok=dev(c["seq_tok"]) if n_seq else None, seq_n=dev(c["seq_n"]) if n_seq else None,
                          row_first=None if c["row_first"] is None else dev(c["row_first"]), row_max_len=dev(c["row_max_len"]),
                          n_finished=nfin if with_optional else None, matched=matched if with_optional else None,
                          n_commit=nc if with_optional else None, max_len=c["max_len"])
    torch.cuda.synchronize()
    return seq_len, out_tok, out_lp, nc, finished, nfin, matched


NAMES = ("seq_len", "tokens", "lps", "n_commit", "finished", "n_finished", "matched")


def _assert_equal(got, want, names=NAMES):
    for name, g, w in zip(names, got, want):
        g = g.cpu().numpy()
        w = np.asarray(w, dtype=g.dtype).reshape(g.shape)
        assert g.tobytes() == w.tobytes(), name


def _assert_construction(c, ref):
    """The reference did to every row what its scenario was built to have done."""
    ln, tk, lp, nc, fin, nf, mt = ref
    for b, r in enumerate(c["rows"]):
        appended, reason, which = r.want
        assert (int(nc[b]), int(fin[b])) == (appended, reason), (r.name, b, int(nc[b]), int(fin[b]), r.want)
        assert int(mt[b]) == (SENT_MATCH if which is None else which), (r.name, b, int(mt[b]))
        assert int(ln[b]) == r.len + appended
        assert [int(t) for t in tk[b, r.len:r.len + appended]] == r.cand()[:appended]
        assert (tk[b, r.len + appended:] == SENT_TOK).all()
    entering = sum(1 for r in c["rows"] if r.finished)
    assert int(nf) == N_FINISHED_0 + int((fin != 0).sum()) - entering


CASES = [(B, K, first) for B, K in GRID for first in range(0, len(SCENARIOS), B)]


def test_every_scenario_occurs_and_the_reference_gives_its_outcome():
    seen = set()
    for B, K, first in CASES:
        c = _case(B, K, first)
        _assert_construction(c, _reference(c))
        seen |= {r.name for r in c["rows"]}
        assert {int(np.clip(n, 0, K)) for n in c["n_acc"]} >= ({0, 1, K} if B >= 33 else set())
    assert seen == {f.__name__ for f in SCENARIOS}
    # per K of the grid: the scenarios it allows all occur at that K
    for B, K in GRID:
        names = {r.name for b, k, first in CASES if (b, k) == (B, K) for r in _case(b, k, first)["rows"]}
        allowed = {f.__name__ for f in SCENARIOS if f(Row(np.random.default_rng(0), K, K + 24, K + 22)) is not False}
        assert names == allowed, (B, K, allowed - names)
    assert any(len(r.seqs) == 0 for B, K, first in CASES for r in _case(B, K, first)["rows"])


@pytest.mark.parametrize("B,K,first", CASES)
def test_commit_step_finish_matches_the_reference(B, K, first):
    c = _case(B, K, first)
    want = _reference(c)
    _assert_construction(c, want)
    got = _device(c)
    _assert_equal(got, want)
    assert (got[1].cpu().numpy()[:, c["max_len"]:] == SENT_TOK).all()           # nothing past max_len
    # a second launch on the outputs of the first: rows that finished, and what they added to the counter, stay as they are
    before = [t.clone() for t in got]
    want2 = _reference(c, (want[0], want[1], want[2], want[4], want[6]), want[5])
    got2 = _device(c, [got[0], got[1], got[2], got[4], got[6], got[5]])
    _assert_equal(got2, want2)
    done = (before[4] != 0).cpu().numpy()
    assert (got2[3].cpu().numpy()[done] == 0).all()
    for i in (0, 1, 2, 4, 6):
        assert got2[i].cpu().numpy()[done].tobytes() == before[i].cpu().numpy()[done].tobytes(), NAMES[i]
    # n_commit, n_finished and matched may be NULL
    got3 = _device(c, with_optional=False)
    _assert_equal((got3[0], got3[1], got3[2], got3[4]), (want[0], want[1], want[2], want[4]), ("seq_len", "tokens", "lps", "finished"))


@pytest.mark.parametrize("B,K,first", [(B, K, first) for B, K, first in CASES if B > 1 or first % 5 == 0])
def test_without_row_first_every_row_owns_all_sequences(B, K, first):
    c = _case(B, K, first, shared=True)
    want = _reference(c)
    _assert_equal(_device(c), want)


def test_without_row_first_sequences_of_other_rows_stop_a_row():
    stops = 0
    for B, K, first in CASES:
        if B in (3, 5):
            own, shared = _reference(_case(B, K, first)), _reference(_case(B, K, first, shared=True))
            stops += int(((shared[4] == STOP) & (own[4] != STOP)).sum()) + int((shared[6] != own[6]).sum())
    assert stops >= 1


def test_no_sequences_at_all_is_the_length_rule_alone():
    c = _case(33, 8, 0)
    c.update(seq_tok=np.zeros((0, 8), np.int32), seq_n=np.zeros(0, np.int32), row_first=None)
    want = _reference(c)
    assert ((want[4] == STOP) == (c["finished"] == STOP)).all() and (want[4] == LENGTH).sum() > (c["finished"] == LENGTH).sum()
    _assert_equal(_device(c), want)


def test_start_zero_and_a_stream_shorter_than_the_window():
    """start = 0 and two committed tokens: an 8-token sequence would begin at a negative position (never read, no match); a
    3-token one that begins exactly at position 0 stops the row."""
    import torch
    from asd_amd import kernels as Kn
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()            # noqa: E731
    T = 16
    out = np.full((2, T), SENT_TOK, np.int32)
    out[:, :2] = [[11, 12], [21, 22]]
    tok = np.array([[13, 14], [23, 24]], np.int32)
    args = dict(tok=tok, lp_tok=np.full((2, 2), -1.5, np.float32), n_acc=np.array([2, 2], np.int32), drawn=np.array([15, 25], np.int32),
                lp_drawn=np.array([-2.5, -3.5], np.float32))
    seq_tok = np.array([[0, 0, 0, 0, 0, 11, 12, 13], [21, 22, 23, 0, 0, 0, 0, 0]], np.int32)
    seq_n = np.array([8, 3], np.int32)
    want = ref_commit_finish(args["tok"], args["lp_tok"], args["n_acc"], args["drawn"], args["lp_drawn"], np.array([2, 2], np.int32),
                             out, np.full((2, T), SENT_LP, np.float32), np.zeros(2, np.int32), 0, np.full(2, SENT_MATCH, np.int32),
                             seq_tok, seq_n, None, None, 0, T)
    assert want[3].tolist() == [3, 1] and want[4].tolist() == [0, STOP] and want[6].tolist() == [SENT_MATCH, 1]
    seq_len, o, lp, fin, mt = dev(np.array([2, 2], np.int32)), dev(out), dev(np.full((2, T), SENT_LP, np.float32)), \
        dev(np.zeros(2, np.int32)), dev(np.full(2, SENT_MATCH, np.int32))
    nc, nf = dev(np.full(2, SENT_NC, np.int32)), dev(np.zeros(1, np.int32))
    Kn.commit_step_finish(dev(args["tok"]), dev(args["lp_tok"]), dev(args["n_acc"]), dev(args["drawn"]), dev(args["lp_drawn"]),
                          seq_len, o, lp, fin, 0, seq_tok=dev(seq_tok), seq_n=dev(seq_n), n_finished=nf, matched=mt, n_commit=nc,
                          max_len=T)
    torch.cuda.synchronize()
    _assert_equal((seq_len, o, lp, nc, fin, nf, mt), want)


def test_a_match_straddles_launches():
    """Three chained steps on one set of buffers: an 8-token sequence begins in the tokens step 1 commits, runs through all of
    step 2's and ends inside step 3's accepted prefix; a second row's 2-token sequence is split between steps 1 and 2."""
    import torch
    from asd_amd import kernels as Kn
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()            # noqa: E731
    B, K, T = 3, 4, 40
    rng = np.random.default_rng(7)
    steps = []
    for _ in range(3):
        steps.append(dict(tok=rng.integers(100, 151000, (B, K)).astype(np.int32), lp_tok=(-rng.uniform(0, 9, (B, K))).astype(np.float32),
                          n_acc=np.array([2, 4, 1], np.int32), drawn=rng.integers(100, 151000, B).astype(np.int32),
                          lp_drawn=(-rng.uniform(0, 9, B)).astype(np.float32)))
    row0 = [int(t) for s in steps for t in list(s["tok"][0, :2]) + [int(s["drawn"][0])]]          # 3 tokens per step
    row1 = [int(t) for s in steps for t in list(s["tok"][1, :4]) + [int(s["drawn"][1])]]          # 5 per step
    seqs = [row0[0:8], [row1[4], row1[5]]]             # row 0: ends at step 3's candidate 1; row 1: drawn of step 1 + first of step 2
    seq_tok = np.array([s + [0] * (8 - len(s)) for s in seqs], np.int32)
    seq_n = np.array([8, 2], np.int32)
    row_first = np.array([0, 1, 2, 2], np.int32)
    out = np.full((B, T), SENT_TOK, np.int32)
    out[:, :START] = rng.integers(100, 151000, (B, START))
    ref = (np.full(B, START, np.int32), out, np.full((B, T), SENT_LP, np.float32), None, np.zeros(B, np.int32), 0,
           np.full(B, SENT_MATCH, np.int32))
    d = [dev(ref[0]), dev(ref[1]), dev(ref[2]), dev(ref[4]), dev(ref[6])]
    nf, nc = dev(np.zeros(1, np.int32)), dev(np.full(B, SENT_NC, np.int32))
    d_seq_tok, d_seq_n, d_first = dev(seq_tok), dev(seq_n), dev(row_first)
    for s in steps:
        ref = ref_commit_finish(s["tok"], s["lp_tok"], s["n_acc"], s["drawn"], s["lp_drawn"], ref[0], ref[1], ref[2], ref[4], ref[5],
                                ref[6], seq_tok, seq_n, row_first, None, START, T)
        Kn.commit_step_finish(dev(s["tok"]), dev(s["lp_tok"]), dev(s["n_acc"]), dev(s["drawn"]), dev(s["lp_drawn"]), d[0], d[1], d[2],
                              d[3], START, seq_tok=d_seq_tok, seq_n=d_seq_n, row_first=d_first, n_finished=nf, matched=d[4],
                              n_commit=nc, max_len=T)
        torch.cuda.synchronize()
        _assert_equal((d[0], d[1], d[2], nc, d[3], nf, d[4]), ref)
    assert ref[4].tolist() == [STOP, STOP, 0] and ref[0].tolist() == [START + 8, START + 6, START + 6] and ref[5] == 2
    assert ref[6].tolist() == [0, 0, SENT_MATCH]


@pytest.mark.parametrize("B,K", [(33, 8), (5, 64), (7, 0)])
def test_with_sequences_of_length_one_it_is_commit_step_stop(B, K):
    """Random inputs over a vocabulary of 40 ids, so stop ids are hit everywhere: every output has asd_commit_step_stop's bytes."""
    import torch
    from asd_amd import kernels as Kn
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()            # noqa: E731
    rng = np.random.default_rng(B * 100 + K)
    T = K + 12
    max_len = T - 2
    for n_stop in (0, 1, 8):
        stops = rng.choice(40, n_stop, replace=False).astype(np.int32)
        tok = rng.integers(0, 40, (B, K)).astype(np.int32)
        lp_tok = (-rng.uniform(0, 20, (B, K))).astype(np.float32)
        drawn, lp_drawn = rng.integers(0, 40, B).astype(np.int32), (-rng.uniform(0, 20, B)).astype(np.float32)
        n_acc = rng.integers(-1, K + 2, B).astype(np.int32)
        seq_len = rng.integers(2, 12, B).astype(np.int32)
        finished = (rng.integers(0, 6, B) // 4 * rng.integers(1, 3, B)).astype(np.int32)
        hist = rng.integers(0, 40, (B, T)).astype(np.int32)
        outs = []
        for finish in (False, True):
            d_len, d_fin = dev(seq_len.copy()), dev(finished.copy())
            d_tok, d_lp = dev(hist.copy()), dev(np.full((B, T), SENT_LP, np.float32))
            nc, nf = dev(np.full(B, SENT_NC, np.int32)), dev(np.full(1, N_FINISHED_0, np.int32))
            args = (dev(tok) if K else None, dev(lp_tok) if K else None, dev(n_acc), dev(drawn), dev(lp_drawn), d_len, d_tok, d_lp, d_fin)
            if finish:
                seq_tok = np.full((n_stop, 8), SENT_TOK, np.int32)
                seq_tok[:, 0] = stops
                Kn.commit_step_finish(*args, int(rng.integers(0, 3)), seq_tok=dev(seq_tok) if n_stop else None,
                                      seq_n=dev(np.ones(n_stop, np.int32)) if n_stop else None, n_finished=nf, n_commit=nc,
                                      max_len=max_len)
            else:
                Kn.commit_step_stop(*args, stop_ids=dev(stops) if n_stop else None, n_finished=nf, n_commit=nc, max_len=max_len)
            torch.cuda.synchronize()
            outs.append([t.cpu().numpy().tobytes() for t in (d_tok, d_lp, d_len, nc, d_fin, nf)])
        assert outs[0] == outs[1], n_stop
        want = ref_commit_stop(tok if K else None, lp_tok if K else None, n_acc, drawn, lp_drawn, seq_len, hist,
                               np.full((B, T), SENT_LP, np.float32), finished, N_FINISHED_0, stops, max_len)
        assert outs[1][2] == want[0].tobytes() and outs[1][4] == want[4].tobytes()
        if n_stop == 8:
            assert (want[4] == STOP).sum() > (finished == STOP).sum()


def test_python_side_argument_checks():
    import torch
    from asd_amd import kernels as Kn
    z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device="cuda")     # noqa: E731
    B, K, T = 4, 8, 32
    a = (z(B, K), z(B, K, dt=torch.float32), z(B), z(B), z(B, dt=torch.float32), z(B), z(B, T), z(B, T, dt=torch.float32), z(B))
    seq_tok, seq_n = z(3, 8) + 200000, z(3) + 1
    Kn.commit_step_finish(*a, 0, seq_tok=seq_tok, seq_n=seq_n)                  # valid
    for kw in (dict(seq_tok=seq_tok), dict(seq_tok=z(3, 7), seq_n=seq_n), dict(seq_tok=seq_tok, seq_n=z(2)),
               dict(seq_tok=z(17, 8), seq_n=z(17)), dict(seq_tok=seq_tok, seq_n=seq_n, row_first=z(B)),
               dict(seq_tok=seq_tok, seq_n=seq_n, row_max_len=z(B + 1)), dict(seq_tok=seq_tok, seq_n=seq_n, matched=z(B + 1)),
               dict(seq_tok=seq_tok.to(torch.int64), seq_n=seq_n), dict(seq_tok=seq_tok, seq_n=seq_n, n_finished=z(2))):
        with pytest.raises(ValueError):
            Kn.commit_step_finish(*a, 0, **kw)
    with pytest.raises(ValueError):
        Kn.commit_step_finish(*a, -1, seq_tok=seq_tok, seq_n=seq_n)
    Kn.commit_step_finish(*a, 0, seq_tok=z(17, 8), seq_n=z(17), row_first=z(B + 1))     # with row_first the total may exceed 16
    torch.cuda.synchronize()
