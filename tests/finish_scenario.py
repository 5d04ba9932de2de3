"""Shared by tests/test_finish.py (CPU, oracle ops twin), tests/test_gpu_finish_stages.py (HipOps) and
tests/test_gpu_commit_finish.py (the kernel): the numpy reference of asd_commit_step_finish, written from the header's text and
not from the kernel, the ops twin that commits through it, and the helpers that pick stop sequences out of a free run.

TEST INFRASTRUCTURE, like tests/stop_scenario.py: never importable from the package."""
import numpy as np
import torch

from tests.stage_scenario import MAX_TOKENS, PROMPTS, TEMPERATURE, text_ids
from tests.stop_scenario import LENGTH, STOP, StopOracleOps

MAX_STOP_SEQS, MAX_STOP_SEQ_LEN = 16, 8              # ASD_MAX_STOP_SEQS, ASD_MAX_STOP_SEQ_LEN of include/asd_hip.h


def ref_commit_finish(tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, tokens, lps, finished, n_finished, matched, seq_tok, seq_n,
                      row_first, row_max_len, start, max_len):
    """asd_commit_step_finish on numpy arrays -> (seq_len, tokens, lps, n_commit, finished, n_finished, matched); bits are
    copied.  One row at a time, over the list of candidates: no window, no lanes.  matched may be None."""
    seq_len, tokens, lps, finished = seq_len.copy(), tokens.copy(), lps.copy(), finished.copy()
    matched = None if matched is None else matched.copy()
    B = drawn.shape[0]
    K = 0 if tok is None else tok.shape[1]
    n_seq = 0 if seq_tok is None else seq_tok.shape[0]
    n_commit = np.full(B, -1, np.int32)
    n_finished = int(n_finished)
    for b in range(B):
        if finished[b] != 0:
            n_commit[b] = 0
            continue
        limit = int(max_len) if row_max_len is None else min(int(max_len), max(int(row_max_len[b]), 0))
        na = min(max(int(n_acc[b]), 0), K)
        length = int(seq_len[b])
        cand = [(tok[b, k], lp_tok[b, k]) for k in range(na)] + [(drawn[b], lp_drawn[b])]
        cand = cand[:min(na + 1, max(limit - length, 0))]    # fit: what the limit cuts off is neither written nor matched
        owned = range(n_seq) if row_first is None else range(int(row_first[b]), int(row_first[b + 1]))
        owned = [s for s in owned if 0 <= s < n_seq][:MAX_STOP_SEQS]
        stream = [int(t) for t in tokens[b, :length]] + [int(t) for t, _ in cand]
        hit = which = None
        for j in range(len(cand)):
            for idx, s in enumerate(owned):
                m = int(seq_n[s])
                if not 1 <= m <= MAX_STOP_SEQ_LEN:
                    continue
                begin = length + j - m + 1
                if begin >= start and stream[begin:length + j + 1] == [int(t) for t in seq_tok[s, :m]]:
                    hit, which = j, idx
                    break
            if hit is not None:
                break
        if hit is not None:
            cand = cand[:hit + 1]                            # the matched tokens are committed
        for i, (t, lp) in enumerate(cand):
            tokens[b, length + i] = t
            lps[b, length + i] = lp
        n_commit[b] = len(cand)
        seq_len[b] = length + len(cand)
        finished[b] = STOP if hit is not None else (LENGTH if seq_len[b] >= limit else 0)
        n_finished += int(finished[b] != 0)
        if hit is not None and matched is not None:
            matched[b] = which
    return seq_len, tokens, lps, n_commit, finished, np.int32(n_finished), matched


class FinishOracleOps(StopOracleOps):
    """StopOracleOps + commit_step_finish on the reference above."""

    def commit_step_finish(self, tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, tokens, lps, n_commit, max_len, start, seq_tok, seq_n,
                           row_first, row_max_len, finished, n_finished, matched):
        self.calls["commit_step_finish"] += 1
        np_ = lambda t: None if t is None else t.numpy()
        ln, tk, lp, nc, fin, nf, mt = ref_commit_finish(np_(tok), np_(lp_tok), n_acc.numpy(), drawn.numpy(), lp_drawn.numpy(),
                                                        seq_len.numpy(), tokens.numpy(), lps.numpy(), finished.numpy(),
                                                        n_finished.numpy()[0], np_(matched), np_(seq_tok), np_(seq_n),
                                                        np_(row_first), np_(row_max_len), start, max_len)
        seq_len.copy_(torch.from_numpy(ln))
        tokens.copy_(torch.from_numpy(tk))
        lps.copy_(torch.from_numpy(lp))
        n_commit.copy_(torch.from_numpy(nc))
        finished.copy_(torch.from_numpy(fin))
        n_finished.fill_(int(nf))
        if matched is not None:
            matched.copy_(torch.from_numpy(mt))


# ------------------------------------------------------------------------------------------ the prefix property
KINDS = ("accepted", "drawn", "straddle")


def step_of(kinds):
    """Per token of a free run's row: the index of the step that committed it (a step ends behind its drawn token)."""
    out, step = [], 0
    for k in kinds:
        out.append(step)
        step += k == "drawn"
    return out


def match_kind(kinds, i, m):
    """How a sequence of m >= 2 tokens that ends at generated token i was committed: "straddle" (it begins in an earlier step),
    "accepted" (one step, ends on an accepted draft token) or "drawn" (one step, ends on its drawn token: n_acc >= 1)."""
    steps = step_of(kinds)
    if steps[i - m + 1] != steps[i]:
        return "straddle"
    return kinds[i]


def expected_with_sequences(free, row_seqs, limits=None):
    """Per row of a free run: (n tokens kept, "stop" | "length", the sequence that ended it or None, its match kind or None):
    the row up to and including the first position at which one of ITS sequences is complete in the generated tokens, or up
    to its limit.  Among sequences ending together the first of the row's list counts."""
    out = []
    for b, (toks, kinds) in enumerate(zip(free["tokens"], free["kinds"])):
        limit = len(toks) if limits is None else min(len(toks), limits[b])
        got = None
        for i in range(limit):
            for s in row_seqs[b]:
                m = len(s)
                if i - m + 1 >= 0 and tuple(toks[i - m + 1:i + 1]) == tuple(s):
                    got = (i + 1, "stop", tuple(s), match_kind(kinds, i, m) if m >= 2 else kinds[i])
                    break
            if got:
                break
        out.append(got or (limit, "length", None, None))
    return out


def pick_stop_sequences(free, max_seqs=8, lengths=(2, 3)):
    """Stop sequences of 2-3 tokens from the free run's own output, common to every row, chosen so that -- where the run offers
    them -- one row ends on a match of each of KINDS and one row does not end at all."""
    rows = range(len(free["tokens"]))
    best, best_score = [], -1
    for spare in rows:                                        # the row that must not stop
        seqs, got = [], set()
        for want in KINDS:
            done = False
            for r in rows:
                if r == spare:
                    continue
                toks = free["tokens"][r]
                for i in range(len(toks)):
                    for m in lengths:
                        if i - m + 1 < 0 or len(seqs) >= max_seqs:
                            continue
                        s = tuple(toks[i - m + 1:i + 1])
                        if s in seqs:
                            continue
                        before = expected_with_sequences(free, [seqs] * len(rows))
                        after = expected_with_sequences(free, [seqs + [s]] * len(rows))
                        keeps = all(a == o for k, (a, o) in enumerate(zip(after, before)) if k != r)
                        if keeps and before[r][1] == "length" and after[r] == (i + 1, "stop", s, want):
                            seqs.append(s)
                            got.add(want)
                            done = True
                            break
                    if done:
                        break
                if done:
                    break
        if len(got) > best_score:
            best, best_score = seqs, len(got)
    return best


def assert_finish_prefix(free, row_seqs, texts, lps, stats, limits=None):
    """The run returned every row of the free run up to and including its first match (or up to its limit), said why it ended
    and which sequence ended it."""
    want = expected_with_sequences(free, row_seqs, limits)
    for b, (n, reason, seq, _) in enumerate(want):
        assert text_ids(texts[b]) == free["tokens"][b][:n], (b, n)
        assert lps[b].dtype == np.float32 and lps[b].tobytes() == free["lps"][b][:n].tobytes(), (b, n)
        assert len(texts[b].split()) == len(lps[b]) == n
    assert stats["n_tokens"] == [w[0] for w in want] and stats["finish_reasons"] == [w[1] for w in want]
    assert [None if m is None else tuple(m) for m in stats["stop_matches"]] == [w[2] for w in want]
    return want


# ------------------------------------------------------------------------------------------ combined with the other arguments
SEEDS = [7, 2 ** 63 + 1, 9, 10, 11]
COMBINED_LIMITS = [12, 12, 3, 12, 9]


def check_combined(stage):
    """logprobs=3 + one seed per prompt + a stop list per prompt + a limit per prompt: the seeded free run cut per row, with the
    top-N tables and the log-probs ragged alike -> stats of the cut run."""
    B = len(PROMPTS)
    kw = dict(prompts=PROMPTS, temperature=TEMPERATURE, seed=SEEDS, logprobs=3)
    base = stage.generate(max_tokens=MAX_TOKENS, **kw)
    fr = dict(tokens=[text_ids(t) for t in base[0]], lps=base[1], kinds=[["drawn"] * MAX_TOKENS] * B)
    rows = [[tuple(fr["tokens"][b][4:6])] if b % 2 else [] for b in range(B)]
    texts, lps, stats = stage.generate(max_tokens=COMBINED_LIMITS, stop_sequences_per_prompt=rows, **kw)
    want = expected_with_sequences(fr, rows, COMBINED_LIMITS)
    assert "stop" in stats["finish_reasons"] and "length" in stats["finish_reasons"]
    for b, (n, reason, seq, _) in enumerate(want):
        assert text_ids(texts[b]) == fr["tokens"][b][:n] and lps[b].tobytes() == base[1][b][:n].tobytes()
        assert stats["top_token_ids"][b].shape == (n, 3) and stats["top_logprobs"][b].shape == (n, 3)
        assert stats["top_token_ids"][b].tobytes() == base[2]["top_token_ids"][b][:n].tobytes()
        assert stats["top_logprobs"][b].tobytes() == base[2]["top_logprobs"][b][:n].tobytes()
        assert stats["finish_reasons"][b] == reason and stats["stop_matches"][b] == seq
    return stats


def check_greedy(stage, limits):
    """Temperature 0: the greedy free run (step inputs kept, so the match kinds are known), then the run with sequences picked
    from it and per-row limits -> what every row was expected to do."""
    B = len(PROMPTS)
    stage.keep_inputs = True
    try:
        base = stage.generate(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0)
    finally:
        stage.keep_inputs = False
    kinds = [[] for _ in range(B)]
    for s in stage.step_inputs:
        K = 0 if s["tok"] is None else s["tok"].shape[1]
        na = np.clip(s["n_acc"].cpu().numpy(), 0, K)
        for b in range(B):
            kinds[b] += ["accepted"] * int(na[b]) + ["drawn"]
    fr = dict(tokens=[text_ids(t) for t in base[0]], lps=base[1], kinds=[k[:MAX_TOKENS] for k in kinds])
    seqs = pick_stop_sequences(fr)
    assert seqs
    texts, lps, stats = stage.generate(prompts=PROMPTS, max_tokens=limits, temperature=0.0, stop_sequences=[list(s) for s in seqs])
    want = assert_finish_prefix(fr, [seqs] * B, texts, lps, stats, limits)
    assert "stop" in [w[1] for w in want]
    return want
