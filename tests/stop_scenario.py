"""Shared by tests/test_stop_tokens.py (CPU, oracle ops twin), tests/test_gpu_stop_tokens.py (HipOps) and
tests/test_gpu_commit_stop.py (the kernel): the numpy reference of asd_commit_step_stop, written from the header's text and not
from the kernel, the ops twin that commits through it, and the helpers of the prefix-property tests.

TEST INFRASTRUCTURE, like tests/stage_scenario.py: never importable from the package."""
import numpy as np
import torch

from tests.stage_scenario import MAX_TOKENS, PROMPTS, TEMPERATURE, StageOracleOps, text_ids

STOP, LENGTH = 1, 2


def ref_commit_stop(tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, tokens, lps, finished, n_finished, stop_ids, max_len):
    """asd_commit_step_stop on numpy arrays -> (seq_len, tokens, lps, n_commit, finished, n_finished); bits are copied.
    One row at a time, over the list of candidates: no mask, no lanes."""
    seq_len, tokens, lps, finished = seq_len.copy(), tokens.copy(), lps.copy(), finished.copy()
    stops = set() if stop_ids is None else {int(s) for s in stop_ids}
    B = drawn.shape[0]
    K = 0 if tok is None else tok.shape[1]
    n_commit = np.full(B, -1, np.int32)
    n_finished = int(n_finished)
    for b in range(B):
        if finished[b] != 0:
            n_commit[b] = 0
            continue
        na = min(max(int(n_acc[b]), 0), K)
        length = int(seq_len[b])
        cand = [(tok[b, k], lp_tok[b, k]) for k in range(na)] + [(drawn[b], lp_drawn[b])]
        cand = cand[:max(max_len - length, 0)]                # what max_len cuts off is neither written nor a stop
        hit = next((j for j, (t, _) in enumerate(cand) if int(t) in stops), None)
        if hit is not None:
            cand = cand[:hit + 1]                              # the stop token itself is committed
        for i, (t, lp) in enumerate(cand):
            tokens[b, length + i] = t
            lps[b, length + i] = lp
        n_commit[b] = len(cand)
        seq_len[b] = length + len(cand)
        finished[b] = STOP if hit is not None else (LENGTH if seq_len[b] >= max_len else 0)
        n_finished += int(finished[b] != 0)
    return seq_len, tokens, lps, n_commit, finished, np.int32(n_finished)


class StopOracleOps(StageOracleOps):
    """StageOracleOps + commit_step_stop on the reference above."""

    def commit_step_stop(self, tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, tokens, lps, n_commit, max_len, stop_ids, finished,
                         n_finished):
        self.calls["commit_step_stop"] += 1
        ln, tk, lp, nc, fin, nf = ref_commit_stop(None if tok is None else tok.numpy(), None if lp_tok is None else lp_tok.numpy(),
                                                  n_acc.numpy(), drawn.numpy(), lp_drawn.numpy(), seq_len.numpy(), tokens.numpy(),
                                                  lps.numpy(), finished.numpy(), n_finished.numpy()[0], stop_ids.numpy(), max_len)
        seq_len.copy_(torch.from_numpy(ln))
        tokens.copy_(torch.from_numpy(tk))
        lps.copy_(torch.from_numpy(lp))
        n_commit.copy_(torch.from_numpy(nc))
        finished.copy_(torch.from_numpy(fin))
        n_finished.fill_(int(nf))


# ------------------------------------------------------------------------------------------ the prefix property
def free_run(stage, prompts=PROMPTS, max_tokens=MAX_TOKENS):
    """A run without a stop set that keeps its step inputs -> dict(tokens [B][max_tokens], lps, kinds, stats); kinds[b][i] says how
    token i of row b was committed: "accepted" (a draft token the verify let through) or "drawn" (the commit draw, or stage 0's)."""
    stage.keep_inputs = True
    try:
        texts, lps, stats = stage.generate(prompts=prompts, max_tokens=max_tokens, temperature=TEMPERATURE, stop_token_ids=())
    finally:
        stage.keep_inputs = False
    B = len(prompts)
    kinds = [[] for _ in range(B)]
    for s in stage.step_inputs:
        if "tok" in s:
            K = s["tok"].shape[1]
            na = np.clip(s["n_acc"].cpu().numpy(), 0, K)
        else:
            na = np.zeros(B, np.int64)
        for b in range(B):
            kinds[b] += ["accepted"] * int(na[b]) + ["drawn"]
    tokens = [text_ids(t) for t in texts]
    assert all(len(t) == max_tokens == len(lp) for t, lp in zip(tokens, lps))
    return dict(tokens=tokens, lps=lps, kinds=[k[:max_tokens] for k in kinds], stats=stats)


def expected_with_stops(free, ids):
    """Per row of a free run: (n tokens kept, "stop" | "length", how the stopping token was committed or None)."""
    out = []
    for toks, kinds in zip(free["tokens"], free["kinds"]):
        hit = next((i for i, t in enumerate(toks) if t in ids), None)
        out.append((len(toks), "length", None) if hit is None else (hit + 1, "stop", "first" if hit == 0 else kinds[hit]))
    return out


def pick_stop_ids(free, max_ids=8):
    """Stop ids from the free run's own output, chosen so that -- where the run offers them -- one row ends on its first token,
    one on an accepted draft token, one on a drawn token (both behind the first position) and one row does not end at all."""
    rows = range(len(free["tokens"]))
    best, best_score = [], -1
    for spare in rows:                                        # the row that must not stop
        ids, got = [], set()
        for want in ("first", "accepted", "drawn"):
            for r in rows:
                done = False
                for i, t in enumerate(free["tokens"][r]):
                    if r == spare or len(ids) >= max_ids or t in ids:
                        continue
                    exp = expected_with_stops(free, ids + [t])
                    before = expected_with_stops(free, ids)
                    keeps = all(e == o for k, (e, o) in enumerate(zip(exp, before)) if k != r and o[1] == "stop")
                    if exp[spare][1] == "length" and keeps and exp[r] == (i + 1, "stop", want) and before[r][1] == "length":
                        ids.append(t)
                        got.add(want)
                        done = True
                        break
                if done:
                    break
        if len(got) > best_score:
            best, best_score = ids, len(got)
    return best


def assert_prefix_property(free, ids, texts, lps, stats):
    """The run with the stop set `ids` returned every row of the free run up to and including its first stop id."""
    want = expected_with_stops(free, ids)
    for b, (n, reason, _) in enumerate(want):
        assert text_ids(texts[b]) == free["tokens"][b][:n], (b, n)
        assert lps[b].dtype == np.float32 and lps[b].tobytes() == free["lps"][b][:n].tobytes(), (b, n)
        assert len(texts[b].split()) == len(lps[b]) == n
    assert stats["n_tokens"] == [w[0] for w in want] and stats["finish_reasons"] == [w[1] for w in want]
    return want
