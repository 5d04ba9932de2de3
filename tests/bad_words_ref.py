"""Multi-token bad words (serving/stages.py, BAD WORDS; include/asd_hip.h, asd_bad_words_rows): the numpy reference of the
kernel, written from the header's text, the oracle ops twin that bans through it, the recorder of the call order, and the
stage-level scenarios that tests/test_bad_words_stages.py (CPU twin) and tests/test_gpu_bad_words_stages.py (HipOps) both run.

TEST INFRASTRUCTURE, like tests/penalty_ref.py: never importable from the package."""
from types import SimpleNamespace

import numpy as np
import torch

from tests.logit_edit_ref import SEEDS, run_kept
from tests.penalty_ref import PenaltyOracleOps
from tests.stage_scenario import MAX_TOKENS, PROMPTS, TEMPERATURE, text_ids
from tests.token_mask_ref import allow_list
from tests.top_logprobs_ref import PAIR_ATOL

MAX_WORDS = 256                                  # ASD_MAX_BAD_WORDS
MAX_WORD_LEN = 8                                 # ASD_MAX_BAD_WORD_LEN


def ref_bad_words(x, words_per_row, tokens, seq_len, start, max_len, step_tok=None, n_prev=0):
    """asd_bad_words_rows on a CPU tensor, IN PLACE (-> x): x [B, V] or [B, K1, V] (any strides); words_per_row: one list of
    words (sequences of ids) per sequence; tokens int [B, >= max_len]; seq_len: B ints; step_tok int [B, n_tok] or None.
    Position j of sequence b has H = tokens[b][start : clamp(seq_len[b], start, max_len)] ++ step_tok[b][: n_prev + j]; the last
    id of a word of m ids becomes -inf when len(H) >= m - 1 and H ends in the word's first m - 1 ids.  A word whose length is
    outside 1..8 or whose last id is outside [0, V) is skipped; only the first 256 words of a sequence are honoured."""
    view = x[:, None] if x.dim() == 2 else x
    Bv, K1, V = view.shape
    tokens = np.asarray(tokens)
    assert len(words_per_row) == Bv and (n_prev == 0 or step_tok is not None) and 0 <= start <= max_len <= tokens.shape[1]
    for b in range(Bv):
        L = min(max(int(seq_len[b]), start), max_len)
        committed = [int(t) for t in tokens[b, start:L]]
        for j in range(K1):
            seen = [] if step_tok is None else [int(t) for t in np.asarray(step_tok)[b, :n_prev + j]]
            assert len(seen) == (0 if step_tok is None else n_prev + j)
            H = committed + seen
            for w in list(words_per_row[b])[:MAX_WORDS]:
                w = [int(t) for t in w]
                m = len(w)
                if not 1 <= m <= MAX_WORD_LEN or not 0 <= w[-1] < V:
                    continue
                if len(H) >= m - 1 and H[len(H) - (m - 1):] == w[:-1]:
                    view[b, j, w[-1]] = float("-inf")                              # a view: the assignment lands in x
    return x


class BadWordsOracleOps(PenaltyOracleOps):
    """PenaltyOracleOps + pack_bad_words and bad_words_rows on the reference above: the tiny stages run without a GPU."""

    def pack_bad_words(self, rows, device):
        self._note("pack_bad_words", ())
        rows = [[tuple(int(t) for t in w) for w in r] for r in rows]
        assert all(len(set(r)) == len(r) <= MAX_WORDS and all(1 <= len(w) <= MAX_WORD_LEN for w in r) for r in rows)   # what the stage hands over
        return SimpleNamespace(rows=rows, B=len(rows))

    def bad_words_rows(self, logits, words, tokens, seq_len, start, max_len, step_tok=None, n_prev=0):
        self._note("bad_words_rows", ())
        assert words.B == logits.shape[0]
        return ref_bad_words(logits, words.rows, tokens.numpy(), seq_len.tolist(), start, max_len,
                             None if step_tok is None else step_tok.numpy(), n_prev)


class CallOrder:
    """Stands between a stage and the named ops of `ops` (instance attributes: the ops object stays what it is) and notes the
    order of their calls; works on the twin and on HipOps alike."""
    NAMES = ("pack_bad_words", "bad_words_rows", "logit_mask_rows", "logit_edit_rows", "penalty_rows")

    def __init__(self, ops):
        self.ops, self.names = ops, []
        for name in self.NAMES:
            def wrapped(*a, _orig=getattr(ops, name), _name=name, **kw):
                self.names.append(_name)
                return _orig(*a, **kw)
            setattr(ops, name, wrapped)

    def close(self):
        for name in self.NAMES:
            delattr(self.ops, name)


# ------------------------------------------------------------------------------------------ helpers
def holds(gen, word):
    """Does the list `gen` hold `word` as a contiguous run?"""
    m = len(word)
    return any(tuple(gen[i:i + m]) == tuple(word) for i in range(len(gen) - m + 1))


def banned_at(prefix, words):
    """The ids a row's words ban at the position behind the generated tokens `prefix`."""
    return {w[-1] for w in words if len(prefix) >= len(w) - 1 and tuple(prefix[len(prefix) - (len(w) - 1):]) == tuple(w[:-1])}


def fresh_bigram(t):
    """The last i at which the bigram (t[i], t[i + 1]) occurs for the first time in t (i = 0 always qualifies)."""
    return max(i for i in range(len(t) - 1) if not holds(t[:i + 1], t[i:i + 2]))


def _cpu(s):
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in s.items()}


def check_no_word(texts, rows):
    for b, (t, words) in enumerate(zip(texts, rows)):
        gen = text_ids(t)
        for w in words:
            assert not holds(gen, w), (b, w, gen)


# ------------------------------------------------------------------------------------------ stage-level scenarios
def scenario_greedy_replay(stage):
    """Scenario 1.  Greedy without bad words; every row bans the bigram at its positions (i, i + 1), the last one that is new
    to the row there: the tokens before i + 1 stay, token i + 1 changes, no row holds its word.  Then the first run's first 8
    tokens as an 8-token word; then all of them and the second run's new bigram in one list."""
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0)
    old = [text_ids(t) for t in stage.generate(**kw)[0]]
    at = [fresh_bigram(t) for t in old]
    words = [[tuple(t[i:i + 2])] for t, i in zip(old, at)]
    texts, lps, _ = stage.generate(bad_words_per_prompt=words, **kw)
    new = [text_ids(t) for t in texts]
    for b, i in enumerate(at):
        assert new[b][:i + 1] == old[b][:i + 1] and new[b][i + 1] != old[b][i + 1], (b, i, old[b], new[b])
        assert np.isfinite(lps[b]).all()
    check_no_word(texts, words)
    # the 8-token word alone: its 7-token prefix is generated again, so token 7 changes and nothing in front of it does
    long = [[tuple(o[:8])] for o in old]
    texts, lps, _ = stage.generate(bad_words_per_prompt=long, **kw)
    for b, t in enumerate(map(text_ids, texts)):
        assert t[:7] == old[b][:7] and t[7] != old[b][7], (b, old[b], t)
        assert np.isfinite(lps[b]).all()
    check_no_word(texts, long)
    # all of them in one list, with the bigram the second run put in the banned one's place (it may occur earlier in the row:
    # the row then leaves the first run at the first position at which one of its words bans the first run's token)
    words = [w + [tuple(t[i:i + 2])] + l for w, t, l, i in zip(words, new, long, at)]
    texts, lps, _ = stage.generate(bad_words_per_prompt=words, **kw)
    for b, t in enumerate(map(text_ids, texts)):
        p = next(p for p in range(MAX_TOKENS) if old[b][p] in banned_at(old[b][:p], words[b]))
        assert p <= 7 and t[:p] == old[b][:p] and t[p] != old[b][p], (b, p, old[b], t)
        assert np.isfinite(lps[b]).all()
    check_no_word(texts, words)
    return texts


def sampled_words(base):
    """A one-token word, a bigram and a trigram per row, from the tokens of the unbanned run: even rows begin with the bigram,
    odd rows with the trigram, so that both are live while a row still follows the unbanned run."""
    rows = []
    for b, t in enumerate(base):
        two, three = (t[0:2], t[3:6]) if b % 2 == 0 else (t[5:7], t[0:3])
        rows.append([(t[-1],), tuple(two), tuple(three)])
    return rows


def check_kept_bans(stage, texts, rows, prompts):
    """Every kept step of a call WITHOUT mask or edit: the logits are -inf exactly where ref_bad_words puts it on a replay from
    the recorded seq_len and proposals (the target's K + 1 positions at a verifying stage), and no proposal completes a word.
    -> the number of (row, position) pairs at which a bigram, and a trigram, matched."""
    V = stage.shape.vocab
    P = stage.encode_prompts(prompts).shape[1]
    B = len(prompts)
    gen = [text_ids(t) for t in texts]
    cap = P + max(len(g) for g in gen)
    tokens = np.zeros((B, cap), dtype=np.int32)
    for b, g in enumerate(gen):
        tokens[b, P:P + len(g)] = g
    hits = {2: 0, 3: 0}
    assert stage.step_inputs
    for step, s in enumerate(map(_cpu, stage.step_inputs)):
        if "tok" in s:
            got = torch.cat([s["logits"], s["bonus"][:, None]], 1)                  # [B, K + 1, V]
            seq_len, tok = s["seq_len"].tolist(), s["tok"].numpy()
        else:
            got, seq_len, tok = s["logits"], [P + step] * B, None                   # stage 0 without a stop set: one token per step
        want = ref_bad_words(torch.zeros(got.shape), rows, tokens, seq_len, P, cap, tok, 0)
        assert torch.equal(torch.isneginf(got), torch.isneginf(want)), step
        for b in range(B):
            n = seq_len[b] - P
            for j in range(0 if tok is None else tok.shape[1] + 1):
                H = gen[b][:n] + tok[b, :j].tolist()
                if j < tok.shape[1]:
                    assert int(tok[b, j]) not in banned_at(H, rows[b]), (step, b, j)   # the DRAFT side was banned too
                for w in rows[b]:
                    hits[len(w)] = hits.get(len(w), 0) + (len(w) > 1 and w[-1] in banned_at(H, [w]))
            if tok is None:
                for w in rows[b]:
                    hits[len(w)] = hits.get(len(w), 0) + (len(w) > 1 and w[-1] in banned_at(gen[b][:n], [w]))
    return hits[2], hits[3]


def scenario_sampled(stage):
    """Scenario 2.  Seeded and sampled: no row holds one of its words; the call repeated is bit-equal; every kept step's -inf
    pattern is the reference's (check_kept_bans)."""
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS)
    base = [text_ids(t) for t in stage.generate(**kw)[0]]
    rows = sampled_words(base)
    texts, lps, _ = run_kept(stage, bad_words_per_prompt=rows, **kw)
    check_no_word(texts, rows)
    assert all(np.isfinite(lp).all() for lp in lps)
    two, three = check_kept_bans(stage, texts, rows, PROMPTS)
    assert two > 0 and three > 0, (two, three)                                       # both multi-token lengths were live
    again, lps2, _ = stage.generate(bad_words_per_prompt=rows, **kw)
    assert again == texts and all(a.tobytes() == b.tobytes() for a, b in zip(lps, lps2))
    return texts


EQUAL_PROMPTS = ["one two three", "four five six", "seven eight nine", "ten eleven twelve", "red green blue"]


def scenario_rows_independent(stage):
    """Scenario 3.  Seeded, equal-length prompts, one list per prompt (row 1: none): row b is bit-equal, in text and log-prob
    bytes, to row b of the call that gives EVERY row b's list."""
    assert len({len(stage.tokenizer.encode(p, return_tensors=None)) for p in EQUAL_PROMPTS}) == 1
    kw = dict(prompts=EQUAL_PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS)
    base = stage.generate(**kw)
    rows = [[(t[2],), tuple(t[0:2]), tuple(t[4:7])] for t in map(text_ids, base[0])]
    rows[1] = []
    mixed = stage.generate(bad_words_per_prompt=rows, **kw)
    for b, words in enumerate(rows):
        alone = stage.generate(bad_words=words, **kw) if words else base
        assert alone[0][b] == mixed[0][b], b
        assert alone[1][b].tobytes() == mixed[1][b].tobytes(), b
    check_no_word(mixed[0], rows)
    assert mixed[0][1] == base[0][1] and sum(m != t for m, t in zip(mixed[0], base[0])) == 4    # (t[2],) changes every other row
    return mixed


def scenario_composition(stage):
    """Scenario 4.  Greedy, with an allow-list, a bias, penalties, logprobs = 2 and a stop id in one call: no word appears, a
    top-N entry is finite only where the list allows and no word bans, and a committed token's log-prob is its table entry."""
    V = stage.shape.vocab
    allowed = allow_list(V, 40, 4)
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0, allowed_token_ids=allowed, logit_bias={allowed[3]: 1.0},
              repetition_penalty=1.3, frequency_penalty=1.5, logprobs=2)                 # (the penalty keeps greedy rows from looping)
    base = [text_ids(t) for t in stage.generate(**kw)[0]]
    unused = [next(t for t in allowed if t not in g) for g in base]
    rows = [[tuple(g[i:i + 2]), (u,)] for g, u, i in zip(base, unused, (fresh_bigram(g) for g in base))]
    others = {t for g in base[1:] for t in g}
    stop = next((t for t in base[0][1:] if t not in others), base[0][1])            # a token of row 0, of no other row if there is one
    texts, lps, stats = stage.generate(bad_words_per_prompt=rows, stop_token_ids=[stop], **kw)
    check_no_word(texts, rows)
    assert stats["finish_reasons"][0] == "stop"
    assert any(text_ids(t) != g[:len(text_ids(t))] for t, g in zip(texts, base))     # some bigram was live
    for b, t in enumerate(map(text_ids, texts)):
        ids, top = stats["top_token_ids"][b], stats["top_logprobs"][b]
        assert ids.shape == top.shape == (len(t), 2) and np.isfinite(lps[b]).all()
        for i in range(len(t)):
            gone = banned_at(t[:i], rows[b])
            for v, lp in zip(ids[i].tolist(), top[i].tolist()):
                assert not np.isfinite(lp) or (v in allowed and v not in gone), (b, i, v)
            assert ids[i][0] == t[i] and abs(float(lps[b][i]) - float(top[i][0])) <= PAIR_ATOL, (b, i)
    return texts


def scenario_call_trace(stage):
    """Scenario 5.  One pack_bad_words; steps x (1 | draft_len + 1) bad_words_rows calls, each directly in front of the step's
    logit_edit_rows call (and behind the mask's) when an edit is on; none at all with empty lists."""
    kw = dict(prompts=PROMPTS, max_tokens=4, temperature=TEMPERATURE, seed=SEEDS, logit_bias={5: 1.0}, frequency_penalty=0.5,
              allowed_token_ids=list(range(0, stage.shape.vocab, 2)))
    log = CallOrder(stage.ops)
    try:
        stage.generate(bad_words=[(2, 4), (6,)], **kw)
        names = list(log.names)
        steps = stage.last_steps
        del log.names[:]
        for empty in (dict(), dict(bad_words=[]), dict(bad_words=(), bad_words_per_prompt=[[] for _ in PROMPTS]), dict(bad_words=None)):
            stage.generate(**empty, **kw)
        quiet = list(log.names)
    finally:
        log.close()
    per_step = 1 if stage.draft is None else stage.config.draft_len + 1
    assert names.count("pack_bad_words") == 1 and names[0] == "pack_bad_words"
    assert names.count("bad_words_rows") == names.count("logit_edit_rows") == steps * per_step
    for i, n in enumerate(names):
        if n == "bad_words_rows":
            assert (names[i - 1], names[i + 1], names[i + 2]) == ("logit_mask_rows", "logit_edit_rows", "penalty_rows"), names[i - 1:i + 3]
    assert quiet and not [n for n in quiet if "bad_words" in n]
    return names


__all__ = ["BadWordsOracleOps", "CallOrder", "banned_at", "check_kept_bans", "check_no_word", "fresh_bigram", "holds",
           "ref_bad_words", "scenario_call_trace", "scenario_composition", "scenario_greedy_replay", "scenario_rows_independent",
           "scenario_sampled"]
