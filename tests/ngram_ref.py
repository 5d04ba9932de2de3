"""no_repeat_ngram_size (serving/stages.py, NO REPEAT N-GRAM; include/asd_hip.h, asd_no_repeat_ngram_rows): the numpy reference of
the kernel, written from the header's text, the oracle ops twin that bans through it, and the stage-level scenarios that
tests/test_no_repeat_ngram_stages.py (CPU twin) and tests/test_gpu_no_repeat_ngram_stages.py (HipOps) both run on
stage_configs(vocab=64) with 32 tokens per row: at that shape every greedy row of the plain run repeats bigrams and trigrams, and
every scenario asserts so before it looks at the run with the rule on.

TEST INFRASTRUCTURE, like tests/bad_words_ref.py: never importable from the package."""
import zlib
from types import SimpleNamespace

import numpy as np
import torch

from tests.fsm_ref import FsmOracleOps
from tests.logit_edit_ref import SEEDS, run_kept
from tests.stage_scenario import NAMES, PROMPTS, TEMPERATURE, LogprobPredictor, text_ids
from tests.top_logprobs_ref import PAIR_ATOL

MAX_NGRAM = 8                                    # ASD_MAX_NGRAM
VOCAB = 64                                       # the stages of the scenarios: stage_configs(vocab=VOCAB)
NG_MAX_TOKENS = 32


def ref_no_repeat_ngram(x, ns, tokens, seq_len, row_start, start, max_len, step_tok=None, n_prev=0):
    """asd_no_repeat_ngram_rows on a CPU tensor, IN PLACE (-> x): x [B, V] or [B, K1, V] (any strides); ns: one int per sequence,
    or ONE int for every sequence (ngram_n == NULL); tokens int [B, >= max_len]; seq_len: B ints; row_start: B ints, or None
    (`start` for every sequence); step_tok int [B, n_tok] or None.  Position j of sequence b has
        H = tokens[b][clamp(row_start[b], 0, start) : clamp(seq_len[b], start, max_len)] ++ step_tok[b][: n_prev + j]
    and for every i in [0, len(H) - n] with H[i : i+n-1] == H[len(H)-n+1 :] element H[i+n-1] becomes -inf.  A sequence whose n
    is outside 1..8 is skipped; a history token outside [0, V) is compared but never written."""
    view = x[:, None] if x.dim() == 2 else x
    Bv, K1, V = view.shape
    tokens = np.asarray(tokens)
    ns = [int(ns)] * Bv if np.ndim(ns) == 0 else [int(n) for n in ns]
    assert len(ns) == Bv and (n_prev == 0 or step_tok is not None) and 0 <= start <= max_len <= tokens.shape[1]
    for b in range(Bv):
        n = ns[b]
        if not 1 <= n <= MAX_NGRAM:
            continue
        L = min(max(int(seq_len[b]), start), max_len)
        first = start if row_start is None else min(max(int(row_start[b]), 0), start)
        committed = [int(t) for t in tokens[b, first:L]]
        for j in range(K1):
            seen = [] if step_tok is None else [int(t) for t in np.asarray(step_tok)[b, :n_prev + j]]
            assert len(seen) == (0 if step_tok is None else n_prev + j)
            H = committed + seen
            suffix = H[len(H) - (n - 1):] if n > 1 else []
            for i in range(len(H) - n + 1):
                if H[i:i + n - 1] == suffix and 0 <= H[i + n - 1] < V:
                    view[b, j, H[i + n - 1]] = float("-inf")                       # a view: the assignment lands in x
    return x


class NgramOracleOps(FsmOracleOps):
    """FsmOracleOps + pack_no_repeat_ngram and no_repeat_ngram_rows on the reference above: the tiny stages run without a GPU."""

    def pack_no_repeat_ngram(self, ns, prompt_lens, P, device):
        self._note("pack_no_repeat_ngram", ())
        ns, lens = [int(n) for n in ns], [int(m) for m in prompt_lens]
        assert len(ns) == len(lens) and all(0 <= n <= MAX_NGRAM for n in ns) and all(0 <= m <= P for m in lens)   # what the stage hands over
        return SimpleNamespace(ns=ns, row_start=[int(P) - m for m in lens], P=int(P), B=len(ns))

    def no_repeat_ngram_rows(self, logits, ngram, tokens, seq_len, max_len, step_tok=None, n_prev=0):
        self._note("no_repeat_ngram_rows", ())
        assert ngram.B == logits.shape[0]
        return ref_no_repeat_ngram(logits, ngram.ns, tokens.numpy(), seq_len.tolist(), ngram.row_start, ngram.P, max_len,
                                   None if step_tok is None else step_tok.numpy(), n_prev)


class CallOrder:
    """Stands between a stage and the named ops of `ops` (instance attributes: the ops object stays what it is) and notes the
    order of their calls; works on the twin and on HipOps alike."""
    NAMES = ("pack_no_repeat_ngram", "no_repeat_ngram_rows", "bad_words_rows", "logit_mask_rows", "logit_edit_rows", "penalty_rows")

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
def banned_after(H, n):
    """The ids the rule bans at the position behind the history H (a list of ids): HF's definition, restated."""
    if n < 1 or len(H) < n:
        return set()
    suffix = list(H[len(H) - (n - 1):]) if n > 1 else []
    return {H[i + n - 1] for i in range(len(H) - n + 1) if list(H[i:i + n - 1]) == suffix}


def repeats(prompt, gen, n):
    """The positions p of `gen` at which the n-gram that ENDS there equals an earlier n-gram of prompt ++ gen."""
    return [p for p in range(len(gen)) if gen[p] in banned_after(list(prompt) + list(gen[:p]), n)]


def real_ids(stage, prompts):
    """Every row's prompt ids without the padding, and the padded prompt length."""
    ids, real = stage._encode(prompts)
    return real, ids.shape[1]


def check_no_repeat(real, texts, ns):
    for b, (t, n) in enumerate(zip(texts, ns)):
        if n > 0:
            assert not repeats(real[b], text_ids(t), n), (b, n, real[b], text_ids(t))


def _cpu(s):
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in s.items()}


def word_with_id(want, V, taken=()):
    """A word SimpleTokenizer folds to the id `want` of a vocabulary of V ids (crc32 of the word, mod 151936, mod V)."""
    for k in range(100000):
        w = f"w{k}"
        if zlib.crc32(w.encode("utf-8")) % 151936 % V == want and w not in taken:
            return w
    raise AssertionError(want)


# ------------------------------------------------------------------------------------------ stage-level scenarios
def scenario_greedy(stage, n):
    """Scenario 1.  Greedy with the rule off repeats n-grams in every row; with the rule on no n-gram that ends in the generated
    part equals an earlier one of prompt ++ generated, the tokens in front of the plain run's first repeat are the plain
    run's, the token there differs, and the log-probs are finite."""
    real, _ = real_ids(stage, PROMPTS)
    kw = dict(prompts=PROMPTS, max_tokens=NG_MAX_TOKENS, temperature=0.0)
    old = [text_ids(t) for t in stage.generate(**kw)[0]]
    at = [repeats(r, t, n) for r, t in zip(real, old)]
    assert all(len(a) >= 3 for a in at), at                                          # never vacuous: every row repeats
    texts, lps, _ = stage.generate(no_repeat_ngram_size=n, **kw)
    new = [text_ids(t) for t in texts]
    for b, a in enumerate(at):
        p = a[0]
        assert len(new[b]) == NG_MAX_TOKENS and new[b][:p] == old[b][:p] and new[b][p] != old[b][p], (b, p, old[b], new[b])
        assert np.isfinite(lps[b]).all()
    check_no_repeat(real, texts, [n] * len(PROMPTS))
    return texts


def check_kept_bans(stage, texts, ns, prompts):
    """Every kept step of a call WITHOUT mask, edit or bad word: the logits are -inf exactly where ref_no_repeat_ngram puts it on
    a replay from the recorded seq_len and proposals (the target's K + 1 positions at a verifying stage), and no proposal is
    one its history bans: the draft's side was banned too.  -> the number of (row, position) pairs with a non-empty ban set."""
    real, P = real_ids(stage, prompts)
    B = len(prompts)
    gen = [text_ids(t) for t in texts]
    cap = P + max(len(g) for g in gen)
    tokens = np.zeros((B, cap), dtype=np.int32)
    tokens[:, :P] = stage.encode_prompts(prompts).cpu().numpy()
    for b, g in enumerate(gen):
        tokens[b, P:P + len(g)] = g
    row_start = [P - len(r) for r in real]
    hits = 0
    assert stage.step_inputs
    for step, s in enumerate(map(_cpu, stage.step_inputs)):
        if "tok" in s:
            got = torch.cat([s["logits"], s["bonus"][:, None]], 1)                  # [B, K + 1, V]
            seq_len, tok = s["seq_len"].tolist(), s["tok"].numpy()
        else:
            got, seq_len, tok = s["logits"], [P + step] * B, None                   # stage 0 without a stop set: one token per step
        want = ref_no_repeat_ngram(torch.zeros(got.shape), ns, tokens, seq_len, row_start, P, cap, tok, 0)
        assert torch.equal(torch.isneginf(got), torch.isneginf(want)), step
        hits += int(torch.isneginf(want).any(-1).sum())
        for b in range(B):
            for j in range(0 if tok is None else tok.shape[1]):
                H = real[b] + gen[b][:seq_len[b] - P] + tok[b, :j].tolist()
                assert int(tok[b, j]) not in banned_after(H, ns[b]), (step, b, j)
    return hits


def scenario_sampled(stage):
    """Scenario 2.  Seeded and sampled at n = 2: the plain run repeats bigrams in every row, the run with the rule holds none;
    every kept step's -inf pattern is the reference's (check_kept_bans); the call repeated is bit-equal."""
    real, _ = real_ids(stage, PROMPTS)
    kw = dict(prompts=PROMPTS, max_tokens=NG_MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS)
    base = [text_ids(t) for t in stage.generate(**kw)[0]]
    assert all(len(repeats(r, t, 2)) >= 3 for r, t in zip(real, base)), base
    ns = [2] * len(PROMPTS)
    texts, lps, _ = run_kept(stage, no_repeat_ngram_size=2, **kw)
    check_no_repeat(real, texts, ns)
    assert all(np.isfinite(lp).all() for lp in lps)
    assert check_kept_bans(stage, texts, ns, PROMPTS) > 0
    again, lps2, _ = stage.generate(no_repeat_ngram_size=2, **kw)
    assert again == texts and all(a.tobytes() == b.tobytes() for a, b in zip(lps, lps2))
    return texts


PER_PROMPT = [2, 0, 3, 0, 1]


def scenario_per_prompt(stage):
    """Scenario 3.  Seeded, one n per prompt: the rows with 0 are bit-equal, in text and log-prob bytes, to the same call
    without the keyword; every other row b to row b of the call that gives EVERY row b's n."""
    real, _ = real_ids(stage, PROMPTS)
    kw = dict(prompts=PROMPTS, max_tokens=NG_MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS)
    base = stage.generate(**kw)
    assert all(repeats(r, text_ids(t), max(n, 1)) for r, t, n in zip(real, base[0], PER_PROMPT))
    mixed = stage.generate(no_repeat_ngram_size=PER_PROMPT, **kw)
    for b, n in enumerate(PER_PROMPT):
        alone = stage.generate(no_repeat_ngram_size=n, **kw) if n else base
        assert alone[0][b] == mixed[0][b], b
        assert alone[1][b].tobytes() == mixed[1][b].tobytes(), b
        assert n == 0 or mixed[0][b] != base[0][b], b
    check_no_repeat(real, mixed[0], PER_PROMPT)
    return mixed


def scenario_prompt_counts(stage):
    """Scenario 4.  The prompt is history, the padding is not.  Row 0's real ids are a b a: at n = 2 its first token is never b
    and the first step's logits are -inf at b and nowhere else.  Row 1's real ids are q 0, left-padded with id 0 to 0 q 0: the
    pad id in front of q would complete the match 0 -> q, and must not: its first logits hold no -inf."""
    V = stage.shape.vocab
    a, b, q = 5, 9, 7
    wa, wb, wq, w0 = (word_with_id(i, V) for i in (a, b, q, 0))
    prompts = [f"{wa} {wb} {wa}", f"{wq} {w0}"]
    real, P = real_ids(stage, prompts)
    assert real == [[a, b, a], [q, 0]] and P == 3 and stage.encode_prompts(prompts).tolist() == [[a, b, a], [0, q, 0]]
    texts, lps, _ = run_kept(stage, prompts=prompts, max_tokens=4, temperature=0.0, no_repeat_ngram_size=2)
    first = _cpu(stage.step_inputs[0])["logits"]
    first = first[:, 0] if first.dim() == 3 else first                               # a verifying stage: the first proposal's target row
    gone = torch.isneginf(first)
    assert gone[0].nonzero().flatten().tolist() == [b] and not gone[1].any()
    assert text_ids(texts[0])[0] != b and all(np.isfinite(lp).all() for lp in lps)
    check_no_repeat(real, texts, [2, 2])
    return texts


def scenario_composition(stage):
    """Scenario 5.  Greedy at n = 2 with an allow-list large enough for the rule, a bias, penalties, a bad word, logprobs = 2 and
    a stop id in one call: no bigram repeats, a top-N entry is finite only where the list allows and neither the rule nor the
    word bans, a committed token's log-prob is its table entry, and row 0 ends at its stop id."""
    V = stage.shape.vocab
    real, _ = real_ids(stage, PROMPTS)
    allowed = [t for t in range(V) if t % 16 != 3]                                   # 60 of 64 ids
    kw = dict(prompts=PROMPTS, max_tokens=NG_MAX_TOKENS, temperature=0.0, allowed_token_ids=allowed, logit_bias={allowed[3]: 1.0},
              repetition_penalty=1.02, frequency_penalty=0.02, logprobs=2)
    plain = [text_ids(t) for t in stage.generate(**kw)[0]]
    assert all(repeats(r, t, 2) for r, t in zip(real, plain)), plain                 # the mild penalties leave the loops in
    base = [text_ids(t) for t in stage.generate(no_repeat_ngram_size=2, **kw)[0]]
    unused = [next(t for t in allowed if t not in g and t not in r) for g, r in zip(base, real)]
    words = [[(u,), (u, g[0])] for u, g in zip(unused, base)]                        # (neither changes a greedy row that never takes u)
    stop = base[0][5]
    texts, lps, stats = stage.generate(no_repeat_ngram_size=2, bad_words_per_prompt=words, stop_token_ids=[stop], **kw)
    assert stats["finish_reasons"][0] == "stop" and text_ids(texts[0]) == base[0][:base[0].index(stop) + 1]
    check_no_repeat(real, texts, [2] * len(PROMPTS))
    for b, t in enumerate(map(text_ids, texts)):
        ids, top = stats["top_token_ids"][b], stats["top_logprobs"][b]
        assert ids.shape == top.shape == (len(t), 2) and np.isfinite(lps[b]).all()
        for i in range(len(t)):
            gone = banned_after(real[b] + t[:i], 2) | {unused[b]}
            for v, lp in zip(ids[i].tolist(), top[i].tolist()):
                assert not np.isfinite(lp) or (v in allowed and v not in gone), (b, i, v)
            assert ids[i][0] == t[i] and abs(float(lps[b][i]) - float(top[i][0])) <= PAIR_ATOL, (b, i)
    return texts


def scenario_call_trace(stage):
    """Scenario 6.  One pack_no_repeat_ngram; as many no_repeat_ngram_rows calls as bad_words_rows calls -- steps x (1 |
    draft_len + 1) -- each directly behind it and in front of logit_edit_rows; neither op with every n = 0."""
    kw = dict(prompts=PROMPTS, max_tokens=4, temperature=TEMPERATURE, seed=SEEDS, logit_bias={5: 1.0}, frequency_penalty=0.5,
              bad_words=[(2, 4), (6,)])
    log = CallOrder(stage.ops)
    try:
        stage.generate(no_repeat_ngram_size=[2, 0, 3, 0, 1], **kw)
        names, steps = list(log.names), stage.last_steps
        del log.names[:]
        for quiet_kw in (dict(), dict(no_repeat_ngram_size=0), dict(no_repeat_ngram_size=[0] * len(PROMPTS)),
                         dict(no_repeat_ngram_size=None)):
            stage.generate(**quiet_kw, **kw)
        quiet = list(log.names)
    finally:
        log.close()
    per_step = 1 if stage.draft is None else stage.config.draft_len + 1
    assert names.count("pack_no_repeat_ngram") == 1 and names.index("pack_no_repeat_ngram") < names.index("no_repeat_ngram_rows")
    assert names.count("no_repeat_ngram_rows") == names.count("bad_words_rows") == names.count("logit_edit_rows") == steps * per_step
    for i, n in enumerate(names):
        if n == "no_repeat_ngram_rows":
            assert (names[i - 1], names[i + 1], names[i + 2]) == ("bad_words_rows", "logit_edit_rows", "penalty_rows"), names[i - 1:i + 3]
    assert quiet.count("bad_words_rows") == 4 * names.count("bad_words_rows") and not [n for n in quiet if "ngram" in n]
    return names


PIPE_MAX_TOKENS = 12                             # (a request's prompt grows by every stage's output: 8 + 2 * 12 ids at the last
#                                                  stage, so bound_b = 32 + 12 + 4 stays below the 64 ids of the vocabulary)


def scenario_pipeline(manager):
    """Scenario 7, on the stages: one greedy pipeline run through all three stages with n = 2 differs from the plain run, which
    repeats bigrams, and holds no repeated bigram."""
    from asd_amd.serving.pipeline import AdaptiveSpeculativePipeline, PipelineConfig
    cfg = PipelineConfig(lambda_value=100.0, stop_rule="full", stage_names=NAMES)
    pipe = AdaptiveSpeculativePipeline(manager, LogprobPredictor(), object(), cfg)
    kw = dict(max_tokens=PIPE_MAX_TOKENS, temperature=0.0)
    plain = pipe.batch_process(PROMPTS, **kw)
    res = pipe.batch_process(PROMPTS, no_repeat_ngram_size=2, **kw)
    pipe.shutdown()
    assert max(r.stages_run for r in res) > 1
    assert all(len(text_ids(r.output)) == PIPE_MAX_TOKENS for r in res)
    assert [r.output for r in res] != [r.output for r in plain]
    assert any(repeats([], text_ids(r.output), 2) for r in plain)                    # (12 tokens: not every row has looped yet)
    assert not any(repeats([], text_ids(r.output), 2) for r in res)
    return res


__all__ = ["CallOrder", "NG_MAX_TOKENS", "NgramOracleOps", "PER_PROMPT", "PIPE_MAX_TOKENS", "VOCAB", "banned_after", "check_kept_bans", "check_no_repeat",
           "real_ids", "ref_no_repeat_ngram", "repeats", "scenario_call_trace", "scenario_composition", "scenario_greedy",
           "scenario_per_prompt", "scenario_pipeline", "scenario_prompt_counts", "scenario_sampled", "word_with_id"]
