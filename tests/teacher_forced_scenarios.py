"""The scenarios tests/test_teacher_forced_stages.py (CPU twin) and tests/test_gpu_teacher_forced_stages.py (HipOps) share: every
generate call below is checked by tests/teacher_forced_ref.py::check from what it RETURNED alone.  The stages are the three tiny
ones of tests/stage_scenario.py (vocabulary 1000, 5 prompts, 12 tokens, draft_len 4).  "13b" shares its draft's weights and
verifies untruncated what the draft proposed under top_p = 0.9: its steps accept 0 .. 4 proposals, so partial acceptances, whole
blocks and bonus rows all occur there.  "34b" and its draft are unrelated random models: its steps accept next to nothing, which
is the path on which every token is a residual draw and every proposal's KV entry is overwritten.  The scenarios behind
everything() add guided rows, no_repeat_ngram_size (on the same stages at vocabulary 64, where bans are live) and prompt_logprobs.

TEST INFRASTRUCTURE: never importable from the package."""
from tests.logit_edit_ref import SEEDS
from tests.penalty_ref import RECUR, RECUR_BIAS
from tests.per_request_ref import MIXED, TRUNCATED
from tests.stage_scenario import MAX_TOKENS, PROMPTS, TEMPERATURE, text_ids
from tests.teacher_forced_ref import recurring, run_checked

KW = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE)
TARGET_TRUNCATION = {"top_k": dict(top_k=20), "top_p": dict(top_p=0.8), "min_p": dict(min_p=0.1),
                     "all": dict(top_k=50, top_p=0.9, min_p=0.05)}
ROWS = {"mixed": MIXED, "truncated": TRUNCATED}
SHORT_PROMPTS = ["hard", "two words", "easy", "one more", "x"]                   # one and two tokens: P = 2, no draft prefill
# penalties of both signs, one per row (row 1 neutral); rep = 2.0 and 0.8 amplify a logit error by 2 and 1.25
PENALTIES = dict(repetition_penalty=[1.3, 1.0, 0.8, 1.1, 2.0], presence_penalty=[0.5, 0.0, -1.0, 0.0, 2.0],
                 frequency_penalty=[0.25, 0.0, 0.5, -0.5, 0.0])
GREEDY_PENALTIES = dict(repetition_penalty=1.2, presence_penalty=0.5, frequency_penalty=0.5)


def label(stage, what):
    return f"{stage.name} {str(stage.config.dtype).split('.')[-1]} {what}"


def defaults(stage, lp_bar, seeded, prompts=PROMPTS, **extra):
    """Scenario 1: stage 0 draws under its configured top_p = 0.9, a verifying stage against its untruncated target."""
    kw = dict(KW, prompts=prompts, **(dict(seed=SEEDS[:len(prompts)]) if seeded else {}), **extra)
    return run_checked(stage, lp_bar, label(stage, "defaults seeded" if seeded else "defaults"), **kw)[1]


def target_truncation(stage, lp_bar, which):
    """Scenario 2: top_k, top_p, min_p of the stage's own distribution, each alone and all three together."""
    out, rep = run_checked(stage, lp_bar, label(stage, "truncation " + which), **KW, seed=SEEDS, **TARGET_TRUNCATION[which])
    return rep


def rows_route(stage, lp_bar, which):
    """Scenario 3: one (temperature, top_k, top_p, min_p) per prompt; every row is checked at its own four values."""
    kw = dict(KW, seed=SEEDS, **ROWS[which])
    return run_checked(stage, lp_bar, label(stage, "rows " + which), **kw)[1]


def ragged_ends(stage, lp_bar, sync_every):
    """Scenario 4: rows that end at different steps, mid-step, while the loop goes on behind them -- stop ids (with
    min_tokens) chosen from a free run; 2- and 3-token stop sequences per prompt with per-prompt limits."""
    old = stage.config.sync_every
    stage.config.sync_every = sync_every
    try:
        kw = dict(KW, seed=SEEDS)
        free = [text_ids(t) for t in stage.generate(**kw)[0]]
        # a stop id two rows commit early: row 0's third token and row 2's first (held back there by min_tokens)
        stops = list(dict.fromkeys([free[0][2], free[2][0]]))
        (_, _, st), rep1 = run_checked(stage, lp_bar, label(stage, f"stop ids + min_tokens, sync {sync_every}"), **kw,
                                       stop_token_ids=stops, min_tokens=[0, 3, 5, 1, 2])
        assert "stop" in st["finish_reasons"] and len(set(st["n_tokens"])) > 1, st
        seqs = [[tuple(free[0][3:5])], [], [tuple(free[2][1:4])], [tuple(free[3][5:8])], [tuple(free[4][8:10])]]   # row 4's lies behind its limit
        kw2 = dict(kw, max_tokens=[12, 5, 9, 12, 7])
        (_, _, st), rep2 = run_checked(stage, lp_bar, label(stage, f"stop sequences + limits, sync {sync_every}"), **kw2,
                                       stop_sequences_per_prompt=seqs)
        assert {"stop", "length"} <= set(st["finish_reasons"]) and len(set(st["n_tokens"])) > 2, st
        assert {len(m) for m in st["stop_matches"] if m} == {2, 3}, st["stop_matches"]
    finally:
        stage.config.sync_every = old
    return rep1, rep2


def everything(stage, lp_bar, prompts=PROMPTS, max_tokens=MAX_TOKENS, **extra):
    """Scenario 5, seeded, logprobs = 5: an allow-list per prompt (row 1 none, row 3 four tokens: fewer than the table), bad
    words of 1, 2 and 3 tokens from a free run, a bias that makes a token recur, a ban, min_tokens, penalties of both signs per
    row (row 1 neutral) and a stop id.  Log-probs, top-N tables and ends are checked."""
    n, V = len(prompts), stage.shape.vocab
    short = [RECUR, 5, 6, 7]
    allowed = [None if b == 1 else short if b == 3 else sorted(set(range(b % 2, V, 2)) | {RECUR}) for b in range(n)]
    kw = dict(prompts=prompts, max_tokens=max_tokens, temperature=TEMPERATURE, seed=SEEDS[:n], logprobs=5,
              allowed_token_ids=allowed, logit_bias=RECUR_BIAS, **{k: v[:n] for k, v in PENALTIES.items()}, **extra)
    (texts, _, _), _ = run_checked(stage, lp_bar, label(stage, "everything: free run"), **kw)
    free = [text_ids(t) for t in texts]
    words = [[] if b == 3 else [(g[-1],), tuple(g[0:2]), tuple(g[2:5])] for b, g in enumerate(free)]
    outside = [t for g in free for t in g if t != RECUR and t not in short]
    stop, ban = outside[3], next(t for t in outside[4:] if t != outside[3])
    out, rep = run_checked(stage, lp_bar, label(stage, "everything"), **kw, bad_words_per_prompt=words, stop_token_ids=[stop],
                           banned_token_ids=[ban], min_tokens=[0, 3, 5, 1, 2][:n])
    gens = [text_ids(t) for t in out[0]]
    assert recurring(gens) and all(ban not in g for g in gens)
    assert all((i < 0) == (j >= 4) for row in out[2]["top_token_ids"][3] for j, i in enumerate(row))   # the 4-token list: slot 4 unfillable
    return rep


# ------------------------------------------------------------------------------------------ guided rows, n-gram bans, prompt log-probs
STOP = 2
A, B_TOK, C = 40, 41, 43
CHOICES = [(5, 17, 300), (5, 17), (5, 900, 31, 32)]                              # (5, 17): an inner accepting node
OTHER_CHOICES = [(640, 3), (11,), (640, 4, 4, 4)]
GUIDED_HOW = ("defaults", "all", "mixed", "sync1", "sync4", "greedy")


def guided_cases(names):
    """(stage, how) of the guided scenario: "all" is TARGET truncation, so it runs on the verifying stages."""
    return [(name, how) for name in names for how in GUIDED_HOW if how != "all" or name != names[0]]


def _fsms():
    """-> (A, a free token that is not B_TOK, a second free token, C, then only the stop id: `other` states and a forbidden edge;
    a chain of 13 free tokens, B_TOK forbidden in each, whose only accepting state lies behind them: 12 tokens cut it)."""
    from asd_amd.serving.guided import TokenFSM
    free = TokenFSM(5, 0, [{A: 1}, {B_TOK: -1}, {}, {C: 4}, {}], [-1, 2, 3, -1, -1], accepting=[4])
    long = TokenFSM(14, 0, [{B_TOK: -1}] * 13 + [{}], list(range(1, 14)) + [-1], accepting=[13])
    return free, long


def cycle3(V):
    """A three-state TokenFSM over the whole vocabulary: the token at generated position i is congruent to i mod 3.  Every state
    allows another third of the ids, so a state that is one transition off forbids the token the row should produce; every
    state is accepting, so a stop id may end the row anywhere."""
    from asd_amd.serving.guided import TokenFSM
    return TokenFSM(3, 0, [{t: (s + 1) % 3 for t in range(s, V, 3)} for s in range(3)], accepting=[0, 1, 2])


def guided(stage, lp_bar, how):
    """Seeded, logprobs = 5 (a choice row allows one or two tokens: unfillable slots), a different kind of row per prompt:
    choices one of which is a prefix of another; a free row; a general TokenFSM; a second choice list; a TokenFSM that
    max_tokens cuts ("length").  `how`: the stage's defaults (stage 0's top_p = 0.9); "all": the stage's own top-k, top-p and
    min-p together; the rows route MIXED; sync_every 1 and 4; greedy."""
    free, long = _fsms()
    kw = dict(KW, seed=SEEDS, logprobs=5, stop_token_ids=[STOP], guided_fsm=[None, None, free, None, long],
              guided_choice_per_prompt=[CHOICES, None, None, OTHER_CHOICES, None])
    kw.update(TARGET_TRUNCATION["all"] if how == "all" else MIXED if how == "mixed" else dict(temperature=0.0) if how == "greedy" else {})
    if how == "greedy":
        del kw["seed"]
    old = stage.config.sync_every
    stage.config.sync_every = {"sync1": 1, "sync4": 4}.get(how, old)
    try:
        (texts, _, st), rep = run_checked(stage, lp_bar, label(stage, "guided " + how), **kw)
    finally:
        stage.config.sync_every = old
    gens = [text_ids(t) for t in texts]
    assert st["finish_reasons"][0] == st["finish_reasons"][2] == st["finish_reasons"][3] == "stop", st["finish_reasons"]
    assert st["finish_reasons"][4] == "length" and len(gens[4]) == MAX_TOKENS and B_TOK not in gens[4]
    assert (gens[2][0], gens[2][3:]) == (A, [C, STOP]) and gens[2][1] != B_TOK
    assert all(i < 0 for row in st["top_token_ids"][0] for i in row[2:])         # a choice row: at most two tokens are allowed
    return rep


NGRAM_VOCAB = 64                                 # a manager at this vocabulary, as the feature's own stage tests: bans are live
NGRAM_ROWS = [2, 0, 3, 1, 8]
NGRAM_RECUR = 7
NGRAM_LIMITS = [MAX_TOKENS, MAX_TOKENS, 32, MAX_TOKENS, MAX_TOKENS]              # the n = 3 row: up to ngram_ref.NG_MAX_TOKENS


def ngram(stage, lp_bar, greedy):
    """One n per prompt and a bias that makes a token recur, on a stage of vocabulary 64.  Liveness comes from the f64 reference
    alone (teacher_forced_ref: positions whose ban removes more mass than the bound): at least 3 on the n = 1 row and on the
    n = 2 row; -> the figures, whose n = 3 row the caller sums over the scenario."""
    assert stage.shape.vocab == NGRAM_VOCAB
    kw = dict(prompts=PROMPTS, max_tokens=NGRAM_LIMITS, no_repeat_ngram_size=NGRAM_ROWS, logit_bias={NGRAM_RECUR: 4.0},
              **(dict(temperature=0.0) if greedy else dict(temperature=TEMPERATURE, seed=SEEDS)))
    _, rep = run_checked(stage, lp_bar, label(stage, "n-gram greedy" if greedy else "n-gram"), **kw)
    live = rep["ngram_live"]
    assert live[3] >= 3 and live[0] >= 3 and live[1] == 0, live
    return rep


def everything_now(stage, lp_bar, prompts=PROMPTS, max_tokens=MAX_TOKENS, **extra):
    """everything()'s call with the three later features: row 0 follows a TokenFSM (cycle3; it has no min_tokens and
    no n), rows 1, 2 and 4 have n = 2, 3 and 1 (row 3's four-token list is smaller than any n-gram bound), and
    prompt_logprobs = 5.  Log-probs, generated tables, ends, prompt log-probs, ranks and prompt tables are checked."""
    n, V = len(prompts), stage.shape.vocab
    short = [RECUR, 5, 6, 7]
    allowed = [None if b == 1 else short if b == 3 else sorted(set(range(b % 2, V, 2)) | {RECUR}) for b in range(n)]
    kw = dict(prompts=prompts, max_tokens=max_tokens, temperature=TEMPERATURE, seed=SEEDS[:n], logprobs=5,
              allowed_token_ids=allowed, logit_bias=RECUR_BIAS, **{k: v[:n] for k, v in PENALTIES.items()},
              guided_fsm=[cycle3(V), None, None, None, None][:n], no_repeat_ngram_size=[0, 2, 3, 0, 1][:n],
              prompt_logprobs=5, **extra)
    (texts, _, _), _ = run_checked(stage, lp_bar, label(stage, "everything now: free run"), **kw)
    free = [text_ids(t) for t in texts]
    words = [[] if b == 3 else [(g[-1],), tuple(g[0:2]), tuple(g[2:5])] for b, g in enumerate(free)]
    outside = [t for g in free for t in g if t != RECUR and t not in short]
    # (the stop id is no last id of a bad word of the guided row: the state behind it would keep no token, which generate refuses)
    stop = next(t for t in outside[3:] if t not in {w[-1] for w in words[0]})
    ban = next(t for t in outside[4:] if t != stop)
    out, rep = run_checked(stage, lp_bar, label(stage, "everything now"), **kw, bad_words_per_prompt=words, stop_token_ids=[stop],
                           banned_token_ids=[ban], min_tokens=[0, 3, 5, 1, 2][:n])
    gens = [text_ids(t) for t in out[0]]
    assert recurring(gens) and all(ban not in g for g in gens)
    assert all((i < 0) == (j >= 4) for row in out[2]["top_token_ids"][3] for j, i in enumerate(row))   # the 4-token list: slot 4 unfillable
    body = gens[0][:-1] if out[2]["finish_reasons"][0] == "stop" else gens[0]   # (every state is accepting: the stop id ends it anywhere)
    assert all(t % 3 == i % 3 for i, t in enumerate(body))                       # the automaton
    return rep


PROMPT_HOW = ((0, "sampled"), (3, "sampled"), (8, "sampled"), (3, "greedy"), (3, "processors"))


def prompt(stage, lp_bar, n, how, **extra):
    """prompt_logprobs = n on PROMPTS (rows with m = 0 and m = 1): sampled and seeded, greedy, and with processors on -- the
    prompt's numbers are the raw model's regardless."""
    kw = dict(KW, prompt_logprobs=n, **extra)
    if how == "greedy":
        kw["temperature"] = 0.0
    else:
        kw["seed"] = SEEDS
    if how == "processors":
        V = stage.shape.vocab
        kw.update(allowed_token_ids=[t for t in range(V) if t % 4 != 1], logit_bias=RECUR_BIAS, no_repeat_ngram_size=2, **PENALTIES)
    (_, _, st), rep = run_checked(stage, lp_bar, label(stage, f"prompt_logprobs {n} {how}"), **kw)
    m = [len(v) for v in st["prompt_logprobs"]]
    assert 0 in m and 1 in m and max(m) > 2 and rep["prompt_entries"] == sum(m), m
    return rep


def edge_now(make_manager, lp_bar, which):
    """The edges of the loop, crossed with a guided row, n-gram rows and prompt_logprobs = 2.  With one row the guided call and
    the n-gram call are two."""
    margs, gargs = EDGES[which]
    sm = make_manager(**margs)
    reps = []
    for name in sm.names:
        stage = sm.get_stage(name)
        kw = {**KW, "seed": SEEDS, "logit_bias": RECUR_BIAS, "stop_token_ids": [STOP], "prompt_logprobs": 2, **gargs}
        B = len(kw["prompts"])
        calls = [dict(guided_fsm=[cycle3(stage.shape.vocab), None, None, None, None][:B], no_repeat_ngram_size=[0, 1, 0, 2, 3][:B])]
        if B == 1:
            calls.append(dict(no_repeat_ngram_size=[1]))
        for more in calls:
            (_, _, st), rep = run_checked(stage, lp_bar, label(stage, which + " now"), **kw, **more)
            reps.append(rep)
            kept = [[i % stage.shape.vocab for i in stage.tokenizer.encode(p, return_tensors=None)] for p in kw["prompts"]]
            if which == "max_prompt_tokens_3":                                   # the prompt's kept ids are its last 3
                kept = [r[-3:] for r in kept]
                assert any(len(r) == 3 for r in kept)
            assert [v.tolist() for v in st["prompt_token_ids"]] == kept
    return sm, reps


def back_to_back_now(stage, lp_bar):
    """One manager: everything_now -> a plain seeded call -> guided.  The plain call holds no prompt key (the check asserts it),
    and a state or a ban left over would move its log-probs off the plain reference."""
    everything_now(stage, lp_bar)
    (_, _, st), _ = run_checked(stage, lp_bar, label(stage, "a plain call behind everything now"), **dict(KW, prompts=PROMPTS[:3], seed=SEEDS[:3]))
    assert not [k for k in st if k.startswith("prompt_") or k.startswith("top_")], sorted(st)
    guided(stage, lp_bar, "defaults")


def bf16_now(stage, lp_bar):
    """The default (bfloat16) stages under everything_now and prompt and the same formulas: coarse, as bf16() says; stage 0 at
    top_p = 1 for the reason given there."""
    extra = dict(top_p=1.0) if stage.draft is None else {}
    return everything_now(stage, lp_bar, **extra), prompt(stage, lp_bar, 3, "sampled", **extra)


def greedy(stage, lp_bar):
    """Scenario 7: temperature 0 with a stop id and the penalties."""
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0, logit_bias=RECUR_BIAS, **GREEDY_PENALTIES)
    free = [text_ids(t) for t in stage.generate(**kw)[0]]
    stop = next(t for g in free for t in g[2:5] if t != RECUR)
    (_, _, st), rep = run_checked(stage, lp_bar, label(stage, "greedy"), **kw, stop_token_ids=[stop])
    assert "stop" in st["finish_reasons"], st
    return rep


def back_to_back(stage, lp_bar):
    """Scenario 8: one manager, calls back to back, each checked -- nothing of a call's state (penalty state, the step's
    proposals, finished flags, cached workspaces) may reach the next."""
    everything(stage, lp_bar)
    defaults(stage, lp_bar, seeded=True, prompts=PROMPTS[:3])
    ragged_ends(stage, lp_bar, 4)


# The edges of the loop: (manager arguments, generate arguments).  Each runs seeded on all three stages of a fresh manager.
EDGES = {
    "short_prompts": (dict(), dict(prompts=SHORT_PROMPTS)),                       # P = 2: the draft is not prefilled
    "max_prompt_tokens_3": (dict(max_prompt_tokens=3), dict()),                  # the prompts are cut to their last 3 ids
    "one_row": (dict(), dict(prompts=PROMPTS[:1], seed=SEEDS[:1])),
    "one_token": (dict(), dict(max_tokens=1)),
    "draft_len_1": (dict(draft_len=1), dict()),
    "draft_len_8": (dict(draft_len=8), dict()),                                  # 12 tokens: the cap cuts a step
    "seven_tokens": (dict(), dict(max_tokens=7)),                                # not a multiple of K + 1
}


def edge(make_manager, lp_bar, which):
    """Scenario 6.  make_manager(**manager arguments) -> a StageManager of float32 stages."""
    margs, gargs = EDGES[which]
    sm = make_manager(**margs)
    reps = []
    for name in sm.names:
        stage = sm.get_stage(name)
        kw = {**KW, "seed": SEEDS, **gargs}
        reps.append(run_checked(stage, lp_bar, label(stage, which), **kw)[1])
        if which == "short_prompts":
            assert stage.encode_prompts(kw["prompts"]).shape[1] == 2
        if which == "max_prompt_tokens_3":
            assert stage.encode_prompts(kw["prompts"]).shape[1] == 3
    return sm, reps


def bf16(stage, lp_bar):
    """Scenario 10: the default (bfloat16) stages under scenarios 1 and 5 and the same formulas.  eps_x is near 0.5 there, so
    the bound is near 1.5 -- coarse; the sharp check is the float32 one.  STAGE 0 IS RUN AT top_p = 1: under its configured
    top_p = 0.9 a logit move of eps_x = 0.5 shifts the upper mass of any set by far more than one token's share (about 1e-3 at
    vocabulary 1000), so the f64 reference alone calls EVERY position ambiguous (60 of 60 on the CPU twin) and no choice of
    seeds can keep it inside the 5 % cap; untruncated, the share is 0 and every log-prob is checked against one value.  The
    verifying stages run as configured: their proposals still come from stage 0's model under its top_p = 0.9, cast to the
    target's dtype for the residual draw."""
    extra = dict(top_p=1.0) if stage.draft is None else {}
    return defaults(stage, lp_bar, seeded=True, **extra), everything(stage, lp_bar, **extra)
