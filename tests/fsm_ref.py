"""Guided decoding (serving/stages.py, GUIDED DECODING; include/asd_hip.h, asd_fsm_mask_rows / asd_fsm_advance / asd_fsm_commit):
the numpy references of the three kernels, written from the header's text, the oracle ops twin that runs the stages through them,
a dict-based reference automaton that shares no code with serving/guided.py, and the stage-level scenarios that
tests/test_fsm_stages.py (CPU twin) and tests/test_gpu_fsm_stages.py (HipOps) both run.

TEST INFRASTRUCTURE, like tests/bad_words_ref.py: never importable from the package."""
from types import SimpleNamespace

import numpy as np
import torch

from tests import teacher_forced_ref as TF
from tests.bad_words_ref import EQUAL_PROMPTS, BadWordsOracleOps
from tests.logit_edit_ref import SEEDS, run_kept
from tests.stage_scenario import DRAFT_LEN, MAX_TOKENS, PROMPTS, TEMPERATURE, text_ids
from tests.token_mask_ref import allow_list, ref_logit_mask
from tests.top_logprobs_ref import PAIR_ATOL


# ------------------------------------------------------------------------------------------ the kernels' references
def tables_of(state_first, edge_tok, edge_next, state_other, V):
    a = lambda v: np.asarray(v, dtype=np.int64).reshape(-1)                          # noqa: E731
    return SimpleNamespace(state_first=a(state_first), edge_tok=a(edge_tok), edge_next=a(edge_next), state_other=a(state_other),
                           S=len(a(state_other)), E=len(a(edge_tok)), V=int(V))


def ref_delta(t, s, tok):
    """delta(s, tok) by the header's table; the edge range of a state is clamped into [0, E]."""
    s, tok = int(s), int(tok)
    if not 0 <= s < t.S or not 0 <= tok < t.V:
        return s
    lo = min(max(int(t.state_first[s]), 0), t.E)
    hi = min(max(int(t.state_first[s + 1]), lo), t.E)
    at = np.nonzero(t.edge_tok[lo:hi] == tok)[0]                                     # ids are distinct within a state
    to = int(t.edge_next[lo + int(at[0])]) if at.size else int(t.state_other[s])
    return to if 0 <= to < t.S else s


def ref_state_bits(t):
    """uint32 [S, W]: bit v of row s set = token v has a transition in s that is not -1."""
    bits = np.zeros((t.S, (t.V + 31) // 32), dtype=np.uint32)
    for s in range(t.S):
        keep = np.full(t.V, bool(t.state_other[s] >= 0))
        for i in range(int(t.state_first[s]), int(t.state_first[s + 1])):
            keep[int(t.edge_tok[i])] = t.edge_next[i] >= 0
        for v in np.nonzero(keep)[0]:
            bits[s, v >> 5] |= np.uint32(1 << (int(v) & 31))
    return bits


def ref_fsm_mask(x, bits, pos_state, first=0):
    """asd_fsm_mask_rows on a CPU tensor, IN PLACE (-> x): position j of sequence b is masked with row pos_state[b][first + j]
    of bits; a state outside [0, S) leaves the position alone."""
    view = x[:, None] if x.dim() == 2 else x
    for b in range(view.shape[0]):
        for j in range(view.shape[1]):
            ref_logit_mask(view[b:b + 1, j:j + 1], bits, [int(pos_state[b][first + j])])
    return x


def ref_fsm_advance(t, pos_state, k, step_tok):
    """asd_fsm_advance, IN PLACE on the numpy array pos_state [B, ld_state]."""
    for b in range(pos_state.shape[0]):
        pos_state[b, k + 1] = ref_delta(t, pos_state[b, k], step_tok[b][k])


def ref_fsm_commit(t, pos_state, tokens, seq_len, n_commit, max_len):
    """asd_fsm_commit, IN PLACE on the numpy array pos_state [B, ld_state]."""
    for b in range(pos_state.shape[0]):
        c = int(n_commit[b])
        if c <= 0:
            continue
        c = min(c, pos_state.shape[1])
        L = min(max(int(seq_len[b]), 1), max_len)
        pos_state[b, 0] = ref_delta(t, pos_state[b, c - 1], tokens[b][L - 1])


class FsmOracleOps(BadWordsOracleOps):
    """BadWordsOracleOps + pack_fsm, fsm_mask_rows, fsm_advance and fsm_commit on the references above."""

    def pack_fsm(self, fsm, ld_state, device):
        self._note("pack_fsm", ())
        t = tables_of(fsm.state_first, fsm.edge_tok, fsm.edge_next, fsm.state_other, fsm.V)
        assert t.S <= 1024 and t.E <= 2 ** 20 and all(-1 <= s < t.S for s in fsm.starts)      # what the stage hands over
        pos = np.repeat(np.asarray(fsm.starts, dtype=np.int32).reshape(-1, 1), ld_state, axis=1)
        return SimpleNamespace(t=t, bits=ref_state_bits(t), pos_state=pos, B=len(fsm.starts), ld_state=int(ld_state))

    def fsm_mask_rows(self, logits, fsm, first=0):
        self._note("fsm_mask_rows", ())
        assert fsm.B == logits.shape[0] and first + (1 if logits.dim() == 2 else logits.shape[1]) <= fsm.ld_state
        return ref_fsm_mask(logits, fsm.bits, fsm.pos_state, first)

    def fsm_advance(self, fsm, step_tok, k):
        self._note("fsm_advance", ())
        ref_fsm_advance(fsm.t, fsm.pos_state, k, step_tok.numpy())

    def fsm_commit(self, fsm, tokens, seq_len, n_commit, max_len):
        self._note("fsm_commit", ())
        ref_fsm_commit(fsm.t, fsm.pos_state, tokens.numpy(), seq_len.tolist(), n_commit.tolist(), max_len)


# ------------------------------------------------------------------------------------------ the reference automaton
class RefAutomaton:
    """The module docstring's rules on dicts: `edges`, `other`, `accepting` as TokenFSM takes them, Z the row's stop ids.  END
    (state n) allows exactly Z and loops; an accepting state sends a z without an explicit edge to END; elsewhere such a z is
    forbidden, even under `other`."""

    def __init__(self, n, start, edges, other, accepting, Z, V):
        self.n, self.start, self.V, self.Z = n, start, V, set(Z)
        self.edges = [dict(e) for e in edges] + [{}]
        self.other = list(other if other is not None else [-1] * n) + [-1]
        self.accepting = set(accepting)

    @classmethod
    def of_choices(cls, choices, Z, V):
        edges, acc = [{}], set()
        for c in choices:
            s = 0
            for t in c:
                if t not in edges[s]:
                    edges[s][t] = len(edges)
                    edges.append({})
                s = edges[s][t]
            acc.add(s)
        return cls(len(edges), 0, edges, None, acc, Z, V)

    def to(self, s, t):
        """The next state of token t in state s, or -1."""
        if s == self.n:
            return self.n if t in self.Z else -1
        if t in self.edges[s]:
            return self.edges[s][t]
        if t in self.Z:
            return self.n if s in self.accepting else -1
        return self.other[s]

    def allowed(self, s):
        """bool [V]: `to(s, t) >= 0` for every t, without asking for each of the V tokens one by one."""
        keep = np.full(self.V, self.to(s, -1) >= 0)              # -1 is no edge and no stop id: what a token without an edge gets
        for t in set(self.edges[s]) | self.Z:
            keep[t] = self.to(s, t) >= 0
        return keep

    def run(self, tokens, s=None):
        """The state behind `tokens`; every token must be allowed where it stands."""
        s = self.start if s is None else s
        for t in tokens:
            nxt = self.to(s, int(t))
            assert nxt >= 0, (s, int(t), list(tokens))
            s = nxt
        return s


# ------------------------------------------------------------------------------------------ stage-level scenarios
STOP = 2
CHOICES = [(5, 17, 300), (5, 17, 301, 42), (5, 900), (999, 0, 31, 32, 64, 7, 8, 9), (5, 17)]     # (5, 17): an inner accepting node
OTHER_CHOICES = [(640, 3), (11,), (640, 4, 4, 4)]
assert max(map(len, CHOICES + OTHER_CHOICES)) <= 8 and 8 + 1 <= MAX_TOKENS          # choice + stop id fits every row: a condition


def _cpu(s):
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in s.items()}


def check_choice_rows(texts, stats, rows, stop=STOP):
    """Every guided row: exactly one of its choices followed by one stop id, reason "stop"."""
    for b, choices in enumerate(rows):
        if not choices:
            continue
        g = text_ids(texts[b])
        assert tuple(g[:-1]) in set(choices) and g[-1] == stop, (b, g)
        assert stats["finish_reasons"][b] == "stop" and stats["stop_matches"][b] == (stop,), (b, stats["finish_reasons"][b])


def scenario_choices(stage, greedy):
    """Scenario 1.  Every row's tokens are exactly one of the choices plus one stop id, by "stop", greedy and sampled with seeds;
    the stop id as a one-token stop sequence does the same; with max_tokens shorter than the shortest choice a row ends by
    "length" holding a prefix of a choice."""
    kw = dict(prompts=PROMPTS, temperature=0.0) if greedy else dict(prompts=PROMPTS, temperature=TEMPERATURE, seed=SEEDS)
    texts, lps, stats = stage.generate(max_tokens=MAX_TOKENS, guided_choice=CHOICES, stop_token_ids=[STOP], **kw)
    check_choice_rows(texts, stats, [CHOICES] * len(PROMPTS))
    assert all(np.isfinite(lp).all() and (lp <= 1e-6).all() for lp in lps)
    again = stage.generate(max_tokens=MAX_TOKENS, guided_choice=CHOICES, stop_sequences=[(STOP,)], stop_token_ids=[], **kw)
    assert again[0] == texts and again[2]["finish_reasons"] == ["stop"] * len(PROMPTS)
    long = [c for c in CHOICES if len(c) >= 3]
    short, _, st = stage.generate(max_tokens=2, guided_choice=long, stop_token_ids=[STOP], **kw)
    for b, t in enumerate(map(text_ids, short)):
        assert st["finish_reasons"][b] == "length" and len(t) == 2 and any(tuple(t) == c[:2] for c in long), (b, t)
    return texts


def scenario_rows_independent(stage):
    """Scenario 2.  Seeded, equal-length prompts, one list per prompt (rows 1 and 3 unguided: None and []): an unguided row is
    bit-equal, in text and log-prob bytes, to the same call without guidance; a guided row to the call that gives EVERY row
    its list."""
    kw = dict(prompts=EQUAL_PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, stop_token_ids=[STOP])
    rows = [CHOICES, None, OTHER_CHOICES, [], CHOICES]
    base = stage.generate(**kw)
    mixed = stage.generate(guided_choice_per_prompt=rows, **kw)
    alone = {}
    for b, choices in enumerate(rows):
        key = tuple(choices or ())
        if key not in alone:
            alone[key] = stage.generate(guided_choice=choices, **kw) if choices else base
        assert alone[key][0][b] == mixed[0][b], b
        assert alone[key][1][b].tobytes() == mixed[1][b].tobytes(), b
    check_choice_rows(mixed[0], mixed[2], rows)
    return mixed


class MaskRecorder:
    """Stands between a stage and ops.fsm_mask_rows (an instance attribute: the ops object stays what it is; the twin and HipOps
    alike) and keeps, for every call, `first`, the logits' rank and the -inf set the logits have directly behind it -- the only
    place the DRAFT proposals' masked logits can be seen: the kept step records hold the target's rows only."""

    def __init__(self, ops):
        self.ops, self.calls = ops, []

        def wrapped(logits, fsm, first=0, _orig=ops.fsm_mask_rows):
            out = _orig(logits, fsm, first)
            self.calls.append((int(first), logits.dim(), torch.isneginf(logits).cpu().numpy()))
            return out
        ops.fsm_mask_rows = wrapped

    def close(self):
        del self.ops.fsm_mask_rows


def run_kept_recorded(stage, **kw):
    """run_kept with a MaskRecorder around it -> (generate's result, the recorder's calls)."""
    rec = MaskRecorder(stage.ops)
    try:
        return run_kept(stage, **kw), rec.calls
    finally:
        rec.close()


def check_kept_masks(stage, texts, autos, prompts, calls, extra=None):
    """Every kept step: replay the reference automaton over the row's committed stream and the step's proposals.  The -inf set
    of target row j (stage 0: of the one row) AND of draft proposal row j -- `calls`, a MaskRecorder's: what the draft logits
    held directly behind the fsm_mask_rows call with first = j -- equals the complement of the replayed state's allowed set,
    together with `extra(b)`, bool [V]: what the operations in front of the automaton's call (the allow-list) remove.  A free
    row's logits hold no -inf on either side.  Every recorded call has the rank and `first` the loop owes it.
    -> the number of (row, position) pairs checked, target and draft."""
    P = stage.encode_prompts(prompts).shape[1]
    gen = [text_ids(t) for t in texts]
    n_checked = 0
    assert stage.step_inputs
    spec = stage.draft is not None
    Kd = stage.config.draft_len if spec else 0
    assert len(calls) == len(stage.step_inputs) * (Kd + 1), (len(calls), len(stage.step_inputs))
    for step, s in enumerate(map(_cpu, stage.step_inputs)):
        mine = calls[step * (Kd + 1):(step + 1) * (Kd + 1)]
        # draft_len calls on one proposal's [B, V] logits with first = k, then one on the target's [B, K+1, V] output; stage 0: one
        assert [(f, d) for f, d, _ in mine] == [(k, 2) for k in range(Kd)] + [(0, 3 if spec else 2)], [(f, d) for f, d, _ in mine]
        for b, auto in enumerate(autos):
            if spec:
                rows = torch.cat([s["logits"][b], s["bonus"][b][None]], 0)          # [K + 1, V]
                n, tok = int(s["seq_len"][b]) - P, s["tok"][b].tolist()
                assert len(tok) == Kd
            else:
                rows, n, tok = s["logits"][b].reshape(1, -1), min(step, len(gen[b])), []   # stage 0: one token per step until the row ends
            final = mine[-1][2][b].reshape(rows.shape[0], -1)                       # the target's rows (stage 0: the one row) behind the call
            if auto is None:
                assert extra is not None or not (torch.isneginf(rows).any() or final.any() or any(m[b].any() for _, _, m in mine[:-1])), (step, b)
                continue
            state = auto.run(gen[b][:n])
            for j in range(rows.shape[0]):
                gone = ~auto.allowed(state)
                if extra is not None:
                    gone |= extra(b)
                assert np.array_equal(torch.isneginf(rows[j]).numpy(), gone), (step, b, j)
                assert np.array_equal(final[j], gone), (step, b, j)
                n_checked += 1
                if j < len(tok):
                    assert np.array_equal(mine[j][2][b], gone), (step, b, j, "the draft proposal's logits")
                    n_checked += 1
                    assert auto.to(state, tok[j]) >= 0, (step, b, j, tok)
                    state = auto.to(state, tok[j])
    return n_checked


def scenario_kept_steps(stage):
    """Scenario 3.  Seeded and sampled, one list per prompt with an unguided row: every kept step under check_kept_masks, the
    draft proposals' logits included."""
    V = stage.shape.vocab
    rows = [CHOICES, OTHER_CHOICES, None, CHOICES, OTHER_CHOICES]
    (texts, _, stats), calls = run_kept_recorded(stage, prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS,
                                                 stop_token_ids=[STOP], guided_choice_per_prompt=rows)
    check_choice_rows(texts, stats, rows)
    autos = [None if c is None else RefAutomaton.of_choices(c, [STOP], V) for c in rows]
    n = check_kept_masks(stage, texts, autos, PROMPTS, calls)
    assert n >= 4 * 3 * (2 if stage.draft is not None else 1), n
    return texts


def scenario_logprobs(stage, lp_bar):
    """Scenario 4.  The returned log-probs against an f64 log-softmax over the allowed set of the replayed state, teacher-forced:
    tests/teacher_forced_ref.py's dense f64 forward, its processors and its bound 2 inv_t a eps_x + lp_bar, unchanged.  The
    automaton has free positions (`other`), so the restricted distribution is not a point mass.  top_p = 1: nothing truncates,
    so no position is ambiguous."""
    V = stage.shape.vocab
    fsm, auto = free_fsm(V, [STOP])
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, stop_token_ids=[STOP], top_p=1.0)
    out = stage.generate(guided_fsm=fsm, **kw)
    texts, lps, stats = out
    rows = TF.resolve(stage, kw)
    gens = [text_ids(t) for t in texts]
    TF.check_ends(rows, gens, stats)
    x, eps_x, _, prompts = TF.dense_logits(stage, kw["prompts"], gens)
    worst = bound = 0.0
    for b, (row, gen) in enumerate(zip(rows, gens)):
        assert (gen[0], gen[3:]) == (A, [C, STOP]) and len(gen) == 5, (b, gen)
        bound = 2.0 * row["inv_t"] * eps_x + lp_bar
        state = auto.start
        for i, tok in enumerate(gen):
            y = TF.processed(x[b, i], row, prompts[b], gen, i)
            y[~auto.allowed(state)] = TF.NEG_INF
            z = y * row["inv_t"]
            err = abs(float(lps[b][i]) - TF._lp_at(z, tok, -np.inf))
            worst = max(worst, err)
            state = auto.run([tok], state)
    print(f"[fsm teacher-forced] {stage.name}: eps_x {eps_x:.3e}  bound {bound:.3e}  worst |lp - f64| {worst:.3e}")
    assert worst <= bound, (worst, bound)
    return worst


A, B_TOK, C = 40, 41, 43


def free_fsm(V, Z):
    """A -> one free token (B_TOK forbidden by an edge to -1) -> a second free token -> C -> accepting: a general TokenFSM with
    `other` states, and its dict reference."""
    from asd_amd.serving.guided import TokenFSM
    edges = [{A: 1}, {B_TOK: -1}, {}, {C: 4}, {}]
    other = [-1, 2, 3, -1, -1]
    return TokenFSM(5, 0, edges, other, accepting=[4]), RefAutomaton(5, 0, edges, other, [4], Z, V)


def scenario_composition(stage):
    """Scenario 5.  Greedy; allow-list + bias + penalties + bad words + logprobs = 2 + a general TokenFSM with `other` states:
    A, two free tokens from what the list, the bans and the words leave, C, the stop id.  The bad word (A, f1) of the run
    without words changes the first free token; top-N entries are finite only where state, list and words allow."""
    V = stage.shape.vocab
    allowed = sorted(set(allow_list(V, 40, 4)) | {A, B_TOK, C, STOP})
    fsm, auto = free_fsm(V, [STOP])
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0, allowed_token_ids=allowed, logit_bias={allowed[7]: 1.0},
              repetition_penalty=1.3, frequency_penalty=1.5, logprobs=2, stop_token_ids=[STOP], guided_fsm=fsm)
    base = [text_ids(t) for t in stage.generate(**kw)[0]]
    words = [[(A, g[1])] for g in base]
    texts, lps, stats = run_kept(stage, bad_words_per_prompt=words, **kw)
    for b, g in enumerate(map(text_ids, texts)):
        assert len(g) == 5 and (g[0], g[3], g[4]) == (A, C, STOP) and stats["finish_reasons"][b] == "stop", (b, g)
        assert g[1] != base[b][1] and g[1] in set(allowed) - {STOP, B_TOK} and g[2] in set(allowed) - {STOP}, (b, g, base[b])
        ids, top = stats["top_token_ids"][b], stats["top_logprobs"][b]
        state = auto.start
        for i, t in enumerate(g):
            ok = auto.allowed(state)
            for v, lp in zip(ids[i].tolist(), top[i].tolist()):
                assert not np.isfinite(lp) or (ok[v] and v in allowed and not (i == 1 and v == words[b][0][1])), (b, i, v)
            assert ids[i][0] == t and abs(float(lps[b][i]) - float(top[i][0])) <= PAIR_ATOL, (b, i)
            state = auto.run([t], state)
    # the kept steps (greedy: every record carries seq_len): the first row of a step is -inf wherever the state behind the row's
    # committed tokens or the list removes a token, and beyond that at most at the one id a word bans there
    outside = np.ones(V, dtype=bool)
    outside[allowed] = False
    P = stage.encode_prompts(PROMPTS).shape[1]
    assert stage.step_inputs
    for s in map(_cpu, stage.step_inputs):
        for b in range(len(PROMPTS)):
            neg = torch.isneginf(s["logits"][b].reshape(-1, V)[0]).numpy()
            gone = ~auto.allowed(auto.run(text_ids(texts[b])[:int(s["seq_len"][b]) - P])) | outside
            assert neg[gone].all() and int((neg & ~gone).sum()) <= 1, b
    return texts


class CallLog:
    """Stands between a stage and the named ops and notes the order of their calls; works on the twin and on HipOps alike."""
    NAMES = ("pack_fsm", "fsm_mask_rows", "fsm_advance", "fsm_commit", "logit_mask_rows", "bad_words_rows", "logit_edit_rows", "penalty_commit")

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


def scenario_call_trace(stage):
    """Scenario 6.  One pack_fsm; per speculative step draft_len + 1 fsm_mask_rows, draft_len fsm_advance and one fsm_commit, per
    plain step 1, 0 and 1; every fsm_mask_rows directly behind the allow-list's call and in front of the bad words'; fsm_commit
    behind penalty_commit; with no guided keyword none of the four names appears."""
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, stop_token_ids=[STOP], frequency_penalty=0.5,
              allowed_token_ids=list(range(0, stage.shape.vocab)), bad_words=[(600, 601)], logit_bias={5: 1.0})
    log = CallLog(stage.ops)
    try:
        stage.generate(guided_choice=CHOICES, **kw)
        names, steps = list(log.names), stage.last_steps
        del log.names[:]
        for quiet_kw in (dict(), dict(guided_fsm=None, guided_choice=None), dict(guided_choice_per_prompt=[None, [], None, [], None])):
            stage.generate(**quiet_kw, **kw)
        quiet = list(log.names)
    finally:
        log.close()
    spec = stage.draft is not None
    assert names.count("pack_fsm") == 1 and names.index("pack_fsm") < names.index("fsm_mask_rows")
    assert names.count("fsm_mask_rows") == steps * (DRAFT_LEN + 1 if spec else 1) == names.count("logit_mask_rows")
    assert names.count("fsm_advance") == (steps * DRAFT_LEN if spec else 0) and names.count("fsm_commit") == steps
    for i, n in enumerate(names):
        if n == "fsm_mask_rows":
            assert (names[i - 1], names[i + 1], names[i + 2]) == ("logit_mask_rows", "bad_words_rows", "logit_edit_rows"), names[i - 1:i + 3]
        if n == "fsm_commit":
            assert names[i - 1] == "penalty_commit", names[i - 2:i + 1]
    assert quiet and not [n for n in quiet if "fsm" in n]
    return names


__all__ = ["CHOICES", "FsmOracleOps", "MaskRecorder", "OTHER_CHOICES", "RefAutomaton", "run_kept_recorded", "STOP", "check_choice_rows", "check_kept_masks", "free_fsm",
           "ref_delta", "ref_fsm_advance", "ref_fsm_commit", "ref_fsm_mask", "ref_state_bits", "scenario_call_trace", "scenario_choices",
           "scenario_composition", "scenario_kept_steps", "scenario_logprobs", "scenario_rows_independent", "tables_of"]
