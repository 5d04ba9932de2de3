"""Teacher-forced f64 check of what Stage.generate RETURNS (serving/stages.py; generate's docstring: `logprobs[i]` is the
log-prob of every committed token under this stage's processed, truncated, renormalised distribution given the prompt and the
tokens before it).  That sentence mentions no steps, proposals, n_prev or draft_len, so it is checked here from the returned
text alone: a dense f64 forward of a copy of the stage's model over prompt + returned tokens, the processors and the truncation
written again in f64 from the docstrings, and a bound that comes from the reference side only.

Nothing here reads Stage.step_inputs, Stage.prompt_inputs, a recorder or an ops trace, and none of the kernels' references
(ref_penalty, ref_logit_edit, ref_bad_words, the mask reference, fsm_ref, ngram_ref, prompt_logprobs_ref) is called: they mirror
the kernels' argument conventions, which is what a plumbing defect would share with the loop.

GUIDED ROWS, N-GRAM BANS, PROMPT LOG-PROBS.  The processors are allow-list -> the automaton's state -> bad words -> n-gram -> bias
/ bans / min_tokens -> penalties.  A guided row's automaton (`Automaton`: a dict walk over the caller's TokenFSM, or the trie of
its choices) is advanced by the RETURNED tokens alone -- no state column, no proposal -- and the n-gram history is the row's real
prompt ids followed by the returned tokens in front of the position.  A token the state forbids, or one that completes a repeated
n-gram, fails as "removed by the row's processors"; a ban computed from another history that still prevents repeats returns the
log-probs of another restricted distribution and fails the bound.  Whether a scenario's bans are LIVE is measured here too, from
the reference alone: a position counts when its ban set removes more probability mass than the position's bound, the mass taken
in f64 under the distribution without the ban.  generate(prompt_logprobs=N) is checked by check_prompt against the same dense f64
forward's rows for the prompt positions: raw logits, temperature 1, every entry, ranks inside a window of the reference's own.

THE BOUND.  eps_x = 4 * max |dense_dtype - dense_f64|, where dense_dtype is the lock-step `forward` of the stage's own model in
its own dtype on its own device over the same ids: the dtype's arithmetic noise with no ragged pass involved.  The loop's passes
are the same modules at other GEMM shapes (T = 1, 2, K + 1); each deviates from exact by the same class of error, so loop against
dense is at most twice it, and the other factor of 2 is headroom -- a plumbing defect moves logits by 0.1 to 10.  A logit error e
becomes at most a * e behind the penalties, a = max(1, rep, 1 / rep), and a log-prob (one logit minus a log-sum-exp of logits
times inv_t) moves by at most 2 * inv_t * a * e.  So |returned - f64| <= 2 * inv_t * a * eps_x + lp_bar, with lp_bar the
project's bar for a kernel log-prob against f64 at its own row (2e-5 on HipOps, 1e-6 on the CPU twin).

TRUNCATION BOUNDARIES.  No position is left out.  With d = inv_t * a * eps_x (a logit's move in scaled units; two logits move
against each other by 2 d) a position is AMBIGUOUS when a boundary of the f64 row could flip:
  top-k   the k-th and the (k+1)-th largest value are at most 2 d apart;
  top-p   with S the upper mass of a set, logit(S) = ln S - ln(1 - S) moves by at most 2 d (numerator and denominator each by a
          factor e^{+-d}): ambiguous when logit(S) of the nucleus, or of the nucleus without its last value, lies within 2 d of
          logit(top_p); or when the last value of the nucleus and the first one outside are at most 2 d apart (they may swap);
  min-p   z - z_max moves by at most 2 d: ambiguous when the last kept or the first dropped value lies within 2 d of
          z_max + ln(min_p).
At an ambiguous position the returned log-prob may match the nucleus one distinct logit value larger or smaller instead; at every
other position the kept set is the reference's.  At most 5 % of a scenario's positions may be ambiguous (asserted); without
truncation none is.

TEST INFRASTRUCTURE, like tests/penalty_ref.py: never importable from the package."""
import copy
from collections import Counter

import numpy as np
import torch

from tests.stage_scenario import text_ids

AMBIGUOUS_CAP = 0.05
GREEDY_KEEP = 0.95
NEG_INF = float("-inf")


class TeacherForcedError(AssertionError):
    """The check's own failure: the returned text, log-probs, tables or ends contradict the f64 teacher-forced reference."""


def _fail(msg):
    raise TeacherForcedError(msg)


# ------------------------------------------------------------------------------------------ the call's values, per row
def _is_seq(v):
    return isinstance(v, (list, tuple))


def _rows(value, n, default):
    """One value for the call, one per prompt, or None = the default -> n values."""
    value = default if value is None else value
    return list(value) if _is_seq(value) else [value] * n


def _lists(value, n):
    """None, one flat sequence of ids for every prompt, or one sequence (or None) per prompt -> n tuples or Nones."""
    if value is None:
        return [None] * n
    if any(_is_seq(v) or v is None for v in value):
        assert len(value) == n
        return [None if v is None else tuple(int(t) for t in v) for v in value]
    return [tuple(int(t) for t in value)] * n


def _words(entries):
    out = []
    for w in entries or ():
        assert not isinstance(w, str), "the reference takes token-id sequences only"
        if tuple(int(t) for t in w) not in out:
            out.append(tuple(int(t) for t in w))
    return out


class Automaton:
    """generate's guided row on dicts, from the docstrings: `edges[s]` = {token: next state, -1 = forbidden}, `other[s]` = the
    next state of every token without an edge (-1 = forbidden), `accepting`, and Z, the row's stop ids and one-token stop
    sequences.  The state END allows exactly Z and loops; in an accepting state every z of Z without an explicit edge is allowed
    and leads to END (it ends the row); in a non-accepting state every such z is forbidden, even under `other`."""

    def __init__(self, start, edges, other, accepting, Z, V):
        self.start, self.edges, self.other, self.accepting = int(start), [dict(e) for e in edges], list(other), set(accepting)
        self.Z, self.V, self.END = set(int(z) for z in Z), int(V), len(self.edges)

    @classmethod
    def of_fsm(cls, fsm, Z, V):
        return cls(fsm.start, fsm.edges, fsm.other, fsm.accepting, Z, V)

    @classmethod
    def of_choices(cls, choices, Z, V):
        """The trie of the choices: a choice's end node is accepting, an inner node too when a choice is a prefix of another."""
        edges, accepting = [{}], set()
        for c in choices:
            s = 0
            for t in c:
                if t not in edges[s]:
                    edges[s][t] = len(edges)
                    edges.append({})
                s = edges[s][t]
            accepting.add(s)
        return cls(0, edges, [-1] * len(edges), accepting, Z, V)

    def step(self, s, t):
        """The state behind token t in state s, or -1: t is forbidden there."""
        if s == self.END:
            return self.END if t in self.Z else -1
        if t in self.edges[s]:
            return self.edges[s][t]
        if t in self.Z:
            return self.END if s in self.accepting else -1
        return self.other[s]

    def allowed(self, s):
        """bool [V]: the tokens state s allows."""
        keep = np.full(self.V, s != self.END and self.other[s] >= 0)
        for t in (set() if s == self.END else set(self.edges[s])) | self.Z:
            keep[t] = self.step(s, t) >= 0
        return keep

    def state_behind(self, tokens):
        """The state the returned tokens lead to, or -1 behind a token that is forbidden where it stands."""
        s = self.start
        for t in tokens:
            s = self.step(s, int(t))
            if s < 0:
                return -1
        return s


def resolve(stage, kw):
    """generate's keyword arguments -> one dict per row, by the rules of generate's docstring: the call's value, the per-row
    list's, or the StageConfig default; stage 0 truncates with top_k / top_p / min_p, a verifying stage with target_*.  `ngram`:
    the row's no_repeat_ngram_size; `fsm`: the row's Automaton (from its TokenFSM, or the trie of its choices, kept in `choices`)
    or None; `n_prompt`: the call's prompt_logprobs N, None when off."""
    cfg, n = stage.config, len(kw["prompts"])
    own = (cfg.top_k, cfg.top_p, cfg.min_p) if stage.draft is None else (cfg.target_top_k, cfg.target_top_p, cfg.target_min_p)
    temp = _rows(kw.get("temperature", 0.7), n, None)
    top_k, top_p, min_p = (_rows(kw.get(k), n, d) for k, d in zip(("top_k", "top_p", "min_p"), own))
    limits = _rows(kw.get("max_tokens", 512), n, None)
    stop = tuple(int(t) for t in (cfg.stop_token_ids if kw.get("stop_token_ids") is None else kw["stop_token_ids"]))
    common = _words(cfg.stop_sequences if kw.get("stop_sequences") is None else kw["stop_sequences"])
    per = kw.get("stop_sequences_per_prompt") or [[] for _ in range(n)]
    bias = kw.get("logit_bias", None)
    bias = cfg.logit_bias if bias is None else bias
    bias = [dict(b or {}) for b in bias] if _is_seq(bias) else [dict(bias or {})] * n
    banned = _lists(cfg.banned_token_ids if kw.get("banned_token_ids") is None else kw["banned_token_ids"], n)
    allowed = _lists(cfg.allowed_token_ids if kw.get("allowed_token_ids") is None else kw["allowed_token_ids"], n)
    min_tokens = _rows(kw.get("min_tokens"), n, cfg.min_tokens)
    rep, pres, freq = (_rows(kw.get(k), n, getattr(cfg, k)) for k in ("repetition_penalty", "presence_penalty", "frequency_penalty"))
    bad_common = _words(cfg.bad_words if kw.get("bad_words") is None else kw["bad_words"])
    bad_per = kw.get("bad_words_per_prompt") or [[] for _ in range(n)]
    n_top = int(cfg.logprobs if kw.get("logprobs") is None else kw["logprobs"])
    ngram = _rows(kw.get("no_repeat_ngram_size"), n, cfg.no_repeat_ngram_size)
    n_prompt = cfg.prompt_logprobs if kw.get("prompt_logprobs") is None else kw["prompt_logprobs"]
    fsms = cfg.guided_fsm if kw.get("guided_fsm") is None else kw["guided_fsm"]
    fsms = list(fsms) if _is_seq(fsms) else [fsms] * n
    common_choice = cfg.guided_choice if kw.get("guided_choice") is None else kw["guided_choice"]
    choice = [_words(c) or None for c in (kw.get("guided_choice_per_prompt") or [None] * n)]
    choice = [c or (_words(common_choice) or None) for c in choice]
    rows = []
    for b in range(n):
        greedy = float(temp[b]) == 0.0
        V = stage.shape.vocab
        row_stops = _words([(t,) for t in stop] + common + _words(per[b]))
        Z = [s[0] for s in row_stops if len(s) == 1]
        assert fsms[b] is None or choice[b] is None
        auto = Automaton.of_fsm(fsms[b], Z, V) if fsms[b] is not None else Automaton.of_choices(choice[b], Z, V) if choice[b] else None
        rows.append(dict(
            greedy=greedy, inv_t=1.0 if greedy else float(np.float32(1.0 / float(temp[b]))),
            top_k=0 if greedy or not 0 < int(top_k[b]) < V else int(top_k[b]),
            top_p=1.0 if greedy or not 0.0 < float(top_p[b]) < 1.0 else float(top_p[b]),
            min_p=0.0 if greedy else float(min_p[b]), limit=int(limits[b]),
            stops=row_stops, bias=bias[b], banned=set(banned[b] or ()),
            allowed=None if allowed[b] is None else sorted(set(allowed[b])), min_tokens=int(min_tokens[b]),
            rep=float(rep[b]), pres=float(pres[b]), freq=float(freq[b]), bad=_words(bad_common + _words(bad_per[b])), n_top=n_top,
            ngram=int(ngram[b]), fsm=auto, choices=choice[b], n_prompt=None if n_prompt is None else int(n_prompt)))
    return rows


# ------------------------------------------------------------------------------------------ the logits
def dense_logits(stage, prompts, gens, with_prompt=False):
    """-> (x [B, N, V] f64: row (b, i) is the f64 model's logits for generated position i of row b given the padded prompt and
    gens[b][:i]; eps_x; P; every row's unpadded prompt ids).  One lock-step forward of a .double() copy of the stage's model on
    the CPU over the padded prompts followed by each row's tokens (right padding of a shorter row is harmless: attention is
    causal), and one of the stage's own model in its own dtype on its own device for eps_x, the maximum over the WHOLE sequence.
    with_prompt: a fifth value, xp [B, P - 1, V] f64 -- row (b, t) is the same forward's logits at padded prompt position t,
    which scores the prompt token at position t + 1."""
    ids, real = stage._encode(prompts)
    B, P = ids.shape
    N = max(len(g) for g in gens)
    full = torch.zeros((B, P + N), dtype=torch.int64)
    full[:, :P] = ids.cpu()
    for b, g in enumerate(gens):
        full[b, P:P + len(g)] = torch.tensor(g, dtype=torch.int64)
    m = stage.model
    m.reset()
    own = m.forward(full.to(ids.device)).double().cpu()
    m.reset()
    m64 = copy.deepcopy(m).to("cpu").double()
    m64.reset()
    with torch.no_grad():
        x = m64.forward(full)                            # (forward multiplies by logit_scale)
    assert x.dtype == torch.float64
    eps_x = 4.0 * float((own - x).abs().max())
    out = (x[:, P - 1:P - 1 + N].numpy(), eps_x, P, real)
    return out + (x[:, :P - 1].numpy(),) if with_prompt else out


# ------------------------------------------------------------------------------------------ the processors, in f64
def ngram_bans(row, prompt, gen, i):
    """The ids no_repeat_ngram_size = n removes at generated position i: with H = (the row's real prompt ids) ++ gen[:i], every
    H[j + n - 1] with j in [0, len(H) - n] and H[j : j + n - 1] == H[len(H) - n + 1 :].  n = 1: every token of H; len(H) < n:
    none.  The left-padding is not history."""
    n, H = row["ngram"], list(prompt) + list(gen[:i])
    if n < 1 or len(H) < n:
        return set()
    tail = H[len(H) - n + 1:]
    return {H[j + n - 1] for j in range(len(H) - n + 1) if H[j:j + n - 1] == tail}


def processed(x, row, prompt, gen, i, ban_ngrams=True):
    """The f64 logits of one position behind allow-list -> the automaton's state -> bad words -> n-gram -> bias / bans /
    min_tokens -> penalties (no temperature yet).  History: the row's unpadded prompt ids and gen[:i]; bad words match over the
    generated tokens only; the automaton's state is the one behind gen[:i], advanced by the returned tokens alone.
    ban_ngrams = False leaves the n-gram rule out: the distribution against which its bans' mass is measured."""
    y = np.array(x, dtype=np.float64, copy=True)
    V = y.size
    if row["allowed"] is not None:                       # 1. allow-list
        keep = np.zeros(V, dtype=bool)
        keep[row["allowed"]] = True
        y[~keep] = NEG_INF
    if row["fsm"] is not None:                           # 1b. the state's allowed set (nothing, behind a forbidden token)
        s = row["fsm"].state_behind(gen[:i])
        y[~row["fsm"].allowed(s) if s >= 0 else np.ones(V, dtype=bool)] = NEG_INF
    H = list(gen[:i])
    for w in row["bad"]:                                 # 2. bad words: the generated tokens end in the word's other tokens
        m = len(w)
        if len(H) >= m - 1 and tuple(H[len(H) - (m - 1):]) == tuple(w[:-1]):
            y[w[-1]] = NEG_INF
    if ban_ngrams:                                       # 2b. no repeated n-gram: the prompt's real ids count, the padding does not
        for t in ngram_bans(row, prompt, gen, i):
            y[t] = NEG_INF
    for t, v in row["bias"].items():                     # 3. bias (raw logit units), then the bans, which win
        y[int(t)] += float(v)
    for t in row["banned"]:
        y[t] = NEG_INF
    if i < row["min_tokens"]:
        for s in row["stops"]:
            if len(s) == 1:
                y[s[0]] = NEG_INF
    rep, pres, freq = row["rep"], row["pres"], row["freq"]
    if rep != 1.0 or pres != 0.0 or freq != 0.0:         # 4. penalties: seen = prompt + generated; counts = generated only
        seen = np.zeros(V, dtype=bool)
        seen[list(prompt) + H] = True
        c = np.bincount(np.asarray(H, dtype=np.int64), minlength=V).astype(np.float64)
        fin = np.isfinite(y)
        if rep != 1.0:
            y = np.where(seen & fin, np.where(y > 0, y / rep, y * rep), y)
        y = np.where((c > 0) & fin, y - freq * c - pres, y)
    return y


def _lse(z):
    z = z[np.isfinite(z)]
    m = z.max()
    return float(m + np.log(np.exp(z - m).sum()))


def _logit(s):
    s = min(max(float(s), 0.0), 1.0)
    with np.errstate(divide="ignore"):
        return float(np.log(s) - np.log1p(-s)) if s < 1.0 else float("inf")


def nucleus(z, top_k, top_p, min_p, d):
    """z: one row's scaled logits (f64, -inf where removed).  -> (vals: the distinct finite values, descending; m: the kept set
    is { z >= vals[m] }; ambiguous).  Temperature -> TopK -> TopP -> MinP with the set definitions of include/asd_hip.h: every
    tie at a threshold is kept; top-p is the largest value whose upper mass, renormalised over the top-k set, reaches top_p;
    min-p keeps z >= z_max + ln(min_p).  `ambiguous`: the module docstring's criteria at scale d."""
    fin = z[np.isfinite(z)]
    vals, counts = (v[::-1] for v in np.unique(fin, return_counts=True))
    m, amb = len(vals) - 1, False
    if 0 < top_k < z.size and top_k <= fin.size:
        s = np.sort(fin)[::-1]
        m = int(np.searchsorted(-vals, -s[top_k - 1]))
        if top_k < fin.size:
            amb |= bool(s[top_k - 1] - s[top_k] <= 2 * d)
    if 0.0 < top_p < 1.0:
        inside = vals[:m + 1]
        mass = np.exp(inside - vals[0]) * counts[:m + 1]
        S = np.cumsum(mass) / mass.sum()
        j = int(np.argmax(S >= top_p)) if (S >= top_p).any() else len(inside) - 1
        amb |= abs(_logit(S[j]) - _logit(top_p)) <= 2 * d or (j > 0 and abs(_logit(S[j - 1]) - _logit(top_p)) <= 2 * d)
        if j + 1 < len(vals) and j < m:
            amb |= bool(vals[j] - vals[j + 1] <= 2 * d)
        m = j
    if min_p > 0.0:
        zmp = vals[0] + np.log(min_p)
        j = int(np.count_nonzero(vals >= zmp)) - 1
        j = max(j, 0)                                    # the maximum is always kept
        amb |= bool(j > 0 and vals[j] - zmp <= 2 * d) or bool(j + 1 < len(vals) and zmp - vals[j + 1] <= 2 * d)
        m = min(m, j)
    return vals, m, bool(amb)


def _lp_at(z, tok, thr):
    return float(z[tok] - _lse(z[z >= thr])) if z[tok] >= thr else NEG_INF


def top_table(z, n):
    """The n largest of log-softmax(z) over the finite entries, lowest id on ties; unfillable slots hold -1 and -inf.
    -> (ids [n], lps [n], order: every finite id, most likely first)."""
    lsm = z - _lse(z)
    order = [int(v) for v in np.lexsort((np.arange(z.size), -z)) if np.isfinite(z[v])]
    ids = np.full(n, -1, dtype=np.int64)
    lps = np.full(n, NEG_INF)
    k = min(n, len(order))
    ids[:k] = order[:k]
    lps[:k] = lsm[order[:k]]
    return ids, lps, order


# ------------------------------------------------------------------------------------------ how a row ends, from the text
def expected_end(gen, row):
    """From the generated tokens alone -> (n, reason, sequences complete at the last token).  The row ends behind the first
    position at which a stop id or one of its stop sequences is complete in the generated tokens; otherwise at its limit."""
    for i in range(len(gen)):
        done = [s for s in row["stops"] if i + 1 >= len(s) and tuple(gen[i + 1 - len(s):i + 1]) == s]
        if done:
            if i < row["min_tokens"]:
                _fail(f"a stop {done} is complete at generated position {i}, in front of min_tokens = {row['min_tokens']}")
            return i + 1, "stop", done
    return row["limit"], "length", []


def check_ends(rows, gens, stats):
    """Every row's end from its tokens.  A guided-choice row ends by "stop" holding exactly one choice followed by one stop id,
    or by "length" holding a proper prefix of some choice; a TokenFSM row ends on a stop id only in an accepting state."""
    for b, (row, gen) in enumerate(zip(rows, gens)):
        n, reason, done = expected_end(gen, row)
        if len(gen) != n or not 1 <= len(gen) <= row["limit"]:
            _fail(f"row {b} returned {len(gen)} tokens, the text ends at {n} ({reason}): {gen}")
        if row["choices"] is not None:
            g = tuple(gen)
            if reason == "stop" and not (g[:-1] in set(row["choices"]) and (g[-1],) in done):
                _fail(f"row {b} ends by stop and does not hold one choice followed by one stop id: {gen}")
            if reason == "length" and not any(len(g) < len(c) and c[:len(g)] == g for c in row["choices"]):
                _fail(f"row {b} ends by length and holds no proper prefix of a choice: {gen}")
        elif row["fsm"] is not None and reason == "stop" and any(len(s) == 1 for s in done):
            if row["fsm"].state_behind(gen[:-1]) not in row["fsm"].accepting:
                _fail(f"row {b} ends on a stop id outside an accepting state: {gen}")
        if "finish_reasons" in stats:
            if stats["finish_reasons"][b] != reason or stats["n_tokens"][b] != n:
                _fail(f"row {b}: stats say {stats['finish_reasons'][b]} at {stats['n_tokens'][b]}, the text says {reason} at {n}")
            match = stats["stop_matches"][b]
            if (reason == "length" and match is not None) or (reason == "stop" and tuple(match) not in done):
                _fail(f"row {b}: stop_matches {match}, the text ends in {done}")


# ------------------------------------------------------------------------------------------ the check
def check(stage, kw, out, lp_bar, label=""):
    """stage.generate(**kw) returned `out` = (texts, logprobs, stats): every returned log-prob, every top-N table and every
    row's end against the f64 teacher-forced reference.  Raises TeacherForcedError; -> the figures, which are printed."""
    texts, lps, stats = out
    rows = resolve(stage, kw)
    gens = [text_ids(t) for t in texts]
    B = len(gens)
    if len(lps) != B or any(len(lp) != len(g) or lp.dtype != np.float32 for lp, g in zip(lps, gens)):
        _fail("logprobs do not have one float32 per returned token")
    check_ends(rows, gens, stats)
    x, eps_x, P, prompts, xp = dense_logits(stage, kw["prompts"], gens, with_prompt=True)
    rep = dict(eps_x=eps_x, positions=0, ambiguous=0, worst=0.0, bound=0.0, worst_top=0.0, swaps=0, unclear=0,
               ngram_live=[0] * B, ngram_bans=[0] * B)
    check_prompt(stats, rows[0]["n_prompt"], xp, eps_x, P, prompts, lp_bar, rep, label)
    truncating, bad = False, []
    for b, (row, gen) in enumerate(zip(rows, gens)):
        a = max(1.0, row["rep"], 1.0 / row["rep"])
        d = row["inv_t"] * a * eps_x
        bound = 2.0 * d + lp_bar
        rep["bound"] = max(rep["bound"], bound)
        truncating |= row["top_k"] > 0 or row["top_p"] < 1.0 or row["min_p"] > 0.0
        for i, tok in enumerate(gen):
            y = processed(x[b, i], row, prompts[b], gen, i)
            z = y * row["inv_t"]
            got = float(lps[b][i])
            rep["positions"] += 1
            if not np.isfinite(y[tok]):
                _fail(f"{label} row {b} position {i}: token {tok} is removed by the row's processors")
            gone = ngram_bans(row, prompts[b], gen, i)
            if gone:                                     # liveness, from the reference alone: the mass the ban removes, measured
                free = processed(x[b, i], row, prompts[b], gen, i, ban_ngrams=False) * row["inv_t"]      # without the ban
                mass = float(np.exp(free[sorted(gone)] - _lse(free)).sum())
                rep["ngram_bans"][b] += 1
                rep["ngram_live"][b] += mass > bound
            if row["greedy"]:
                top2 = np.sort(y[np.isfinite(y)])[-2:]
                if len(top2) < 2 or top2[1] - top2[0] > 2 * a * eps_x:
                    if int(np.argmax(y)) != tok:
                        _fail(f"{label} row {b} position {i}: token {tok} is not the reference arg-max {int(np.argmax(y))} (gap {top2[-1] - top2[0]:.3e})")
                else:
                    rep["unclear"] += 1
            vals, m, amb = nucleus(z, row["top_k"], row["top_p"], row["min_p"], d)
            err = abs(got - _lp_at(z, tok, vals[m]))
            if amb:
                rep["ambiguous"] += 1
                err = min([err] + [abs(got - _lp_at(z, tok, vals[j])) for j in (m - 1, m + 1) if 0 <= j < len(vals)])
            if not err <= bound:
                bad.append((err, f"row {b} position {i} token {tok}: returned {got!r}, f64 teacher-forced {_lp_at(z, tok, vals[m])!r}, "
                                 f"|diff| {err:.3e} > bound {bound:.3e} (eps_x {eps_x:.3e}, ambiguous {amb})"))
            rep["worst"] = max(rep["worst"], err)
            if row["n_top"]:
                _check_table(stats, b, i, z, y, row, a, eps_x, bound, rep, label)
    share = rep["ambiguous"] / max(rep["positions"], 1)
    rep["share"] = share
    print(f"[teacher-forced] {label}: eps_x {eps_x:.3e}  bound {rep['bound']:.3e}  worst |lp - f64| {rep['worst']:.3e}  "
          f"worst top-N {rep['worst_top']:.3e} ({rep['swaps']} swaps)  ambiguous {rep['ambiguous']}/{rep['positions']} = {share:.3f}"
          + (f"  greedy positions inside the gap {rep['unclear']}" if rows[0]["greedy"] else "")
          + (f"  live n-gram bans per row {rep['ngram_live']} of {rep['ngram_bans']}" if any(r["ngram"] for r in rows) else "")
          + (f"  prompt: worst |lp - f64| {rep['prompt_worst']:.3e}  worst table {rep['prompt_worst_top']:.3e} "
             f"({rep['prompt_swaps']} swaps)  rank windows wider than one value {rep['prompt_wide']}/{rep['prompt_entries']}"
             if rows[0]["n_prompt"] is not None else ""))
    if bad:
        _fail(f"{label}: {len(bad)} of {rep['positions']} log-probs miss the f64 teacher-forced value; the worst: {max(bad)[1]}")
    if share > AMBIGUOUS_CAP or (not truncating and rep["ambiguous"]):
        _fail(f"{label}: {rep['ambiguous']} of {rep['positions']} positions are ambiguous")
    if rows[0]["greedy"] and rep["unclear"] > (1.0 - GREEDY_KEEP) * rep["positions"]:
        _fail(f"{label}: {rep['unclear']} of {rep['positions']} greedy positions lie inside the arg-max gap")
    return rep


PROMPT_KEYS = ("prompt_token_ids", "prompt_logprobs", "prompt_ranks", "prompt_top_token_ids", "prompt_top_logprobs")


def check_prompt(stats, n, xp, eps_x, P, real, lp_bar, rep, label):
    """generate(prompt_logprobs=n)'s five keys against the f64 model's RAW logits at temperature 1, whatever processors the call
    has.  n None: none of the keys.  Else, with m_i = (row i's real prompt tokens) - 1 and entry j of row i belonging to real
    prompt token j + 1 (scored by the logits at the padded position in front of it): prompt_token_ids are the real ids (int32
    [m_i + 1]); |log-prob - f64| <= 2 eps_x + lp_bar (the module's formula with inv_t = a = 1); the rank lies in
    [1 + #{v : x_v > x_t + 2 eps_x}, 1 + #{v != t : x_v >= x_t - 2 eps_x}] -- a window around the reference's rank, a single
    value wherever no other logit lies within 2 eps_x of the token's; every entry is checked; the tables (n >= 1) under
    _check_table on the raw row with a = 1.  The figures go into `rep`."""
    if n is None:
        if any(k in stats for k in PROMPT_KEYS):
            _fail(f"{label}: prompt_logprobs is off and stats holds {[k for k in PROMPT_KEYS if k in stats]}")
        return
    for k in PROMPT_KEYS:
        if (k in stats) != (n > 0 or not k.startswith("prompt_top")) or (k in stats and len(stats[k]) != len(real)):
            _fail(f"{label}: prompt_logprobs = {n} and stats {'holds' if k in stats else 'lacks'} {k} (or not one entry per prompt)")
    bound = 2.0 * eps_x + lp_bar
    fig = dict(worst_top=0.0, swaps=0)
    worst = wide = entries = 0
    for i, r in enumerate(real):
        m = max(len(r) - 1, 0)
        ids, lp, rank = stats["prompt_token_ids"][i], stats["prompt_logprobs"][i], stats["prompt_ranks"][i]
        if ids.dtype != np.int32 or ids.tolist() != [int(t) for t in r]:
            _fail(f"{label} row {i}: prompt_token_ids {ids.tolist()} ({ids.dtype}), the real prompt ids are {list(r)}")
        if lp.shape != (m,) or lp.dtype != np.float32 or rank.shape != (m,) or rank.dtype != np.int32:
            _fail(f"{label} row {i}: prompt_logprobs {lp.shape} {lp.dtype}, prompt_ranks {rank.shape} {rank.dtype}, m = {m}")
        table = None
        if n:
            table = dict(top_token_ids=[stats["prompt_top_token_ids"][i]], top_logprobs=[stats["prompt_top_logprobs"][i]])
            tid, tlp = table["top_token_ids"][0], table["top_logprobs"][0]
            if tid.shape != (m, n) or tid.dtype != np.int32 or tlp.shape != (m, n) or tlp.dtype != np.float32:
                _fail(f"{label} row {i}: prompt tables {tid.shape} {tid.dtype} / {tlp.shape} {tlp.dtype}, m = {m}, N = {n}")
        for j in range(m):
            row, t = xp[i, P - len(r) + j], int(r[j + 1])
            err = abs(float(lp[j]) - float(row[t] - _lse(row)))
            if not err <= bound:
                _fail(f"{label} row {i} prompt token {j + 1} ({t}): returned {float(lp[j])!r}, f64 {float(row[t] - _lse(row))!r}, "
                      f"|diff| {err:.3e} > bound {bound:.3e} (eps_x {eps_x:.3e})")
            lo = 1 + int(np.count_nonzero(row > row[t] + 2 * eps_x))
            hi = 1 + int(np.count_nonzero(row >= row[t] - 2 * eps_x)) - 1          # (the token itself is counted by >=)
            if not lo <= int(rank[j]) <= hi:
                _fail(f"{label} row {i} prompt token {j + 1} ({t}): rank {int(rank[j])}, the f64 window is [{lo}, {hi}]")
            worst, wide, entries = max(worst, err), wide + (hi > lo), entries + 1
            if n:
                _check_table(table, 0, j, row, row, dict(n_top=n), 1.0, eps_x, bound, fig, f"{label} prompt row {i}:")
    rep.update(prompt_worst=worst, prompt_worst_top=fig["worst_top"], prompt_swaps=fig["swaps"], prompt_wide=wide, prompt_entries=entries)


def _check_table(stats, b, i, z, y, row, a, eps_x, bound, rep, label):
    """Row b, position i of the top-N tables: the N largest of the processed, UNTRUNCATED, temperature-scaled log-softmax.  Ids
    exact wherever the reference's adjacent gap exceeds 2 a eps_x; elsewhere neighbours may swap -- in a run of several such
    gaps (bf16: dozens of tokens lie inside one) more than once, so a slot's id must lie in the run of the reference's id, and
    no id may cross a gap above 2 a eps_x.  Log-probs within the bound of the id that is listed."""
    n = row["n_top"]
    got_id, got_lp = stats["top_token_ids"][b][i], stats["top_logprobs"][b][i]
    if got_id.shape != (n,) or got_lp.shape != (n,):
        _fail(f"{label} row {b} position {i}: a top-N table of shape {got_id.shape}")
    ids, lps, order = top_table(z, n)
    lsm = z - _lse(z)
    # runs of the reference's order whose adjacent gaps are all <= 2 a eps_x: inside a run neighbours may swap (and swap again)
    yo = y[order]
    run_of = dict(zip(order, np.concatenate([[0], np.cumsum((yo[:-1] - yo[1:]) > 2 * a * eps_x)]).tolist()))
    if len(set(got_id.tolist()) - {-1}) != int((got_id >= 0).sum()):
        _fail(f"{label} row {b} position {i}: a top-N table that lists an id twice: {got_id.tolist()}")
    for j in range(n):
        g = int(got_id[j])
        if ids[j] < 0 or g < 0:
            if g != ids[j] or not (g >= 0 or got_lp[j] == NEG_INF):
                _fail(f"{label} row {b} position {i} slot {j}: id {g} / {got_lp[j]}, the reference has {ids[j]}")
            continue
        if g != ids[j]:
            if run_of.get(g, -1) != run_of[int(ids[j])]:
                _fail(f"{label} row {b} position {i} slot {j}: id {g}, the reference has {ids[j]} and a gap above {2 * a * eps_x:.3e} between them")
            rep["swaps"] += 1
        err = abs(float(got_lp[j]) - float(lsm[g]))
        if not err <= bound:
            _fail(f"{label} row {b} position {i} slot {j}: top-N log-prob {got_lp[j]!r}, f64 {lsm[g]!r}, |diff| {err:.3e} > {bound:.3e}")
        rep["worst_top"] = max(rep["worst_top"], err)


def run_checked(stage, lp_bar, label="", **kw):
    """generate(**kw), checked -> (out, the figures)."""
    out = stage.generate(**kw)
    return out, check(stage, kw, out, lp_bar, label or stage.name)


def recurring(gens):
    """Does some row hold a token twice?"""
    return any(max(Counter(g).values()) > 1 for g in gens if g)
