"""Teacher-forced f64 check of what Stage.generate RETURNS (serving/stages.py; generate's docstring: `logprobs[i]` is the
log-prob of every committed token under this stage's processed, truncated, renormalised distribution given the prompt and the
tokens before it).  That sentence mentions no steps, proposals, n_prev or draft_len, so it is checked here from the returned
text alone: a dense f64 forward of a copy of the stage's model over prompt + returned tokens, the processors and the truncation
written again in f64 from the docstrings, and a bound that comes from the reference side only.

Nothing here reads Stage.step_inputs, a recorder or an ops trace, and none of the kernels' references (ref_penalty,
ref_logit_edit, ref_bad_words, the mask reference) is called: they mirror the kernels' argument conventions, which is what a
plumbing defect would share with the loop.

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


def resolve(stage, kw):
    """generate's keyword arguments -> one dict per row, by the rules of generate's docstring: the call's value, the per-row
    list's, or the StageConfig default; stage 0 truncates with top_k / top_p / min_p, a verifying stage with target_*."""
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
    rows = []
    for b in range(n):
        greedy = float(temp[b]) == 0.0
        V = stage.shape.vocab
        rows.append(dict(
            greedy=greedy, inv_t=1.0 if greedy else float(np.float32(1.0 / float(temp[b]))),
            top_k=0 if greedy or not 0 < int(top_k[b]) < V else int(top_k[b]),
            top_p=1.0 if greedy or not 0.0 < float(top_p[b]) < 1.0 else float(top_p[b]),
            min_p=0.0 if greedy else float(min_p[b]), limit=int(limits[b]),
            stops=_words([(t,) for t in stop] + common + _words(per[b])), bias=bias[b], banned=set(banned[b] or ()),
            allowed=None if allowed[b] is None else sorted(set(allowed[b])), min_tokens=int(min_tokens[b]),
            rep=float(rep[b]), pres=float(pres[b]), freq=float(freq[b]), bad=_words(bad_common + _words(bad_per[b])), n_top=n_top))
    return rows


# ------------------------------------------------------------------------------------------ the logits
def dense_logits(stage, prompts, gens):
    """-> (x [B, N, V] f64: row (b, i) is the f64 model's logits for generated position i of row b given the padded prompt and
    gens[b][:i]; eps_x; P; every row's unpadded prompt ids).  One lock-step forward of a .double() copy of the stage's model on
    the CPU over the padded prompts followed by each row's tokens (right padding of a shorter row is harmless: attention is
    causal), and one of the stage's own model in its own dtype on its own device for eps_x."""
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
    return x[:, P - 1:P - 1 + N].numpy(), eps_x, P, real


# ------------------------------------------------------------------------------------------ the processors, in f64
def processed(x, row, prompt, gen, i):
    """The f64 logits of one position behind mask -> bad words -> bias / bans / min_tokens -> penalties (no temperature yet).
    History: the row's unpadded prompt ids and gen[:i]; bad words match over the generated tokens only."""
    y = np.array(x, dtype=np.float64, copy=True)
    V = y.size
    if row["allowed"] is not None:                       # 1. allow-list
        keep = np.zeros(V, dtype=bool)
        keep[row["allowed"]] = True
        y[~keep] = NEG_INF
    H = list(gen[:i])
    for w in row["bad"]:                                 # 2. bad words: the generated tokens end in the word's other tokens
        m = len(w)
        if len(H) >= m - 1 and tuple(H[len(H) - (m - 1):]) == tuple(w[:-1]):
            y[w[-1]] = NEG_INF
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
    for b, (row, gen) in enumerate(zip(rows, gens)):
        n, reason, done = expected_end(gen, row)
        if len(gen) != n or not 1 <= len(gen) <= row["limit"]:
            _fail(f"row {b} returned {len(gen)} tokens, the text ends at {n} ({reason}): {gen}")
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
    x, eps_x, P, prompts = dense_logits(stage, kw["prompts"], gens)
    rep = dict(eps_x=eps_x, positions=0, ambiguous=0, worst=0.0, bound=0.0, worst_top=0.0, swaps=0, unclear=0)
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
          + (f"  greedy positions inside the gap {rep['unclear']}" if rows[0]["greedy"] else ""))
    if bad:
        _fail(f"{label}: {len(bad)} of {rep['positions']} log-probs miss the f64 teacher-forced value; the worst: {max(bad)[1]}")
    if share > AMBIGUOUS_CAP or (not truncating and rep["ambiguous"]):
        _fail(f"{label}: {rep['ambiguous']} of {rep['positions']} positions are ambiguous")
    if rows[0]["greedy"] and rep["unclear"] > (1.0 - GREEDY_KEEP) * rep["positions"]:
        _fail(f"{label}: {rep['unclear']} of {rep['positions']} greedy positions lie inside the arg-max gap")
    return rep


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
