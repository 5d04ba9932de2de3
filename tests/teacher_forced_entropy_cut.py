"""What generate(typical_p= / epsilon_cutoff= / eta_cutoff=) RETURNS against the f64 teacher-forced reference, from the returned
text alone: builds on tests/teacher_forced_ref.py (resolve / dense_logits / processed / _lse / check_ends, imported, not
modified) and adds the f64 processor of the cut.  Shared by tests/test_teacher_forced_entropy_cut.py (the oracle twin) and
tests/test_gpu_teacher_forced_entropy_cut.py (HipOps), both on the float32 tiny stages.  Nothing here reads Stage.step_inputs, a
recorder or an ops trace, and ref_entropy_cut is not called: the cut is written again below, in nats, from generate's docstring.

At generated position i of row b: y = processed(...) (f64 logits behind the row's other processors), z = y * inv_t,
p = softmax(z), H its entropy.  The row's own cut -- the call's keyword, else StageConfig.typical_p / epsilon_cutoff / eta_cutoff
at stage 0 and the target_* fields at a verifying stage -- keeps a set K of tokens, and the returned log-prob must be
z_tok - lse(z over K) (the scenarios switch top-k, top-p and min-p off).

THE WINDOW (the rule of tests/entropy_cut_ref.py, at the scale of this check).  The loop's logits differ from the f64 model's by
at most a * eps_x, so scaled logits move by d = inv_t * a * eps_x (tests/teacher_forced_ref.py, THE BOUND), ln p_v by 2 d, and H
by dH = 2 d sum p |z - mu| (tests/teacher_forced_token_stats.py's first-order bound with its factor 2).  With KERNEL = 2e-5 nats
for the kernel's own f32 keys and 1e-5 for its masses (entropy cuts, at V <= 1000):
  typical   a key d_v = |-ln p_v - H| moves by at most e = 2 d + dH + KERNEL, a cumulative mass by w_m = 2 d + 1e-5 (every p_v
            by a factor e^{+-2d}).  With k_lo / k_hi the first distinct keys whose cumulative mass reaches m - w_m / m + w_m, a
            token is surely kept when d_v <= k_lo - 2 e, surely cut when d_v > k_hi + 2 e, UNDECIDED in between -- unless the
            tokens in between hold one value and k_lo = k_hi (or the mass never reaches m + w_m): then they are the threshold,
            or the last group, and are kept.
  epsilon   ln p_v against ln e: undecided within 2 d + KERNEL, and only below the maximum; a token within 2 d of the maximum
            may tie it in the loop and is undecided when it is below the bound.
  eta       the same against ln min(e, sqrt(e) exp(-H)), with dH added.
The committed token must be kept or undecided.  Every position is checked: the returned log-prob must lie within
2 d + lp_bar of the interval spanned by the kept set with every undecided token in and with every undecided token out.  At
most 5 % of a scenario's positions may hold an undecided token, which depends on the f64 reference alone.

TEST INFRASTRUCTURE: never importable from the package."""
import numpy as np

from tests.logit_edit_ref import SEEDS
from tests.stage_scenario import MAX_TOKENS, PROMPTS, TEMPERATURE, text_ids
from tests.teacher_forced_ref import TeacherForcedError, _lse, check_ends, dense_logits, processed, resolve
from tests.teacher_forced_scenarios import label

UNDECIDED_CAP = 0.05
KERNEL, KERNEL_MASS = 2e-5, 1e-5
KW = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, top_p=1.0, top_k=0, min_p=0.0)
CUT_KEYS = ("typical_p", "epsilon_cutoff", "eta_cutoff")


def scenarios():
    """name -> (the stages it runs at, generate's keywords)."""
    return {
        "typical": (("8b",), dict(KW, typical_p=0.6)),                       # stage 0
        "eta": (("13b", "34b"), dict(KW, eta_cutoff=0.02)),                  # a verifying stage: the target side's cut
        "typical_rows": (("8b",), dict(KW, typical_p=[0.5, 1.0, 0.3, 0.9, 0.2], temperature=[0.7, 1.0, 0.5, 1.3, 0.7])),
    }


def _fail(msg):
    raise TeacherForcedError(msg)


def cut_rows(stage, kw):
    """Every row's (key, value) of its OWN cut, or None: the call's keyword, else the configuration's -- StageConfig.<key> at
    stage 0, StageConfig.target_<key> at a verifying stage.  typical_p is off at 0 and 1, the other two at 0."""
    n, cfg = len(kw["prompts"]), stage.config
    rows = [None] * n
    for key in CUT_KEYS:
        v = kw.get(key)
        v = getattr(cfg, key if stage.draft is None else "target_" + key) if v is None else v
        for b, one in enumerate(list(v) if isinstance(v, (list, tuple)) else [v] * n):
            one = float(np.float32(one))
            if 0.0 < one < 1.0:
                assert rows[b] is None, "two cuts on one row"
                rows[b] = (key, one)
    return rows


def cut_sets(z, cut, d):
    """z: one position's scaled f64 logits (-inf where removed), cut = (key, value), d: a scaled logit's move.
    -> (keep, undecided), bool [V] each, by the module docstring."""
    fin = np.isfinite(z)
    logp = np.where(fin, z - _lse(z), -np.inf)
    p = np.where(fin, np.exp(logp), 0.0)
    H = -float((p[fin] * logp[fin]).sum())
    mu = float((p[fin] * z[fin]).sum())
    dH = 2.0 * d * float((p[fin] * np.abs(z[fin] - mu)).sum())
    key, value = cut
    if key == "typical_p":
        dist = np.where(fin, np.abs(-logp - H), np.inf)
        e, w_m = 2.0 * d + dH + KERNEL, 2.0 * d + KERNEL_MASS
        ids = sorted(np.nonzero(fin)[0], key=lambda v: dist[v])
        keys, cum, mass = [], [], 0.0                                       # the distinct keys, ascending, and their cumulative masses
        for v in ids:
            mass += p[v]
            if keys and dist[v] == keys[-1]:
                cum[-1] = mass
            else:
                keys.append(dist[v])
                cum.append(mass)
        first = lambda bar: next((k for k, c in zip(keys, cum) if c >= bar), np.inf)      # noqa: E731
        d_star, k_lo, k_hi = first(value), first(value - w_m), first(value + w_m)
        keep = fin & (dist <= d_star)
        sure_keep = dist <= k_lo - 2.0 * e
        sure_cut = dist > k_hi + 2.0 * e
        between = fin & ~sure_keep & ~sure_cut
        if between.any() and np.unique(z[between]).size == 1 and (k_lo == k_hi or k_hi == np.inf):
            between[:] = False               # one value alone at the boundary: it is the threshold (or the last group), and is kept
        return keep, between
    ln_thr = np.log(value)
    e = 2.0 * d + KERNEL
    if key == "eta_cutoff":
        alt = 0.5 * np.log(value) - H
        if abs(alt - ln_thr) <= dH:                                          # which term is the smaller is itself unsure
            e += abs(alt - ln_thr)
        if alt < ln_thr:
            ln_thr, e = alt, e + dH
    zmax = z[fin].max()
    below = fin & (logp < ln_thr)
    keep = fin & ~(below & (z < zmax))
    near_bound = fin & (np.abs(logp - ln_thr) <= e) & (z < zmax)
    near_max = below & (z < zmax) & (z >= zmax - 2.0 * d)
    return keep, near_bound | near_max


def check_cut(stage, kw, out, lp_bar, label="", cut_kw=None):
    """stage.generate(**kw) returned `out`: every returned token and log-prob against the f64 teacher-forced reference behind the
    f64 cut.  cut_kw: the cut keywords the CHECKER believes in (default: kw's; the negative control hands over others).  Raises
    TeacherForcedError; -> the figures."""
    texts, lps, stats = out
    rows = resolve(stage, kw)
    cuts = cut_rows(stage, dict(kw, **(cut_kw or {})))
    gens = [text_ids(t) for t in texts]
    if len(lps) != len(gens) or any(len(lp) != len(g) or lp.dtype != np.float32 for lp, g in zip(lps, gens)):
        _fail("logprobs do not have one float32 per returned token")
    check_ends(rows, gens, stats)
    x, eps_x, P, prompts = dense_logits(stage, kw["prompts"], gens)
    rep = dict(eps_x=eps_x, positions=0, undecided=0, worst=0.0, bound=0.0, cut_tokens=0, live=0)
    for b, (row, gen) in enumerate(zip(rows, gens)):
        assert row["top_k"] == 0 and row["top_p"] == 1.0 and row["min_p"] == 0.0 and not row["greedy"]
        a = max(1.0, row["rep"], 1.0 / row["rep"])
        d = row["inv_t"] * a * eps_x
        bound = 2.0 * d + lp_bar
        rep["bound"] = max(rep["bound"], bound)
        for i, tok in enumerate(gen):
            z = processed(x[b, i], row, prompts[b], gen, i) * row["inv_t"]
            fin = np.isfinite(z)
            keep, und = (fin, np.zeros(z.size, bool)) if cuts[b] is None else cut_sets(z, cuts[b], d)
            rep["positions"] += 1
            rep["undecided"] += bool(und.any())
            rep["cut_tokens"] += int((fin & ~keep).sum())
            if not (keep[tok] or und[tok]):
                _fail(f"{label} row {b} position {i}: token {tok} is removed by the row's cut {cuts[b]}")
            inside, outside = keep | und, keep & ~und
            outside[tok] = True
            lo, hi = float(z[tok] - _lse(z[inside])), float(z[tok] - _lse(z[outside]))
            got = float(lps[b][i])
            err = max(lo - got, got - hi, 0.0)
            # live: the cut moves this position's log-prob by more than the bound, measured on the reference alone
            rep["live"] += (z[tok] - _lse(z[keep])) - (z[tok] - _lse(z)) > bound
            if not err <= bound:
                _fail(f"{label} row {b} position {i} token {tok}: returned {got!r}, the f64 teacher-forced value lies in "
                      f"[{lo!r}, {hi!r}], off by {err:.3e} > bound {bound:.3e} (eps_x {eps_x:.3e}, cut {cuts[b]})")
            rep["worst"] = max(rep["worst"], err)
    print(f"[teacher-forced entropy cut] {label}: eps_x {eps_x:.3e}  bound {rep['bound']:.3e}  worst miss of the interval "
          f"{rep['worst']:.3e}  positions with an undecided token {rep['undecided']}/{rep['positions']}  tokens cut "
          f"{rep['cut_tokens']}  positions the cut moves beyond the bound {rep['live']}")
    if rep["undecided"] > UNDECIDED_CAP * rep["positions"]:
        _fail(f"{label}: {rep['undecided']} of {rep['positions']} positions hold an undecided token")
    return rep


def run_scenario(stage, which, lp_bar):
    kw = scenarios()[which][1]
    out = stage.generate(**kw)
    rep = check_cut(stage, kw, out, lp_bar, label(stage, "entropy cut, " + which))
    assert rep["positions"] == sum(out[2]["n_tokens"]) > 0
    assert rep["live"] >= rep["positions"] // 2, rep                         # the cut is live at most positions of the scenario
    return out, rep
