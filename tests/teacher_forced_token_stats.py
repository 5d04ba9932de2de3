"""What generate(token_stats=True) RETURNS against the f64 teacher-forced reference, from the returned text alone: builds on
tests/teacher_forced_ref.py (resolve / dense_logits / processed / _lse / _check_table, imported, not modified).  Shared by
tests/test_teacher_forced_token_stats.py (the oracle twin) and tests/test_gpu_teacher_forced_token_stats.py (HipOps), both on
the float32 tiny stages.

At generated position i of row b: y = processed(...) (f64 logits behind the row's processors), z = y * inv_t, p = softmax(z).
With a = max(1, rep, 1 / rep) and d = inv_t * a * eps_x (a scaled logit's move between the stage's model and the f64 model, as
in that module):
  entropy   |returned - H(z)| <= 2 d sum_v p_v |z_v - mu| + bar_H, mu = sum p z: dH/dz_v = -p_v (z_v - mu), so logit moves of
            at most d change H by at most d sum p |z - mu| to first order; the factor 2 is that module's headroom.  d <= 1e-3
            is asserted, so that the second-order term (of order d^2) stays below the headroom.
  arg-max   a one-slot table under _check_table: the id exact wherever the reference's top gap exceeds 2 a eps_x, else inside
            the run; the log-prob within 2 d + lp_bar of the listed id's.
  rank      in [1 + #{y_v > y_tok + 2 a eps_x}, #{y_v >= y_tok - 2 a eps_x}] (the token itself is counted by >=).
Every position is checked; at most 5 % of a scenario's rank windows may be wider than one value, which depends on the f64
reference alone (the seeds below were chosen on the CPU so that it holds).

TEST INFRASTRUCTURE: never importable from the package."""
import numpy as np

from tests.logit_edit_ref import SEEDS
from tests.stage_scenario import MAX_TOKENS, PROMPTS, TEMPERATURE, text_ids
from tests.teacher_forced_ref import TeacherForcedError, _check_table, _lse, dense_logits, processed, resolve
from tests.teacher_forced_scenarios import CHOICES, OTHER_CHOICES, STOP, label

WIDE_CAP = 0.05
KW = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, token_stats=True)


def scenarios(V):
    allowed = [t for t in range(V) if t % 4 != 1]
    return {
        "plain": dict(KW),
        "top_k_top_p": dict(KW, top_k=20, top_p=0.9),
        "greedy": dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.0, token_stats=True),
        "temperatures": dict(KW, temperature=[0.7, 1.0, 0.5, 1.3, 0.7]),
        "edited": dict(KW, allowed_token_ids=allowed, logit_bias={allowed[5]: 4.0}, repetition_penalty=1.3, frequency_penalty=0.5,
                       presence_penalty=0.2),
        "guided_choice": dict(KW, stop_token_ids=[STOP], guided_choice_per_prompt=[CHOICES, None, None, OTHER_CHOICES, None]),
    }


def _fail(msg):
    raise TeacherForcedError(msg)


def check_token_stats(stage, kw, out, lp_bar, h_bar, label=""):
    """stage.generate(**kw) returned `out`: token_entropy, token_max_logprobs, token_argmax_ids and token_ranks of every returned
    token against the f64 teacher-forced reference.  h_bar(H) -> the entropy's own bar.  Raises TeacherForcedError; -> the figures."""
    texts, _, stats = out
    rows = resolve(stage, kw)
    gens = [text_ids(t) for t in texts]
    x, eps_x, P, prompts = dense_logits(stage, kw["prompts"], gens)
    rep = dict(eps_x=eps_x, positions=0, wide=0, worst_h=0.0, bound_h=0.0, worst_top=0.0, swaps=0, max_rank=0)
    for b, (row, gen) in enumerate(zip(rows, gens)):
        a = max(1.0, row["rep"], 1.0 / row["rep"])
        d = row["inv_t"] * a * eps_x
        if not d <= 1e-3:
            _fail(f"{label} row {b}: d = {d:.3e} is too large for the first-order entropy bound")
        for key, dtype in (("token_entropy", np.float32), ("token_max_logprobs", np.float32), ("token_argmax_ids", np.int32),
                           ("token_ranks", np.int32)):
            if stats[key][b].shape != (len(gen),) or stats[key][b].dtype != dtype:
                _fail(f"{label} row {b}: {key} is {stats[key][b].shape} {stats[key][b].dtype} for {len(gen)} tokens")
        table = dict(top_token_ids=[stats["token_argmax_ids"][b][:, None]], top_logprobs=[stats["token_max_logprobs"][b][:, None]])
        for i, tok in enumerate(gen):
            y = processed(x[b, i], row, prompts[b], gen, i)
            z = y * row["inv_t"]
            fin = np.isfinite(z)
            logp = z[fin] - _lse(z)
            p = np.exp(logp)
            H = float(-(p * logp).sum())
            mu = float((p * z[fin]).sum())
            bound = 2.0 * d * float((p * np.abs(z[fin] - mu)).sum()) + h_bar(H)
            err = abs(float(stats["token_entropy"][b][i]) - H)
            if not err <= bound:
                _fail(f"{label} row {b} position {i}: entropy {float(stats['token_entropy'][b][i])!r}, f64 teacher-forced {H!r}, "
                      f"|diff| {err:.3e} > bound {bound:.3e} (eps_x {eps_x:.3e})")
            rep["worst_h"], rep["bound_h"] = max(rep["worst_h"], err), max(rep["bound_h"], bound)
            _check_table(table, 0, i, z, y, dict(n_top=1), a, eps_x, 2.0 * d + lp_bar, rep, f"{label} arg-max of row {b}:")
            lo = 1 + int(np.count_nonzero(y > y[tok] + 2 * a * eps_x))
            hi = int(np.count_nonzero(y >= y[tok] - 2 * a * eps_x))
            rank = int(stats["token_ranks"][b][i])
            if not lo <= rank <= hi:
                _fail(f"{label} row {b} position {i} token {tok}: rank {rank}, the f64 window is [{lo}, {hi}]")
            if row["greedy"] and hi == lo and rank != 1:
                _fail(f"{label} row {b} position {i}: a greedy token of rank {rank}")
            rep["positions"] += 1
            rep["wide"] += hi > lo
            rep["max_rank"] = max(rep["max_rank"], rank)
    print(f"[teacher-forced token stats] {label}: eps_x {eps_x:.3e}  worst |H - f64| {rep['worst_h']:.3e} (largest bound "
          f"{rep['bound_h']:.3e})  worst |max lp - f64| {rep['worst_top']:.3e} ({rep['swaps']} swaps)  rank windows wider than one "
          f"value {rep['wide']}/{rep['positions']}  largest rank {rep['max_rank']}")
    if rep["wide"] > WIDE_CAP * rep["positions"]:
        _fail(f"{label}: {rep['wide']} of {rep['positions']} rank windows are wider than one value")
    return rep


def run_scenario(stage, which, lp_bar, h_bar):
    kw = scenarios(stage.shape.vocab)[which]
    out = stage.generate(**kw)
    rep = check_token_stats(stage, kw, out, lp_bar, h_bar, label(stage, "token stats, " + which))
    assert rep["positions"] == sum(out[2]["n_tokens"]) > 0
    if which == "guided_choice":
        assert out[2]["finish_reasons"][0] == out[2]["finish_reasons"][3] == "stop"
    if which == "plain":
        assert rep["max_rank"] > 1                                       # sampled tokens are not all the arg-max
    return out, rep
