"""Entropy cuts (serving/stages.py, ENTROPY CUTS; include/asd_hip.h, asd_entropy_cut_rows): the numpy f64 reference of the
kernel, written from the header's text, the boundary window that says which decisions the kernel's f32 arithmetic may flip, the
oracle ops twin that cuts through the reference, and the stage-level scenarios that tests/test_entropy_cut_stages.py (CPU twin)
and tests/test_gpu_entropy_cut_stages.py (HipOps) both run on stage_configs(vocab=64).

THE BOUNDARY WINDOW.  The reference decides in f64; the kernel compares f32 keys and sums 2^-40 fixed-point masses.  A token
is UNDECIDED when the kernel's rounding can flip the reference's decision; only undecided tokens are excused, every other token
of every row must match exactly.  The bounds follow the kernel's arithmetic, with u = 2^-24, everything in log2 units (the
kernel's domain; the reference works in nats, so the code below multiplies by ln 2), per row:
  xs      = max |x_v| * inv_t / ln 2 over the finite elements: the size of x_v c2.
  R       = u (ceil(V / (1024 N)) + 75 + log2 V): the relative error of s (and of u).  A lane adds ceil(V / (1024 N)) + 1 vector
            sums in a chain, each term an exp2 of 1 ulp (2u) of an fma rounded once (u |d|, mass-weighted at most u ln 2 log2 V);
            6 DPP steps and a rescale follow (9u), then 16 merges in wave order of about 4u each (64u).  N = 4 (f32), 8 (16-bit).
  dL      = R / ln 2 + 1e-7: the error of L = m2 + log2 s (log2_split is good to 1e-7; m2 is exact; the two-float split of L
            loses 1e-14).
  dH      = dL + (H2 - log2 s)(2R + 2u): the error of H2 = log2 s - u / s, whose second term is a quotient of two such sums.
  a key   k_v = |fma(x_v, c2, -A.hi) - A.lo|, A = L - H2, against the exact |x_v inv_t / ln 2 - A|: c2 = fl(log2(e) inv_t) moves
            log2 p_v by at most 2u xs; the fma and the subtraction round to the key's own size, 2u k_v; A carries dL + dH.  So
            eps(k) = 2u xs + 2u k + dL + dH, and two keys compare reliably when they differ by more than eps(k) + eps(k').
  log2 p_v = fma(x_v, c2, -L.hi) - L.lo for epsilon / eta: 2u xs + 2u |log2 p_v| + dL; the bound's own logarithm adds
            1e-7 + u |log2 e|, and eta's sqrt(e) exp(-H) adds dH.
  a mass  floor(p_v 2^40) with p_v = exp2(log2 p_v): a cumulative mass is off by at most
            w_m = (V + 1) 2^-40 + 2u + ln 2 (2u xs + dL + 2u H2)
            (one floor per token and one for m; exp2's ulp; the error of log2 p_v, mass-weighted: sum p |log2 p| = H2).
TYPICAL.  With the distinct keys ascending and C their cumulative masses, k_lo is the first key with C >= m - w_m and k_hi the
first with C >= m + w_m (+inf when the mass never gets there).  The kernel's threshold lies between them, so a token is surely
kept when k_v + eps(k_v) <= k_lo - eps(k_lo), surely cut when k_v - eps(k_v) > k_hi + eps(k_hi), and undecided in between --
unless every token in between holds ONE stored value: equal bits give equal keys in the kernel, nothing below them reaches m and
all of them together pass it, so they are the threshold and are kept (a flat row, and exact ties at d*).  EPSILON / ETA: a token
below the maximum is undecided when |log2 p_v - log2 bound| is within the sum of the two errors above.
At N(0, 3^2) logits rounded to bf16, T = 0.7, V = 152064 these come to about eps = 1e-4 and w_m = 1e-5, wider than a guess of
5e-5 / 1e-6 because R is a worst-case chain bound; the tests therefore count the undecided rows of their inputs on the reference
alone and assert the cap (at most 2 % of a test's rows) before they look at the kernel.

TEST INFRASTRUCTURE, like tests/token_stats_ref.py: never importable from the package."""
from types import SimpleNamespace

import numpy as np
import torch

from tests.logit_edit_ref import SEEDS, run_kept
from tests.per_request_ref import inv_t_of
from tests.prompt_logprobs_ref import AllCalls
from tests.stage_scenario import MAX_TOKENS, PROMPTS, TEMPERATURE, text_ids
from tests.token_stats_ref import ROW_TEMPERATURES, TokenStatsOracleOps, check_stage_stats
from tests.top_logprobs_ref import step_rows

VOCAB = 64
OFF, TYPICAL, EPSILON, ETA = 0, 1, 2, 3
LN2 = float(np.log(2.0))
U = 2.0 ** -24
CAP = 0.02                                       # at most this share of a test's rows may hold an undecided token


def _lanes(dtype_bytes):
    return 4 if dtype_bytes == 4 else 8


def cut_row(row, inv_t, mode, value, dtype_bytes=4):
    """One row under one record, f64 -> SimpleNamespace(keep, thr, undecided, touched).  row: the stored values (f32, exact);
    inv_t, value: the record's f32 numbers.  keep: bool [V], the tokens that survive (True everywhere on an untouched row);
    thr: d* in nats (typical; +inf when everything is kept), or the probability bound (epsilon / eta), NaN on an untouched row;
    undecided: bool [V], the module docstring's window; touched: False for mode 0 and for a row without a distribution (a NaN
    or +inf element, or no finite element)."""
    x = np.asarray(row, dtype=np.float32).astype(np.float64)
    V = x.shape[0]
    out = SimpleNamespace(keep=np.ones(V, bool), thr=float("nan"), undecided=np.zeros(V, bool), touched=False)
    fin = np.isfinite(x)
    if mode == OFF or np.isnan(x).any() or np.isposinf(x).any() or not fin.any():
        return out
    a, val = float(np.float32(inv_t)), float(np.float32(value))
    assert a > 0.0 and 0.0 < val < 1.0 and mode in (TYPICAL, EPSILON, ETA)
    out.touched = True
    z = x * a
    zmax = z[fin].max()
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(fin, np.exp(z - zmax), 0.0)
        s = e.sum()
        lnp = np.where(fin, z - zmax - np.log(s), -np.inf)                   # ln p_v; -inf carries no mass
        p = e / s
        H = float(-(p[p > 0] * lnp[p > 0]).sum())
    # ---- the kernel's error bounds (module docstring), log2 units
    xs = np.abs(x[fin]).max() * a / LN2
    log2V = np.log2(max(V, 2))
    R = U * (np.ceil(V / (1024.0 * _lanes(dtype_bytes))) + 75.0 + log2V)
    dL = R / LN2 + 1e-7
    H2 = H / LN2
    spread = max(H2 - np.log2(s), 0.0)                                       # |u| / s
    dH = dL + spread * (2.0 * R + 2.0 * U)
    w_m = (V + 1) * 2.0 ** -40 + 2.0 * U + LN2 * (2.0 * U * xs + dL + 2.0 * U * H2)
    if mode == TYPICAL:
        with np.errstate(invalid="ignore"):
            d = np.where(fin, np.abs(-lnp - H), np.inf)                      # nats
        eps = lambda k: LN2 * (2.0 * U * xs + dL + dH) + 2.0 * U * k         # noqa: E731   (nats: the u k term scales with k)
        order = np.argsort(d, kind="stable")
        ds, cum = d[order], np.cumsum(p[order])
        last = np.r_[ds[1:] != ds[:-1], True]                                # the last token of every distinct key
        keys, C = ds[last], cum[last]
        hit = np.nonzero(C >= val)[0]
        reach = hit.size > 0 and np.isfinite(keys[hit[0]])
        d_star = float(keys[hit[0]]) if reach else float("inf")              # the mass never reaches m: everything is kept
        out.thr = d_star
        out.keep = (d <= d_star) | ~fin                                      # (a -inf element stays -inf: "kept" as it is)
        lo_hit = np.nonzero(C >= val - w_m)[0]
        hi_hit = np.nonzero(C >= val + w_m)[0]
        k_lo = float(keys[lo_hit[0]]) if lo_hit.size and np.isfinite(keys[lo_hit[0]]) else float("inf")
        k_hi = float(keys[hi_hit[0]]) if hi_hit.size and np.isfinite(keys[hi_hit[0]]) else float("inf")
        with np.errstate(invalid="ignore"):
            sure_keep = d + eps(d) <= k_lo - (eps(k_lo) if np.isfinite(k_lo) else 0.0)
            sure_cut = (d - eps(d) > k_hi + eps(k_hi)) if np.isfinite(k_hi) else np.zeros(V, bool)
        between = fin & ~sure_keep & ~sure_cut
        # one stored value alone between the bounds.  k_hi finite: nothing below the group reaches m - w_m and the group passes
        # m + w_m, so it is the threshold.  k_hi = +inf: nothing is surely cut, so the group is the LAST one; whether the kernel's
        # mass reaches m in it or never, everything is kept.  Either way the group is decided, and kept.
        if between.any() and np.unique(x[between]).size == 1 and np.isfinite(k_lo):
            between[:] = False                                               # one stored value: it is the threshold, and kept
        out.undecided = between
        return out
    with np.errstate(divide="ignore"):
        log2p = lnp / LN2
    t2 = np.log2(val)
    e_thr = 1e-7 + U * abs(t2)
    if mode == ETA:
        alt = 0.5 * t2 - H2
        if alt < t2:
            t2, e_thr = alt, 0.5 * e_thr + dH + U * abs(alt)
        elif abs(alt - t2) <= e_thr + dH:                                    # which of the two terms is the smaller is itself unsure
            e_thr = e_thr + dH + abs(alt - t2)
    out.thr = float(2.0 ** t2)
    below_max = x < x[fin].max()
    out.keep = ~((log2p < t2) & below_max) | ~fin                            # (a -inf element stays -inf: "kept" as it is)
    with np.errstate(invalid="ignore"):
        e_key = 2.0 * U * xs + 2.0 * U * np.abs(log2p) + dL
        out.undecided = fin & below_max & (np.abs(log2p - t2) <= e_key + e_thr)
    return out


def ref_entropy_cut(x, table, dtype_bytes=4):
    """asd_entropy_cut_rows in numpy f64.  x: [B, V] or [B, K1, V] stored values (f32); table: B records (inv_t, mode, value)
    -> (keep bool like x: True where the element stays as it is, thr f64 [B, K1]: d* in nats or the probability bound,
    undecided bool like x, touched bool [B, K1])."""
    x = np.asarray(x, dtype=np.float32)
    x3 = x[:, None] if x.ndim == 2 else x
    B, K1, V = x3.shape
    assert len(table) == B
    keep, und = np.ones((B, K1, V), bool), np.zeros((B, K1, V), bool)
    thr, touched = np.full((B, K1), np.nan), np.zeros((B, K1), bool)
    for b, (inv_t, mode, value) in enumerate(table):
        for j in range(K1):
            r = cut_row(x3[b, j], inv_t, int(mode), value, dtype_bytes)
            keep[b, j], und[b, j], thr[b, j], touched[b, j] = r.keep, r.undecided, r.thr, r.touched
    return keep.reshape(x.shape), thr, und.reshape(x.shape), touched


def undecided_rows(und):
    """How many rows of a [.., V] undecided mask hold an undecided token."""
    return int(np.asarray(und).reshape(-1, und.shape[-1]).any(axis=1).sum())


def assert_cap(und, what=""):
    """The cap, on the reference alone: at most 2 % of the rows hold an undecided token."""
    rows = int(np.prod(und.shape[:-1]))
    n = undecided_rows(und)
    assert n <= CAP * rows, (what, n, rows)
    return n


def check_cut(before, after, table, dtype_bytes=4, what=""):
    """`after` is `before` behind the kernel: outside the window every element that the reference keeps has its bits, every
    other one is -inf; an undecided element is one of the two; an untouched row is bit-equal; elements with equal stored values
    of one row share their fate.  before / after: numpy arrays of the SAME dtype view (f32, or uint16 bits beside f32 values)."""
    bx, ax = np.ascontiguousarray(before, np.float32), np.ascontiguousarray(after, np.float32)
    keep, thr, und, touched = ref_entropy_cut(bx, table, dtype_bytes)
    same = (bx.view(np.uint32) == ax.view(np.uint32))
    cut = np.isneginf(ax)
    assert (same | cut).all(), (what, "an element is neither its old bits nor -inf")
    want_cut = ~keep | np.isneginf(bx)
    bad = ~und & (cut != want_cut)
    assert not bad.any(), (what, np.argwhere(bad)[:5], thr.reshape(-1)[:4])
    b3 = bx.reshape(-1, bx.shape[-1])
    c3 = cut.reshape(-1, bx.shape[-1])
    for r in np.nonzero(und.reshape(-1, bx.shape[-1]).any(axis=1))[0]:      # equal bits, equal fate -- also inside the window
        for v in np.unique(b3[r][und.reshape(-1, bx.shape[-1])[r]]):
            assert len(set(c3[r][b3[r] == v].tolist())) == 1, (what, r, v)
    assert same.reshape(-1, bx.shape[-1])[~touched.reshape(-1)].all(), (what, "an untouched row changed")
    return keep, thr, und


class EntropyCutOracleOps(TokenStatsOracleOps):
    """TokenStatsOracleOps + pack_entropy_cut and entropy_cut_rows on the reference above: the tiny stages run without a GPU."""

    def pack_entropy_cut(self, inv_t, modes, values, device):
        self._note("pack_entropy_cut", ())
        table = [(float(np.float32(t)), int(m), float(np.float32(v))) for t, m, v in zip(inv_t, modes, values)]
        assert all(m in (OFF, TYPICAL, EPSILON, ETA) and t > 0 and (m == OFF or 0 < v < 1) for t, m, v in table)
        return SimpleNamespace(table=table, B=len(table))

    def entropy_cut_rows(self, logits, cut):
        self._note("entropy_cut_rows", ())
        assert logits.shape[0] == cut.B
        keep = ref_entropy_cut(logits.float().numpy(), cut.table)[0]
        logits[torch.from_numpy(~keep)] = float("-inf")
        return logits


# ------------------------------------------------------------------------------------------ stage-level scenarios
def _cpu(s):
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in s.items()}


def _table(rows, inv_t, B):
    inv = [float(inv_t)] * B if np.ndim(inv_t) == 0 else [float(t) for t in inv_t]
    return [(inv[b], m, v) for b, (m, v) in enumerate(rows)]


def check_steps(stage, texts, own=None, draft=None, inv_t=inv_t_of(TEMPERATURE)):
    """From the kept steps of a run_kept call.  own / draft: every row's (mode, value) of the call's own cut and, at a verifying
    stage, of the draft stage's configured cut (None: that side is off).  In every step record `cut_in` through
    ref_entropy_cut reproduces the -inf pattern of the recorded logits outside the window (check_cut), likewise cut_in_draft
    against cut_out_draft, and every proposed, accepted and drawn token is a kept one.  -> (rows looked at, undecided rows)."""
    B = len(texts)
    assert stage.step_inputs
    rows = und_rows = 0
    for s in map(_cpu, stage.step_inputs):
        post = step_rows(s)                                                  # [B, K1, V]: the rows the step committed from
        K1 = post.shape[1]
        assert ("cut_in" in s) == (own is not None) and ("cut_in_draft" in s) == (draft is not None and "tok" in s)
        if own is not None:
            before = s["cut_in"].float().numpy().reshape(post.shape)
            _, _, und = check_cut(before, post, _table(own, inv_t, B), what="own")
            rows += B * K1
            und_rows += undecided_rows(und)
        if "cut_in_draft" in s:
            _, _, und = check_cut(s["cut_in_draft"].float().numpy(), s["cut_out_draft"].float().numpy(), _table(draft, inv_t, B),
                                  what="draft")
            rows += B * (K1 - 1)
            und_rows += undecided_rows(und)
            for b in range(B):                                               # a proposal is a token its own row kept
                for k, t in enumerate(s["tok"][b].tolist()):
                    assert s["cut_out_draft"][b, k, t] > float("-inf"), (b, k, t)
        n_acc = s["n_acc"].tolist() if "tok" in s else [0] * B
        for b in range(B):
            for j in range(min(int(n_acc[b]), K1 - 1)):                      # an accepted token survives the target's cut
                assert post[b, j, int(s["tok"][b, j])] > -np.inf, (b, j)
            assert post[b, min(int(n_acc[b]), K1 - 1), int(s["drawn"][b])] > -np.inf, b
    assert und_rows <= CAP * max(rows, 1), (und_rows, rows)
    return rows, und_rows


def _kw(**more):
    return dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=TEMPERATURE, seed=SEEDS, **more)


def scenario_mode(stage, key, value):
    """One mode on its own, as the call's keyword: the cut is live (some token is cut in some step), the patterns are the
    reference's, the tokens are kept ones, and the same call repeated is bit-equal."""
    mode = {"typical_p": TYPICAL, "epsilon_cutoff": EPSILON, "eta_cutoff": ETA}[key]
    texts, lps, _ = run_kept(stage, **_kw(**{key: value}))
    own = [(mode, float(np.float32(value)))] * len(PROMPTS)
    check_steps(stage, texts, own=own)
    cut_some = any((torch.isneginf(torch.as_tensor(step_rows(_cpu(s)))) & ~torch.isneginf(s["cut_in"].cpu().float().reshape(
        step_rows(_cpu(s)).shape))).any() for s in stage.step_inputs)
    assert cut_some, "the cut removed nothing in the whole run"
    again = stage.generate(**_kw(**{key: value}))
    assert again[0] == texts and [a.tobytes() for a in again[1]] == [a.tobytes() for a in lps]
    assert all(np.isfinite(lp).all() for lp in lps)
    return texts


def scenario_per_prompt(stage):
    """Per-prompt values with one row off, three modes in one call, and per-prompt temperatures: the table takes each row's
    own 1 / T, and the row that is off is bit-equal to what entered."""
    typ = [0.5, 1.0, 0.0, 0.0, 0.3]
    eps = [0.0, 0.0, 0.02, 0.0, 0.0]
    eta = [0.0, 0.0, 0.0, 0.05, 0.0]
    own = [(TYPICAL, typ[0]), (OFF, 0.0), (EPSILON, eps[2]), (ETA, eta[3]), (TYPICAL, typ[4])]
    own = [(m, float(np.float32(v))) for m, v in own]
    for temperature in (TEMPERATURE, ROW_TEMPERATURES):
        kw = dict(_kw(typical_p=typ, epsilon_cutoff=eps, eta_cutoff=eta), temperature=temperature)
        texts, _, _ = run_kept(stage, **kw)
        inv_t = [inv_t_of(t) for t in temperature] if np.ndim(temperature) else inv_t_of(temperature)
        check_steps(stage, texts, own=own, inv_t=inv_t)
        for s in map(_cpu, stage.step_inputs):
            post = step_rows(s)
            assert np.array_equal(s["cut_in"].float().numpy().reshape(post.shape)[1].view(np.uint32), post[1].view(np.uint32))


def scenario_top_p_behind(stage):
    """Top-p on behind the cut: the nucleus acts on the survivors, so every token is still a kept one."""
    texts, _, _ = run_kept(stage, **_kw(typical_p=0.8, top_p=0.7))
    check_steps(stage, texts, own=[(TYPICAL, float(np.float32(0.8)))] * len(PROMPTS))


def scenario_tables_and_stats(stage):
    """logprobs = 5 plus token_stats: no table slot holds a cut token, and the statistics are those of the cut row."""
    texts, _, stats = run_kept(stage, **_kw(typical_p=0.4, logprobs=5, token_stats=True))
    check_steps(stage, texts, own=[(TYPICAL, float(np.float32(0.4)))] * len(PROMPTS))
    check_stage_stats(stage, texts, stats, inv_t_of(TEMPERATURE), 5)          # ref_token_stats on the rows behind the cut
    holes = 0
    for s in map(_cpu, stage.step_inputs):
        post = step_rows(s)
        ids = s["top_id"].numpy()
        for b, j, k in np.ndindex(*ids.shape):
            if ids[b, j, k] >= 0:
                assert post[b, j, ids[b, j, k]] > -np.inf, (b, j, k)
            else:
                holes += 1
                assert np.isneginf(s["top_lp"].numpy()[b, j, k])
    return holes


def scenario_allow_list(stage):
    """An allow-list in front of the cut: the row enters already masked, and only listed tokens are produced."""
    allowed = list(range(3, 60, 5))
    texts, _, _ = run_kept(stage, **_kw(typical_p=0.6, allowed_token_ids=allowed))
    check_steps(stage, texts, own=[(TYPICAL, float(np.float32(0.6)))] * len(PROMPTS))
    assert all(set(text_ids(t)) <= set(allowed) for t in texts)
    assert torch.isneginf(stage.step_inputs[0]["cut_in"].cpu().float()[..., [0, 1, 2, 4]]).all()


def scenario_configured(stage, key, value, temperature=TEMPERATURE):
    """The cut comes from the configuration (the manager was built with StageConfig.<key> = value on every stage): at stage 0
    it is the stage's own cut, at a verifying stage the DRAFT rows' alone -- the target side follows target_<key>, which is
    off.  temperature: one value, or one per prompt -- the draft side's table then takes each row's own 1 / T."""
    mode = {"typical_p": TYPICAL, "epsilon_cutoff": EPSILON, "eta_cutoff": ETA}[key]
    rows = [(mode, float(np.float32(value)))] * len(PROMPTS)
    texts, _, _ = run_kept(stage, **dict(_kw(), temperature=temperature))
    inv_t = [inv_t_of(t) for t in temperature] if np.ndim(temperature) else inv_t_of(temperature)
    if stage.draft is None:
        check_steps(stage, texts, own=rows, inv_t=inv_t)
    else:
        check_steps(stage, texts, draft=rows, inv_t=inv_t)


def scenario_greedy(stage):
    """Greedy decoding ignores the three keywords and makes no entropy_cut_rows call."""
    log = AllCalls(stage.ops)
    try:
        out = stage.generate(prompts=PROMPTS, max_tokens=4, temperature=0.0, typical_p=0.5)
        names = list(log.names)
        del log.names[:]
        base = stage.generate(prompts=PROMPTS, max_tokens=4, temperature=0.0)
        assert names == list(log.names) and "entropy_cut_rows" not in names and "pack_entropy_cut" not in names
        assert out[0] == base[0]
        del log.names[:]
        stage.generate(prompts=PROMPTS, max_tokens=4, temperature=TEMPERATURE, seed=SEEDS, typical_p=0.5)
        assert log.names.count("entropy_cut_rows") >= stage.last_steps and log.names.count("pack_entropy_cut") == 1
    finally:
        log.close()


__all__ = ["CAP", "ROW_TEMPERATURES", "EPSILON", "ETA", "EntropyCutOracleOps", "OFF", "TYPICAL", "VOCAB", "assert_cap", "check_cut", "check_steps",
           "cut_row", "ref_entropy_cut", "scenario_allow_list", "scenario_configured", "scenario_greedy", "scenario_mode",
           "scenario_per_prompt", "scenario_tables_and_stats", "scenario_top_p_behind", "undecided_rows"]
