"""Mirostat v2 (include/asd_hip.h, asd_mirostat_rows / asd_mirostat_commit): the plain f64 reference of rules 1-5, DESIGN
section 5's bounds, the oracle ops twin, and the stage scenarios that tests/test_mirostat_stages.py (CPU twin) and
tests/test_gpu_mirostat_stages.py (HipOps) run at vocabulary 64.  TEST INFRASTRUCTURE: never importable from the package."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from tests.dry_ref import DryOracleOps
from tests.logit_edit_ref import SEEDS
from tests.stage_scenario import PROMPTS

LN2 = math.log(2.0)
U = 2.0 ** -24
VOCAB = 64
MAX_TOKENS = 16


def ref_mirostat(x, table, mu0, tok=None):
    """Rules 1-4 on x [B, K1, V] (f64 of the stored values); table[b] = (inv_t, tau, eta), tau == 0: off -> (cut [B, K1, V]: the
    elements that become -inf; mu_path [B, K1], NaN when off; gap [B, K1]: the smallest |s_v - mu_{b,j}| below the maximum;
    kk [B, K1]: the largest |log2 p| a decision or a kept element of the row has)."""
    x = np.asarray(x, dtype=np.float64)
    B, K1, V = x.shape
    cut = np.zeros(x.shape, dtype=bool)
    path, gap, kk = np.full((B, K1), np.nan), np.full((B, K1), np.inf), np.zeros((B, K1))
    for b, (inv_t, tau, eta) in enumerate(table):
        if not tau > 0:
            continue
        mu = float(mu0[b])
        for j in range(K1):
            path[b, j] = mu
            r = x[b, j]
            if np.isnan(r).any() or (r == np.inf).any() or not np.isfinite(r).any():
                continue                                                     # rule 2
            with np.errstate(divide="ignore"):
                z = r * float(inv_t)
                lse = z.max() + math.log(np.exp(z - z.max()).sum())
                s = -(z - lse) / LN2
            c = (s > mu) & (r < r.max())
            cut[b, j] = c & np.isfinite(r)
            below = np.isfinite(r) & (r < r.max())
            if below.any():
                gap[b, j] = np.abs(s[below] - mu).min()
            kk[b, j] = max(abs(mu), s.min())
            if j == K1 - 1:
                break
            t = int(tok[b][j])
            if not 0 <= t < V or r[t] == -np.inf or c[t]:                    # rule 4: rejected with certainty
                path[b, j + 1:] = mu
                break
            s_hat = s[t] + math.log2(np.exp(z[~c] - lse).sum())              # rule 3
            mu = mu - float(eta) * (s_hat - float(tau))
    return cut, path, gap, kk


def bounds(V, per_vec, xs, path, kk, eta):
    """DESIGN section 5, Mirostat, for one sequence's reference mu_path and kk -> (w [K1]: the window around mu_{b,j} inside
    which a decision may flip; dmu [K1]: the bound of |mu_path - reference|).  xs = max |x| inv_t / ln 2; R: the relative
    error of a row sum; a key is off by ek(k); log2 Z by ek + R / ln 2 + 1e-7; mu is carried in f32."""
    R = U * (math.ceil(V / (1024.0 * per_vec)) + 75.0 + math.log2(max(V, 2)))
    d_l = R / LN2 + 1e-7
    ek = lambda k: 2 * U * xs + 2 * U * abs(k) + d_l                         # noqa: E731
    w, dmu, acc = np.zeros(len(path)), np.zeros(len(path)), 0.0
    for j in range(len(path)):
        dmu[j] = acc
        w[j] = ek(kk[j]) + acc
        if j + 1 < len(path) and np.isfinite(path[j + 1]):
            acc += float(eta) * (2 * ek(kk[j]) + R / LN2 + 1e-7) + U * abs(path[j + 1]) + U * abs(path[j])
    return w, dmu


def ref_commit(path, n_acc, lp, seq_len, n_commit, table, mu, out):
    """asd_mirostat_commit on numpy arrays, in place on mu [B] f32 and out [B, max_len] f32."""
    K1 = path.shape[1]
    for b, (_, tau, eta) in enumerate(table):
        a = min(max(int(n_acc[b]), 0), K1 - 1)
        c = min(int(n_commit[b]), a + 1)
        if not tau > 0 or c <= 0:
            continue
        for i in range(c):
            pos = int(seq_len[b]) - c + i
            if 0 <= pos < out.shape[1]:
                out[b, pos] = path[b, i]
        if c == a + 1 and np.isfinite(lp[b]):
            mu[b] = np.float32(float(path[b, a]) - float(eta) * (-float(lp[b]) / LN2 - float(tau)))


class MirostatOracleOps(DryOracleOps):
    """DryOracleOps + the three Mirostat ops on the reference above: the tiny stages run without a GPU."""

    def pack_mirostat(self, inv_t, taus, etas, device):
        self._note("pack_mirostat", ())
        table = [(float(np.float32(t)), float(np.float32(a)), float(np.float32(e))) for t, a, e in zip(inv_t, taus, etas)]
        assert all(t > 0 and 0 <= a <= 32 and (a == 0 or 0 < e <= 1) for t, a, e in table)
        return SimpleNamespace(table=table, mu=torch.tensor([2.0 * a for _, a, _ in table], dtype=torch.float32), B=len(table))

    def mirostat_rows(self, logits, miro, step_tok=None):
        self._note("mirostat_rows", ())
        view = logits[:, None] if logits.dim() == 2 else logits
        assert view.shape[0] == miro.B and (view.shape[1] == 1 or step_tok.shape[1] >= view.shape[1] - 1)
        cut, path, _, _ = ref_mirostat(view.double().numpy(), miro.table, miro.mu.numpy(),
                                       None if step_tok is None else step_tok.numpy())
        view[torch.from_numpy(cut)] = float("-inf")
        return torch.from_numpy(path.astype(np.float32))

    def mirostat_commit(self, miro, mu_path, n_acc, lp, seq_len, n_commit, mu_out):
        self._note("mirostat_commit", ())
        ref_commit(mu_path.numpy(), n_acc.numpy(), lp.numpy(), seq_len.numpy(), n_commit.numpy(), miro.table, miro.mu.numpy(),
                   mu_out.numpy())


# ------------------------------------------------------------------------------------------ stage-level scenarios
TAU, ETA = 3.0, 0.25
CONFIG = dict(top_p=1.0, mirostat_tau=TAU, mirostat_eta=ETA, target_mirostat_tau=TAU, target_mirostat_eta=ETA)


def step_bound(V, xs, mu, eta, lp):
    """The bound of |mu_{i+1} - (mu_i - eta (-lp_i / ln 2 - tau))|: the chain's error of one row, and the
    verify's returned log-prob against f64 (1e-5 + 1e-6 |lp|) with its f32 rounding."""
    _, dmu = bounds(V, 4, xs, np.array([mu, mu]), np.array([abs(mu) + abs(lp) / LN2] * 2), eta)
    return dmu[1] + eta * (1e-5 + 1e-6 * abs(lp) + 2 * U * abs(lp)) / LN2


def check_mu(texts, lps, stats, taus, etas, V=VOCAB, xs=64.0):
    """mu_0 = 2 tau, mu_{i+1} = mu_i - eta (-lp_i / ln 2 - tau) to the bound, every log-prob finite; an off row holds NaN.
    xs: a bound of |x| / (T ln 2) of the tiny stages' logits (|x| < 30)."""
    for b, (lp, mu, tau, eta) in enumerate(zip(lps, stats["mirostat_mu"], taus, etas)):
        assert mu.dtype == np.float32 and mu.shape == lp.shape == (len(texts[b].split()),)
        if not tau > 0:
            assert np.isnan(mu).all(), b
            continue
        assert np.isfinite(lp).all() and mu[0] == np.float32(2.0 * tau), b
        for i in range(len(mu) - 1):
            want = float(mu[i]) - eta * (-float(lp[i]) / LN2 - tau)
            assert abs(float(mu[i + 1]) - want) <= step_bound(V, xs, float(mu[i]), eta, float(lp[i])), (b, i, mu[i + 1], want)
    return True


def scenario_configured(stage):
    """(a) The configuration's values (target_* at a verifying stage), seeded: mu's chain, and the repeated call bit-equal."""
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, temperature=0.7, seed=SEEDS)
    texts, lps, stats = stage.generate(**kw)
    check_mu(texts, lps, stats, [TAU] * len(PROMPTS), [ETA] * len(PROMPTS))
    assert all(len(set(mu.tolist())) > 1 for mu in stats["mirostat_mu"])
    again = stage.generate(**kw)
    assert again[0] == texts and all(a.tobytes() == b.tobytes() for a, b in zip(again[1], lps))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again[2]["mirostat_mu"], stats["mirostat_mu"]))
    plain = stage.generate(mirostat_tau=0.0, **kw)
    assert "mirostat_mu" not in plain[2]
    assert any(a.tobytes() != b.tobytes() for a, b in zip(plain[1], lps))    # ... and the cut is felt: the kept mass renormalises
    return texts


PER_PROMPT = dict(mirostat_tau=[2.0, 0.0, 4.0, 1.5, 3.0], mirostat_eta=[0.1, 0.1, 0.5, 1.0, 0.2], temperature=[0.7, 1.0, 0.5, 1.3, 0.9])


def scenario_per_prompt(stage):
    """(b) One value per prompt, row 1 off, per-row temperatures: every row's own chain; row 1 bit-equals the plain call."""
    kw = dict(prompts=PROMPTS, max_tokens=MAX_TOKENS, seed=SEEDS)
    texts, lps, stats = stage.generate(**PER_PROMPT, **kw)
    check_mu(texts, lps, stats, PER_PROMPT["mirostat_tau"], PER_PROMPT["mirostat_eta"])
    off = stage.generate(mirostat_tau=0.0, temperature=PER_PROMPT["temperature"], **kw)
    assert off[0][1] == texts[1] and off[1][1].tobytes() == lps[1].tobytes()
    return texts


def scenario_greedy(stage):
    """(c) Greedy decoding ignores Mirostat: the plain greedy text, and none of the three ops is reached."""
    def never(*a, **k):
        raise AssertionError("a Mirostat op was called under greedy decoding")
    kw = dict(prompts=PROMPTS, max_tokens=8, temperature=0.0)
    base = stage.generate(mirostat_tau=0.0, **kw)
    stage.ops.pack_mirostat = stage.ops.mirostat_rows = stage.ops.mirostat_commit = never
    try:
        out = stage.generate(**kw)
    finally:
        del stage.ops.pack_mirostat, stage.ops.mirostat_rows, stage.ops.mirostat_commit
    assert out[0] == base[0] and "mirostat_mu" not in out[2]
