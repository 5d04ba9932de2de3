"""Shared by tests/test_stages.py (CPU, oracle ops twin) and tests/test_gpu_stages.py (HipOps): the three-stage scenario, the
f64 references of the two new steps (log-softmax over a thresholded row; the per-sequence scatter) and the oracle's Bayes + DP
on the log-probs a stage returned.

TEST INFRASTRUCTURE, like tests/oracle_backend.py: never importable from the package."""
from collections import Counter

import numpy as np
import torch

from oracle import oracle as O
from tests.oracle_backend import OracleOps

PROMPTS = ["easy one", "a somewhat longer prompt , with punctuation .", "hard", "mid length prompt here", "two words"]
NAMES = ("8b", "13b", "34b")
COSTS = (1.0, 4.5, 10.0)
MAX_TOKENS = 12
DRAFT_LEN = 4
TEMPERATURE = 0.7


def ref_logprob(row, tok, inv_t, thr=-np.inf):
    """f64 log p^N(tok): softmax(x * inv_t) over { x >= thr } of one row (f32 values of the stored logits), renormalised."""
    x = np.asarray(row, dtype=np.float64)
    a = float(np.float32(inv_t))
    keep = x >= float(thr)
    z = x[keep] * a
    m = z.max()
    return float(x[int(tok)] * a - (m + np.log(np.exp(z - m).sum()))) if keep[int(tok)] else float("-inf")


def ref_commit_lp(tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, tokens, lps, max_len):
    """The per-sequence scatter of asd_commit_step_lp on numpy arrays -> (seq_len, tokens, lps, n_commit); bits are copied."""
    seq_len, tokens, lps = seq_len.copy(), tokens.copy(), lps.copy()
    B = drawn.shape[0]
    K = 0 if tok is None else tok.shape[1]
    n_commit = np.zeros(B, np.int32)
    for b in range(B):
        na = min(max(int(n_acc[b]), 0), K)
        length = int(seq_len[b])
        items = [(tok[b, k], lp_tok[b, k]) for k in range(na)] + [(drawn[b], lp_drawn[b])]
        for i, (t, lp) in enumerate(items):
            if length + i < max_len:
                tokens[b, length + i] = t
                lps[b, length + i] = lp
        n_commit[b] = min(max(max_len - length, 0), na + 1)
        seq_len[b] = length + n_commit[b]
    return seq_len, tokens, lps, n_commit


class StageOracleOps(OracleOps):
    """OracleOps + the two steps the stages add, in numpy f64, + call counters."""

    def __init__(self):
        self.calls = Counter()

    def verify_accept(self, *a, **kw):
        self.calls["verify"] += 1
        return super().verify_accept(*a, **kw)

    def draft_sample(self, *a, **kw):
        self.calls["draft_sample"] += 1
        return super().draft_sample(*a, **kw)

    def residual_sample_lp(self, t_logits, d_logits, n_acc, r, bonus, inv_temperature=1.0, d_threshold=None, t_threshold=None,
                           top_k=0, top_p=1.0):
        assert top_k <= 0 and not 0.0 < top_p < 1.0, "the CPU twin has no target truncation"
        self.calls["residual_sample_lp"] += 1
        tok = self.residual_sample(t_logits, d_logits, n_acc, r, bonus, inv_temperature, d_threshold)
        K = t_logits.shape[1]
        lp = np.full(tok.shape[0], np.nan, np.float32)
        for b, t in enumerate(tok.tolist()):
            if t >= 0:
                j = int(n_acc[b])
                row = t_logits[b, j] if 0 <= j < K else bonus[b]
                lp[b] = ref_logprob(row.float().numpy(), t, inv_temperature)
        return tok, torch.from_numpy(lp)

    def commit_step_lp(self, tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, tokens, lps, n_commit, max_len):
        self.calls["commit_step_lp"] += 1
        ln, tk, lp, nc = ref_commit_lp(None if tok is None else tok.numpy(), None if lp_tok is None else lp_tok.numpy(),
                                       n_acc.numpy(), drawn.numpy(), lp_drawn.numpy(), seq_len.numpy(), tokens.numpy(),
                                       lps.numpy(), max_len)
        seq_len.copy_(torch.from_numpy(ln))
        tokens.copy_(torch.from_numpy(tk))
        lps.copy_(torch.from_numpy(lp))
        n_commit.copy_(torch.from_numpy(nc))

    def check_status(self):
        self.calls["check_status"] += 1


def stage_configs(vocab=1000, **kw):
    """Three tiny stages; stage 1 shares stage 0's weights (whole blocks pass: bonus rows), stage 2 has its own."""
    from asd_amd.serving.stages import StageConfig
    from asd_amd.serving.synthetic_lm import tiny
    return [StageConfig(model_name=f"tiny-{n}", model_size=n, cost_per_token=c, shape=tiny(vocab=vocab), model_seed=s,
                        logit_scale=3.0, draft_len=DRAFT_LEN, seed=11 + i, **kw)
            for i, (n, c, s) in enumerate(zip(NAMES, COSTS, (0, 0, 1)))]


class LogprobPredictor:
    """The reference's predictor duck type: acceptance probability from the stage's own per-token log-probs."""

    def predict(self, prompt, draft_output, draft_logprobs, stage_id, feature_extractor):
        return self.score(draft_logprobs, stage_id)

    @staticmethod
    def score(lp, stage_id):
        lp = np.asarray(lp, dtype=np.float64)
        return float(np.clip(np.exp(lp.mean() / 2.0) + 0.15 * stage_id, 0.01, 0.99))


def record_generate(manager, ops_counter=None):
    """Wrap every stage's generate: log (stage name, prompts, logprobs, verify calls inside) per call."""
    log = []
    for name in manager.names:
        stage = manager.get_stage(name)

        def wrapped(*a, _stage=stage, _name=name, _orig=stage.generate, **kw):
            before = ops_counter() if ops_counter else 0
            out = _orig(*a, **kw)
            log.append(dict(stage=_name, prompts=list(kw.get("prompts", a[0] if a else [])), texts=out[0], logprobs=out[1],
                            verifies=(ops_counter() if ops_counter else 0) - before))
            return out
        stage.generate = wrapped
    return log


def expected_results(log, prompts, lam, stop_rule="full", n_obs=100):
    """Oracle Bayes + DP over the log-probs the stages returned -> per prompt (stage_probabilities, stopped_at_stage)."""
    L = len(NAMES)
    out = []
    for p in prompts:
        probs, k, current = [], None, p
        for i, name in enumerate(NAMES):
            if i == L - 1:
                raw = 1.0
            else:
                call = next(c for c in log if c["stage"] == name and current in c["prompts"])
                j = call["prompts"].index(current)
                raw = LogprobPredictor.score(call["logprobs"][j], i)
                current = p + " " + call["texts"][j]
            probs.append(O.py_bayesian_adjustment(raw, n_obs, 1.0, 1.0) if i < L - 1 else 1.0)
            if stop_rule == "prefix":
                k, _ = O.py_optimal_stopping_rule(probs, list(COSTS[:i + 1]), lam)
                stop = k == i
            else:
                P = [1.0] * L
                P[:i + 1] = probs
                k, _ = O.py_optimal_stopping_rule(P, list(COSTS), lam)
                stop = k <= i
            if stop or i == L - 1:
                break
        k = k if 0 <= k < len(probs) else len(probs) - 1
        out.append((probs, k))
    return out


def text_ids(text):
    return [int(w[1:]) for w in text.split()]


def check_generation(stage, texts, lps, inv_t, atol, thr_of_bonus=None, max_tokens=MAX_TOKENS):
    """From the kept step inputs: replay the commits (f64 / bit-copy reference) and compare with what generate returned; every
    accepted token carries the verify's lp_t, every drawn token the f64 log-prob at its row."""
    B = len(texts)
    got_tok = np.array([text_ids(t) for t in texts], dtype=np.int32)
    got_lp = np.stack(lps)
    assert got_tok.shape == (B, max_tokens) and got_lp.shape == (B, max_tokens) and got_lp.dtype == np.float32
    assert np.isfinite(got_lp).all() and (got_lp <= 0).all()
    seq_len = np.zeros(B, np.int32)
    tokens = np.full((B, max_tokens), -7, np.int32)
    want_lp = np.full((B, max_tokens), np.nan, np.float32)
    worst = 0.0
    for s in stage.step_inputs:
        c = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in s.items()}
        drawn, lp_drawn = c["drawn"].numpy(), c["lp_drawn"].numpy()
        if "tok" in c:                                   # a verifying stage
            n_acc, K = c["n_acc"].numpy(), c["tok"].shape[1]
            rows = [c["logits"][b, n_acc[b]] if n_acc[b] < K else c["bonus"][b] for b in range(B)]
            thr = [(-np.inf if c["t_thr"] is None else float(c["t_thr"][b, n_acc[b]])) if n_acc[b] < K
                   else (-np.inf if thr_of_bonus is None else thr_of_bonus(c["bonus"])[b]) for b in range(B)]
            tok, lp_tok = c["tok"].numpy(), c["lp_t"].numpy()
        else:                                            # stage 0: the draw's own log q
            n_acc, rows, thr, tok, lp_tok = np.zeros(B, np.int32), list(c["logits"]), c["thr"].numpy(), None, None
        for b in range(B):
            ref = ref_logprob(rows[b].float().numpy(), drawn[b], inv_t, thr[b])
            worst = max(worst, abs(float(lp_drawn[b]) - ref))
        seq_len, tokens, want_lp, _ = ref_commit_lp(tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, tokens, want_lp, max_tokens)
    assert (seq_len == max_tokens).all()
    assert np.array_equal(tokens, got_tok)
    assert want_lp.tobytes() == got_lp.tobytes()         # accepted: the verify's lp_t bits; drawn: the draw's lp bits
    assert worst <= atol, worst
    return worst
