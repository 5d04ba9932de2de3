"""Shared by the greedy-decoding tests (tests/test_greedy_stages.py on the CPU twin, tests/test_gpu_greedy.py and
tests/test_gpu_greedy_stages.py on the GPU): the numpy f64 reference of asd_verify_greedy, written from the header's text, the
ops twin that decodes through it, and the stage-level checks both stage test files run.

TEST INFRASTRUCTURE, like tests/stage_scenario.py: never importable from the package."""
import numpy as np
import torch

from tests.stage_scenario import MAX_TOKENS, PROMPTS, ref_commit_lp, ref_logprob, stage_configs, text_ids
from tests.stop_scenario import StopOracleOps

LOSSLESS_GAP = 0.05          # top-2 gap (f32-upcast logits) at or below which a teacher-forced position is skipped
LOSSLESS_KEEP = 0.8          # ... and the share of positions that must remain


def ref_argmax(x):
    """Lowest id among the maxima of the last axis of f32 values; NaN never wins; -1 where nothing is above -inf."""
    x = np.asarray(x, dtype=np.float32)
    masked = np.where(np.isnan(x), np.float32(-np.inf), x)
    am = masked.argmax(axis=-1).astype(np.int32)                      # first occurrence = lowest id
    top = np.take_along_axis(masked, am[..., None].astype(np.int64), axis=-1)[..., 0]
    return np.where(top > -np.inf, am, np.int32(-1)).astype(np.int32)


def ref_verify_greedy(x, tok=None, inv_t=1.0):
    """asd_verify_greedy in numpy f64.  x: [B, K+1, V] f32 (the stored values, upcast); tok: [B, K] i32 or None (K = 0)
    -> dict(argmax [B,K+1] i32, lp_argmax [B,K+1] f64, lp_target [B,K] f64, accept [B,K] u8, n_acc [B] i32, drawn [B] i32,
    lp_drawn [B] f64)."""
    x = np.asarray(x, dtype=np.float32)
    B, K1, V = x.shape
    K = K1 - 1
    a = float(np.float32(inv_t))
    am = ref_argmax(x)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        z = x.astype(np.float64) * a
        m = z.max(axis=-1)                                            # NaN rows: NaN (the kernels' lse of such a row is NaN too)
        lse = np.where(np.isneginf(m), -np.inf, m + np.log(np.exp(z - np.where(np.isfinite(m), m, 0.0)[..., None]).sum(axis=-1)))
        lse = np.where(np.isnan(m), np.nan, lse)
        pick = np.take_along_axis(z, np.maximum(am, 0)[..., None].astype(np.int64), axis=-1)[..., 0]
        lp_argmax = np.where(am >= 0, pick - lse, np.nan)
        lp_target = np.full((B, K), -np.inf)
        accept = np.zeros((B, K), np.uint8)
        n_acc = np.zeros(B, np.int32)
        for b in range(B):
            for k in range(K):
                t = int(tok[b, k])
                if 0 <= t < V:
                    lp_target[b, k] = z[b, k, t] - lse[b, k]
                accept[b, k] = am[b, k] >= 0 and t == am[b, k]
            n = 0
            while n < K and accept[b, n]:
                n += 1
            n_acc[b] = n
    rows = np.arange(B)
    return dict(argmax=am, lp_argmax=lp_argmax, lp_target=lp_target, accept=accept, n_acc=n_acc, drawn=am[rows, n_acc],
                lp_drawn=lp_argmax[rows, n_acc])


class GreedyOracleOps(StopOracleOps):
    """StageOracleOps (+ the stop commit) + verify_greedy on the reference above."""

    def verify_greedy(self, logits, tok=None, inv_temperature=1.0, splits=0):
        self.calls["verify_greedy"] += 1
        x = logits.float().numpy()
        if x.ndim == 2:
            x = x[:, None]
        r = ref_verify_greedy(x, None if tok is None else tok.numpy(), inv_temperature)
        f32 = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
        return (f32(r["lp_target"]), torch.from_numpy(r["n_acc"]), torch.from_numpy(r["drawn"]), f32(r["lp_drawn"]),
                torch.from_numpy(r["argmax"]), f32(r["lp_argmax"]))


# ------------------------------------------------------------------------------------------ stage-level checks
def greedy_configs(vocab=1000, **kw):
    return stage_configs(vocab=vocab, **kw)


def run_greedy(stage, prompts=PROMPTS, max_tokens=MAX_TOKENS, keep=False, **kw):
    stage.keep_inputs = keep
    try:
        return stage.generate(prompts=prompts, max_tokens=max_tokens, temperature=0.0, return_logprobs=True, **kw)
    finally:
        stage.keep_inputs = False


def check_shapes(texts, lps, max_tokens=MAX_TOKENS):
    """1. max_tokens tokens and finite, non-positive float32 log-probs per prompt."""
    assert len(texts) == len(lps) == len(PROMPTS)
    for t, lp in zip(texts, lps):
        assert len(t.split()) == max_tokens and lp.shape == (max_tokens,) and lp.dtype == np.float32
        assert np.isfinite(lp).all() and (lp <= 0).all()


def check_replay(stage, texts, lps, max_tokens=MAX_TOKENS, atol=1e-5):
    """2. From the kept step inputs: every committed token is the lowest-id arg-max of the kept row it came from (exact, no row
    skipped), the committed log-probs are the kernel's bits, and they lie within `atol` of ref_logprob(row, tok, 1.0)."""
    B = len(texts)
    got_tok = np.array([text_ids(t) for t in texts], dtype=np.int32)
    got_lp = np.stack(lps)
    seq_len = np.zeros(B, np.int32)
    tokens = np.full((B, max_tokens), -7, np.int32)
    want_lp = np.full((B, max_tokens), np.nan, np.float32)
    worst, rows_checked = 0.0, 0
    assert stage.step_inputs
    for s in stage.step_inputs:
        c = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in s.items()}
        x = c["logits"].float().numpy()
        if x.ndim == 2:
            x = x[:, None]
        K = x.shape[1] - 1
        tok = None if c["tok"] is None else c["tok"].numpy()
        am = ref_argmax(x)
        assert np.array_equal(c["argmax"].numpy().reshape(B, K + 1), am)
        n_acc, drawn, lp_drawn = c["n_acc"].numpy(), c["drawn"].numpy(), c["lp_drawn"].numpy()
        lp_t = None if tok is None else c["lp_t"].numpy()
        for b in range(B):
            n = int(n_acc[b])
            assert 0 <= n <= K
            for k in range(n):                                   # an accepted draft token IS its row's arg-max ...
                assert tok[b, k] == am[b, k] >= 0
                worst = max(worst, abs(float(lp_t[b, k]) - ref_logprob(x[b, k], tok[b, k], 1.0)))
            if n < K:                                            # ... the first rejected one is not ...
                assert tok[b, n] != am[b, n]
            assert drawn[b] == am[b, n] >= 0                     # ... and the token behind the prefix is the next row's
            worst = max(worst, abs(float(lp_drawn[b]) - ref_logprob(x[b, n], drawn[b], 1.0)))
            rows_checked += n + 1
        seq_len, tokens, want_lp, _ = ref_commit_lp(tok, lp_t, n_acc, drawn, lp_drawn, seq_len, tokens, want_lp, max_tokens)
    assert (seq_len == max_tokens).all() and rows_checked >= B * max_tokens
    assert np.array_equal(tokens, got_tok)
    assert want_lp.tobytes() == got_lp.tobytes()
    assert worst <= atol, worst
    return worst


def check_lossless(stage, texts, max_tokens=MAX_TOKENS):
    """5. Teacher-forced: at every generated position the committed token is the arg-max of the stage model's DENSE forward over
    the committed text; positions whose top-2 gap is <= LOSSLESS_GAP are skipped (the T = K + 1 and T = 1 passes may round a
    near-tie differently) and at least LOSSLESS_KEEP of the positions must remain."""
    ids = stage.encode_prompts(PROMPTS)
    P = ids.shape[1]
    gen = torch.tensor([text_ids(t) for t in texts], dtype=torch.int64, device=ids.device)
    m = stage.model
    m.reset()
    logits = m.forward(torch.cat([ids, gen], 1)).float().cpu().numpy()[:, P - 1:P - 1 + max_tokens]      # [B, max_tokens, V]
    m.reset()
    top2 = np.sort(logits, axis=-1)[..., -2:]
    clear = (top2[..., 1] - top2[..., 0]) > LOSSLESS_GAP
    assert clear.mean() >= LOSSLESS_KEEP, clear.mean()
    want = logits.argmax(-1)
    got = gen.cpu().numpy()
    assert np.array_equal(got[clear], want[clear]), np.argwhere(clear & (got != want))
    return float(clear.mean())


def pick_mid_stop(texts):
    """7. (row, position, id) of a token the greedy run commits mid-sequence and not earlier in its row."""
    for b, t in enumerate(texts):
        toks = text_ids(t)
        for i in range(2, len(toks) - 2):
            if toks[i] not in toks[:i]:
                return b, i, toks[i]
    raise AssertionError("no mid-sequence token to stop at")


def check_stop(stage, texts, lps, max_tokens=MAX_TOKENS):
    b0, i0, stop_id = pick_mid_stop(texts)
    t2, lp2, stats = run_greedy(stage, max_tokens=max_tokens, stop_token_ids=(stop_id,))
    for b, (t, lp) in enumerate(zip(texts, lps)):
        toks = text_ids(t)
        n = toks.index(stop_id) + 1 if stop_id in toks else max_tokens
        assert text_ids(t2[b]) == toks[:n] and lp2[b].tobytes() == lp[:n].tobytes()
        assert stats["finish_reasons"][b] == ("stop" if stop_id in toks else "length") and stats["n_tokens"][b] == n
    assert stats["finish_reasons"][b0] == "stop" and stats["n_tokens"][b0] == i0 + 1
