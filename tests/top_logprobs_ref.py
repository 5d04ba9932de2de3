"""Shared by the top-N log-prob tests (tests/test_top_logprobs_stages.py on the CPU twin, tests/test_gpu_top_logprobs.py and
tests/test_gpu_top_logprobs_stages.py on the GPU): the numpy f64 reference of asd_top_logprobs and the numpy scatter of
asd_commit_top_logprobs, both written from the header's text, the ops twin that decodes through them, and the stage-level
checks both stage test files run.

TEST INFRASTRUCTURE, like tests/greedy_ref.py: never importable from the package."""
import numpy as np
import torch

from tests.greedy_ref import GreedyOracleOps
from tests.stage_scenario import MAX_TOKENS, PROMPTS, text_ids

N_TOP = 5                    # the specification's SamplingParams(logprobs=5)
LP_ATOL = 2e-5               # the project's tolerance for kernel log-probs against f64 at V = 152064
PAIR_ATOL = 4e-5             # two kernels, each within LP_ATOL of f64


def ref_top_logprobs(x, n, inv_t=1.0):
    """asd_top_logprobs in numpy f64.  x: [..., V] f32 (the stored values, upcast: exact) -> (ids int32 [..., n], lp f64 [..., n]).
    Order: value descending, then id ascending; NaN and -inf logits are never listed; unfilled slots hold (-1, -inf);
    lp = x[id]*a - lse(x*a) over the whole row (NaN where the row holds a NaN)."""
    x = np.asarray(x, dtype=np.float32)
    lead, V = x.shape[:-1], x.shape[-1]
    rows = x.reshape(-1, V)
    a = float(np.float32(inv_t))
    ids = np.full((rows.shape[0], n), -1, np.int32)
    lps = np.full((rows.shape[0], n), -np.inf, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for r, row in enumerate(rows):
            listed = np.flatnonzero(~np.isnan(row) & (row > -np.inf))
            order = listed[np.argsort(-row[listed], kind="stable")][:n]          # stable: equal values stay in id order
            z = row.astype(np.float64) * a
            if np.isnan(z).any():
                lse = np.nan
            else:
                m = z.max()
                lse = m + np.log(np.exp(z - m).sum()) if np.isfinite(m) else m
            ids[r, :len(order)] = order
            lps[r, :len(order)] = z[order] - lse
    return ids.reshape(*lead, n), lps.reshape(*lead, n)


def ref_commit_top(top_id, top_lp, seq_len, n_commit, out_id, out_lp, max_len):
    """asd_commit_top_logprobs on numpy arrays -> (out_id, out_lp): out[b, seq_len[b] - n_commit[b] + j] = top[b, j] for
    j < min(n_commit[b], K1), positions outside [0, max_len) not written; bits are copied."""
    out_id, out_lp = out_id.copy(), out_lp.copy()
    B, K1, _ = top_id.shape
    for b in range(B):
        first = int(seq_len[b]) - int(n_commit[b])
        for j in range(min(int(n_commit[b]), K1)):
            if 0 <= first + j < max_len:
                out_id[b, first + j] = top_id[b, j]
                out_lp[b, first + j] = top_lp[b, j]
    return out_id, out_lp


class TopOracleOps(GreedyOracleOps):
    """GreedyOracleOps + top_logprobs / commit_top_logprobs on the references above."""

    def top_logprobs(self, logits, n, inv_temperature=1.0, splits=0):
        self.calls["top_logprobs"] += 1
        x = logits.float().numpy()
        if x.ndim == 2:
            x = x[:, None]
        ids, lps = ref_top_logprobs(x, n, inv_temperature)
        return torch.from_numpy(ids), torch.from_numpy(np.ascontiguousarray(lps, dtype=np.float32))

    def commit_top_logprobs(self, top_id, top_lp, seq_len, n_commit, out_id, out_lp, max_len):
        self.calls["commit_top_logprobs"] += 1
        oi, ol = ref_commit_top(top_id.numpy(), top_lp.numpy(), seq_len.numpy(), n_commit.numpy(), out_id.numpy(), out_lp.numpy(),
                                max_len)
        out_id.copy_(torch.from_numpy(oi))
        out_lp.copy_(torch.from_numpy(ol))


# ------------------------------------------------------------------------------------------ stage-level checks
def run(stage, temperature, n=None, keep=False, prompts=PROMPTS, max_tokens=MAX_TOKENS, **kw):
    stage.keep_inputs = keep
    try:
        if n is not None:
            kw["logprobs"] = n
        return stage.generate(prompts=prompts, max_tokens=max_tokens, temperature=temperature, return_logprobs=True, **kw)
    finally:
        stage.keep_inputs = False


def step_rows(c):
    """The rows a kept step committed from, [B, K1, V] f32: stage 0's [B, V] logits, a greedy verifying step's [B, K+1, V], a
    sampled verifying step's score rows with the bonus row behind them."""
    x = c["logits"].float().numpy()
    if x.ndim == 2:
        x = x[:, None]
    if "bonus" in c:
        x = np.concatenate([x, c["bonus"].float().numpy()[:, None]], axis=1)
    return x


def check_tables(steps, texts, lps, stats, n, inv_t, greedy):
    """Shapes and dtypes; replay from the kept steps (every step's table is the reference's: ids exact, log-probs within LP_ATOL,
    no row skipped; the rows appended per sequence are the step's first n_commit rows, bit for bit); slot 0 is the committed
    token at every greedy position; a committed token found in its row is reported with a log-prob not below the row's entry
    (equal within PAIR_ATOL where nothing truncates: the caller checks that).  -> max |lp - f64|."""
    B = len(texts)
    ids_out, lps_out = stats["top_token_ids"], stats["top_logprobs"]
    assert len(ids_out) == len(lps_out) == B
    for b in range(B):
        n_b = len(texts[b].split())
        assert ids_out[b].shape == (n_b, n) and ids_out[b].dtype == np.int32
        assert lps_out[b].shape == (n_b, n) and lps_out[b].dtype == np.float32
        assert stats["n_tokens"][b] == n_b == len(lps[b])
    want_id = [[] for _ in range(B)]
    want_lp = [[] for _ in range(B)]
    worst = 0.0
    assert steps
    for s in steps:
        c = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in s.items()}
        x = step_rows(c)
        ref_id, ref_lp = ref_top_logprobs(x, n, inv_t)
        got_id, got_lp = c["top_id"].numpy(), c["top_lp"].numpy()
        assert got_id.shape == ref_id.shape and got_id.dtype == np.int32 and got_lp.dtype == np.float32
        assert np.array_equal(got_id, ref_id)
        assert np.isfinite(got_lp).all()
        worst = max(worst, float(np.abs(got_lp.astype(np.float64) - ref_lp).max()))
        nc = c["n_commit"].numpy()
        for b in range(B):
            assert 0 <= nc[b] <= x.shape[1]
            for j in range(int(nc[b])):
                want_id[b].append(got_id[b, j])
                want_lp[b].append(got_lp[b, j])
    assert worst <= LP_ATOL, worst
    for b in range(B):
        assert np.array_equal(np.array(want_id[b], np.int32).reshape(-1, n), ids_out[b]), b
        assert np.array(want_lp[b], np.float32).reshape(-1, n).tobytes() == lps_out[b].tobytes(), b
        toks = text_ids(texts[b])
        for i, t in enumerate(toks):
            row = ids_out[b][i].tolist()
            assert len(set(row)) == n and (np.diff(lps_out[b][i]) <= 0).all()          # distinct ids, most likely first
            if greedy:
                assert row[0] == t, (b, i)
            if t in row:
                assert lps[b][i] >= lps_out[b][i][row.index(t)] - PAIR_ATOL, (b, i)
    return worst


def pair_gap(texts, lps, stats):
    """Over every committed token found in its table row: max |returned log-prob - table entry|, and how many were found."""
    worst, found = 0.0, 0
    for b, text in enumerate(texts):
        for i, t in enumerate(text_ids(text)):
            row = stats["top_token_ids"][b][i].tolist()
            if t in row:
                found += 1
                worst = max(worst, abs(float(lps[b][i]) - float(stats["top_logprobs"][b][i][row.index(t)])))
    return worst, found
