"""Per-request sampling parameters (serving/stages.py, PER-REQUEST SAMPLING): the oracle ops twin that carries the four *_rows
ops of distributed.HipOps, the mixed parameter sets the CPU and GPU stage tests share, and check_generation of
tests/stage_scenario.py with each row's own temperature and thresholds.

RowsOracleOps implements a *_rows op by calling the SCALAR twin op the stage loop would call for that row's values
(the dispatch of serving/stages.py's _Sampled) on the one-row slice: row b of a mixed call is the scalar call's row by
construction, which is the semantics include/asd_hip.h states for the kernels.

TEST INFRASTRUCTURE, like tests/stage_scenario.py: never importable from the package."""
from types import SimpleNamespace

import numpy as np
import torch

from tests.min_p_ref import MinPOracleOps, combine, x_mp_of
from tests.oracle_backend import _np_store
from tests.philox_ref import step_uniforms_ref
from tests.stage_scenario import MAX_TOKENS, PROMPTS, StageOracleOps, ref_commit_lp, ref_logprob, text_ids
from tests.test_target_top_p import _leading_finite, _masked_tensor
from tests.test_top_k import top_k_thresholds
from tests.top_logprobs_ref import ref_commit_top, ref_top_logprobs

# one value per prompt of stage_scenario.PROMPTS.  MIXED: top-p alone, top-k + min-p, a tight top-p, top-k alone and a row that
# truncates NOTHING (the untruncated-verify exception); rows 0 and 2 differ in every value but share a mode.
MIXED = dict(temperature=[0.7, 1.0, 0.5, 1.3, 0.9], top_p=[0.9, 1.0, 0.8, 1.0, 1.0], top_k=[0, 50, 0, 20, 0],
             min_p=[0.0, 0.1, 0.0, 0.0, 0.0])
# every row truncates something (so a verifying stage's row is bit-equal to the scalar call's); rows 0 and 4 share a set
TRUNCATED = dict(temperature=[0.7, 1.0, 0.5, 1.3, 0.7], top_p=[0.9, 1.0, 0.8, 1.0, 0.9], top_k=[0, 50, 0, 20, 0],
                 min_p=[0.0, 0.1, 0.0, 0.3, 0.0])


def inv_t_of(temperature):
    """The stage's own statement: float(np.float32(1 / T))."""
    return float(np.float32(1.0 / temperature))


def row_values(params, b):
    """Row b's four values as the keyword arguments of a scalar generate call."""
    return {k: v[b] for k, v in params.items()}


def thresholds(t, inv_t, top_k, top_p, min_p):
    """thr of every row of the tensor t [..., V] under Temperature -> TopK -> TopP -> MinP with the off switches of
    include/asd_hip.h (top_k <= 0 or >= V, top_p outside (0, 1), min_p <= 0): -inf where nothing truncates."""
    V = t.shape[-1]
    thr = top_k_thresholds(t, inv_t, top_k if 0 < top_k < V else 0, top_p)
    if min_p > 0.0:
        from oracle import oracle as O
        store, dt = _np_store(t)
        thr = combine(thr, x_mp_of(O.logits_as_f32(store.reshape(-1, V), dt), min_p, inv_t))[0]
    return thr


class RowsOracleOps(MinPOracleOps):
    """MinPOracleOps + the scalar top-k / top-p twins the stage loops dispatch to, + pack_sampling_rows and the four *_rows
    ops (each row through the scalar twin of its values), + the top-N and seeded ops a rows call may add.  `trace` lists the
    ops calls the STAGE made; the scalar calls a *_rows op makes inside are not listed."""

    def __init__(self):
        super().__init__()
        self._inside = 0

    def _note(self, name, kw):
        if not self._inside:
            super()._note(name, kw)

    # ---- scalar twins missing from MinPOracleOps (the masked-row recipe of tests/test_top_k.py)
    def draft_sample_top_k(self, logits, r, inv_temperature=1.0, top_k=0, top_p=1.0):
        self._note("draft_sample_top_k", ())
        thr = thresholds(logits, inv_temperature, top_k, top_p, 0.0)
        tok, lp, _ = StageOracleOps.draft_sample(self, _masked_tensor(logits, thr), r, inv_temperature, 1.0)
        return tok, lp, torch.from_numpy(thr)

    def _verify_masked(self, logits, tok, lp_d, u, inv_t, top_k, top_p, min_p):
        Bv, Kv, _ = logits.shape
        thr = thresholds(logits, inv_t, top_k, top_p, min_p)
        lp_t, acc, n_acc, bits = StageOracleOps.verify_accept(self, _masked_tensor(logits, thr), tok, lp_d, u, inv_t)
        return (lp_t, acc, n_acc, bits, torch.from_numpy(thr.reshape(Bv, Kv).copy()), torch.from_numpy(_leading_finite(lp_t.numpy())))

    def verify_accept_top_k(self, logits, tok, lp_d, u, inv_temperature=1.0, top_k=0, top_p=1.0):
        self._note("verify_accept_top_k", ())
        return self._verify_masked(logits, tok, lp_d, u, inv_temperature, top_k, top_p, 0.0)

    def verify_accept_top_p(self, logits, tok, lp_d, u, inv_temperature=1.0, top_p=1.0):
        self._note("verify_accept_top_p", ())
        return self._verify_masked(logits, tok, lp_d, u, inv_temperature, 0, top_p, 0.0)

    def residual_sample_lp(self, t_logits, d_logits, n_acc, r, bonus, inv_temperature=1.0, d_threshold=None, t_threshold=None,
                           top_k=0, top_p=1.0, **kw):
        self._note("residual_sample_lp", kw)
        min_p = kw.get("min_p", 0.0)
        K, V = t_logits.shape[1], t_logits.shape[2]
        if not 0 < top_k < V and not 0.0 < top_p < 1.0 and not min_p > 0.0:
            return StageOracleOps.residual_sample_lp(self, t_logits, d_logits, n_acc, r, bonus, inv_temperature, d_threshold, None)
        self.calls["residual_sample_lp"] += 1
        b_thr = thresholds(bonus, inv_temperature, top_k, top_p, min_p)
        tok = self.residual_sample(_masked_tensor(t_logits, t_threshold.numpy()), d_logits, n_acc, r, _masked_tensor(bonus, b_thr),
                                   inv_temperature, d_threshold)
        lp = np.full(tok.shape[0], np.nan, np.float32)
        for b, t in enumerate(tok.tolist()):
            if t >= 0:
                j = int(n_acc[b])
                row, thr = (t_logits[b, j], float(t_threshold[b, j])) if 0 <= j < K else (bonus[b], float(b_thr[b]))
                lp[b] = ref_logprob(row.float().numpy(), t, inv_temperature, thr)
        return tok, torch.from_numpy(lp)

    # ---- the packed table: the rows' values, as they are
    def pack_sampling_rows(self, inv_temperature, top_k, top_p, min_p, V, dtype, device):
        self._note("pack_sampling_rows", ())
        n = len(inv_temperature)
        return SimpleNamespace(inv_t=[float(v) for v in inv_temperature], top_k=[0] * n if top_k is None else [int(v) for v in top_k],
                               top_p=[1.0] * n if top_p is None else [float(v) for v in top_p],
                               min_p=[0.0] * n if min_p is None else [float(v) for v in min_p], V=V)

    @staticmethod
    def _values(rows, b):
        k = rows.top_k[b] if 0 < rows.top_k[b] < rows.V else 0
        return rows.inv_t[b], k, rows.top_p[b], rows.min_p[b]

    def _draft_row(self, logits, r, inv_t, top_k, top_p, min_p):
        """_Sampled._draft_op's dispatch."""
        if min_p > 0.0:
            return self.draft_sample_min_p(logits, r, inv_t, top_k=top_k, top_p=top_p, min_p=min_p)
        if top_k > 0:
            return self.draft_sample_top_k(logits, r, inv_t, top_k=top_k, top_p=top_p)
        return self.draft_sample(logits, r, inv_t, top_p)

    def _verify_row(self, logits, tok, lp_d, u, inv_t, top_k, top_p, min_p):
        """_Sampled._verify_op's dispatch; the plain verify's outputs completed with thr = -inf and the leading finite run."""
        if min_p > 0.0:
            return self.verify_accept_min_p(logits, tok, lp_d, u, inv_t, top_k=top_k, top_p=top_p, min_p=min_p)
        if top_k > 0:
            return self.verify_accept_top_k(logits, tok, lp_d, u, inv_t, top_k=top_k, top_p=top_p)
        if 0.0 < top_p < 1.0:
            return self.verify_accept_top_p(logits, tok, lp_d, u, inv_t, top_p=top_p)
        lp_t, acc, n_acc, bits = self.verify_accept(logits, tok, lp_d, u, inv_t)
        return (lp_t, acc, n_acc, bits, torch.full(tuple(tok.shape), float("-inf"), dtype=torch.float32),
                torch.from_numpy(_leading_finite(lp_t.numpy())))

    def draft_sample_rows(self, logits, r, rows):
        self._note("draft_sample_rows", ())
        self._inside += 1
        try:
            out = [self._draft_row(logits[b:b + 1], r[b:b + 1], *self._values(rows, b)) for b in range(logits.shape[0])]
        finally:
            self._inside -= 1
        return tuple(torch.cat([o[i] for o in out]) for i in range(3))

    def verify_accept_rows(self, logits, tok, lp_d, u, rows):
        self._note("verify_accept_rows", ())
        self._inside += 1
        try:
            out = [self._verify_row(logits[b:b + 1], tok[b:b + 1], lp_d[b:b + 1], u[b:b + 1], *self._values(rows, b))
                   for b in range(logits.shape[0])]
        finally:
            self._inside -= 1
        return tuple(torch.cat([o[i] for o in out]) for i in range(6))

    def residual_sample_lp_rows(self, t_logits, d_logits, n_acc, r, bonus, rows, d_threshold=None, t_threshold=None):
        self._note("residual_sample_lp_rows", ())
        self._inside += 1
        try:
            out = []
            for b in range(t_logits.shape[0]):
                inv_t, top_k, top_p, min_p = self._values(rows, b)
                mp = dict(min_p=min_p) if min_p > 0.0 else {}
                s = slice(b, b + 1)
                out.append(self.residual_sample_lp(t_logits[s], d_logits[s], n_acc[s], r[s], bonus[s], inv_t,
                                                   d_threshold=None if d_threshold is None else d_threshold[s],
                                                   t_threshold=t_threshold[s], top_k=top_k, top_p=top_p, **mp))
        finally:
            self._inside -= 1
        return tuple(torch.cat([o[i] for o in out]) for i in range(2))

    def bonus_threshold_rows(self, bonus, rows_values):
        """[B] thresholds of the bonus rows, row b under rows_values[b] = (inv_t, top_k, top_p, min_p)."""
        return np.array([thresholds(bonus[b:b + 1], *v)[0] for b, v in enumerate(rows_values)], np.float32)

    # ---- top-N tables and seeds (tests/top_logprobs_ref.py, tests/philox_ref.py)
    def top_logprobs(self, logits, n, inv_temperature=1.0, splits=0):
        self._note("top_logprobs", ())
        x = logits.float().numpy()
        ids, lps = ref_top_logprobs(x[:, None] if x.ndim == 2 else x, n, inv_temperature)
        return torch.from_numpy(ids), torch.from_numpy(np.ascontiguousarray(lps, dtype=np.float32))

    def top_logprobs_rows(self, logits, n, rows, splits=0):
        self._note("top_logprobs_rows", ())
        self._inside += 1
        try:
            out = [self.top_logprobs(logits[b:b + 1], n, rows.inv_t[b]) for b in range(logits.shape[0])]
        finally:
            self._inside -= 1
        return tuple(torch.cat([o[i] for o in out]) for i in range(2))

    def commit_top_logprobs(self, top_id, top_lp, seq_len, n_commit, out_id, out_lp, max_len):
        self._note("commit_top_logprobs", ())
        oi, ol = ref_commit_top(top_id.numpy(), top_lp.numpy(), seq_len.numpy(), n_commit.numpy(), out_id.numpy(), out_lp.numpy(),
                                max_len)
        out_id.copy_(torch.from_numpy(oi))
        out_lp.copy_(torch.from_numpy(ol))

    def step_uniforms(self, seeds, step, stage, K_draft, K_accept, commit=True, out=None):
        self._note("step_uniforms", ())
        rd, u, rc = step_uniforms_ref(seeds, step, stage, K_draft, K_accept)
        return (torch.from_numpy(rd) if K_draft > 0 else None, torch.from_numpy(u) if K_accept > 0 else None,
                torch.from_numpy(rc) if commit else None)


def own_values(stage, params):
    """(inv_t, top_k, top_p, min_p) of every row of a generate call with the per-prompt `params` on `stage`."""
    B = len(params["temperature"])
    return [(inv_t_of(params["temperature"][b]), int(params["top_k"][b]), float(params["top_p"][b]), float(params["min_p"][b]))
            for b in range(B)]


def check_generation_rows(stage, texts, lps, values, atol, bonus_thr, max_tokens=MAX_TOKENS):
    """tests/stage_scenario.check_generation with every row's own temperature and threshold: `values[b]` = row b's (inv_t,
    top_k, top_p, min_p); bonus_thr(bonus [B, V] tensor) -> the [B] thresholds of the bonus rows under the rows' values.
    Replays the commits from the kept step inputs (f64 / bit-copy reference); every accepted token carries the verify's lp_t,
    every drawn token the f64 log-prob at its row under ITS temperature and threshold.  -> max |lp_drawn - f64|."""
    B = len(texts)
    got_tok = np.array([text_ids(t) for t in texts], dtype=np.int32)
    got_lp = np.stack(lps)
    assert got_tok.shape == (B, max_tokens) and got_lp.shape == (B, max_tokens) and got_lp.dtype == np.float32
    # a kept set of ONE token has q = 1, and the f32 normaliser can leave its log-prob a rounding above 0: that reads as 0
    # exactly where the row's min-p is on (include/asd_hip.h, "Min-p"); elsewhere it stays, bounded by that rounding
    print(f"[per-request] largest returned log-prob per row: {got_lp.max(axis=1).tolist()}")
    assert np.isfinite(got_lp).all(), got_lp
    for b in range(B):
        assert (got_lp[b] <= (0.0 if values[b][3] > 0.0 else 1e-6)).all(), (b, float(got_lp[b].max()))
    seq_len = np.zeros(B, np.int32)
    tokens = np.full((B, max_tokens), -7, np.int32)
    want_lp = np.full((B, max_tokens), np.nan, np.float32)
    worst = 0.0
    assert stage.step_inputs
    for s in stage.step_inputs:
        c = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in s.items()}
        drawn, lp_drawn = c["drawn"].numpy(), c["lp_drawn"].numpy()
        if "tok" in c:                                   # a verifying stage
            n_acc, K = c["n_acc"].numpy(), c["tok"].shape[1]
            assert c["t_thr"] is not None                # the rows route always reports thresholds
            b_thr = bonus_thr(c["bonus"])
            rows = [c["logits"][b, n_acc[b]] if n_acc[b] < K else c["bonus"][b] for b in range(B)]
            thr = [float(c["t_thr"][b, n_acc[b]]) if n_acc[b] < K else float(b_thr[b]) for b in range(B)]
            tok, lp_tok = c["tok"].numpy(), c["lp_t"].numpy()
        else:                                            # stage 0: the draw's own log q
            n_acc, rows, thr, tok, lp_tok = np.zeros(B, np.int32), list(c["logits"]), c["thr"].numpy(), None, None
        for b in range(B):
            x = rows[b].float().numpy()
            assert x[drawn[b]] >= thr[b]                 # the committed draw lies in its row's kept set
            ref = ref_logprob(x, drawn[b], values[b][0], thr[b])
            worst = max(worst, abs(float(lp_drawn[b]) - ref))
        seq_len, tokens, want_lp, _ = ref_commit_lp(tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, tokens, want_lp, max_tokens)
    assert (seq_len == max_tokens).all()
    assert np.array_equal(tokens, got_tok)
    assert want_lp.tobytes() == got_lp.tobytes()         # accepted: the verify's lp_t bits; drawn: the draw's lp bits
    assert worst <= atol, worst
    return worst


def check_stage0_thresholds(stage, values):
    """Stage 0 of a rows call: every kept step's thresholds are the twin's for the row's own values, bit for bit."""
    for s in stage.step_inputs:
        lg = s["logits"].cpu()
        want = np.array([thresholds(lg[b:b + 1], *values[b])[0] for b in range(lg.shape[0])], np.float32)
        assert s["thr"].cpu().numpy().tobytes() == want.tobytes()


__all__ = ["MIXED", "TRUNCATED", "PROMPTS", "RowsOracleOps", "check_generation_rows", "check_stage0_thresholds", "inv_t_of",
           "own_values", "row_values", "thresholds"]
