"""The numpy statement of min-p (include/asd_hip.h, "Min-p behind top-k and top-p") and the oracle ops twin that carries the
three min-p ops of distributed.HipOps by the masked-row recipe of tests/test_top_k.py.

TEST INFRASTRUCTURE, like tests/stage_scenario.py: never importable from the package."""
import math

import numpy as np
import torch

from tests.oracle_backend import _np_store
from tests.stage_scenario import StageOracleOps, ref_logprob
from tests.test_target_top_p import _leading_finite, _masked_tensor
from tests.test_top_k import top_k_thresholds


def min_p_delta(min_p, inv_t):
    """(float)(log((double)min_p) / (double)inv_temperature) of the f32 arguments the launcher is handed."""
    return np.float32(math.log(float(np.float32(min_p))) / float(np.float32(inv_t)))


def x_mp_of(rows_f32, min_p, inv_t):
    """x_max + delta of every row, one f32 addition (a row of -inf: -inf)."""
    x_max = np.asarray(rows_f32, np.float32).max(axis=-1)
    return (x_max + min_p_delta(min_p, inv_t)).astype(np.float32)


def combine(thr_kp, x_mp):
    """(thr, min-p won): thr = max(thr_kp, x_mp)."""
    thr_kp, x_mp = np.asarray(thr_kp, np.float32), np.asarray(x_mp, np.float32)
    return np.maximum(thr_kp, x_mp).astype(np.float32), x_mp > thr_kp


def min_p_thresholds(t, inv_t, top_k, top_p, min_p):
    """thr of every row of the tensor t [..., V]: max(thr_kp, x_mp), thr_kp by the oracle (tests/test_top_k.py)."""
    store, dt = _np_store(t)
    rows = store.reshape(-1, store.shape[-1])
    from oracle import oracle as O
    thr_kp = top_k_thresholds(t, inv_t, top_k, top_p)
    return combine(thr_kp, x_mp_of(O.logits_as_f32(rows, dt), min_p, inv_t))[0]


def direct_min_p(row, inv_t, min_p):
    """The direct f64 statement: softmax(x * inv_t), keep p_v >= min_p * p_max, renormalise -> (p f64 [V], keep bool [V])."""
    z = np.asarray(row, np.float64) * float(np.float32(inv_t))
    p = np.exp(z - z.max())
    p /= p.sum()
    keep = p >= float(min_p) * p.max()
    q = np.where(keep, p, 0.0)
    return q / q.sum(), keep


class MinPOracleOps(StageOracleOps):
    """StageOracleOps + draft_sample_min_p, verify_accept_min_p and residual_sample_lp(min_p=...); `trace` lists every ops call
    of a stage loop as (name, sorted keyword names)."""

    def __init__(self):
        super().__init__()
        self.trace = []

    def _note(self, name, kw):
        self.trace.append((name, tuple(sorted(kw))))

    def draft_sample(self, *a, **kw):
        self._note("draft_sample", kw)
        return super().draft_sample(*a, **kw)

    def verify_accept(self, *a, **kw):
        self._note("verify_accept", kw)
        return super().verify_accept(*a, **kw)

    def commit_step_lp(self, *a, **kw):
        self._note("commit_step_lp", kw)
        return super().commit_step_lp(*a, **kw)

    def draft_sample_min_p(self, logits, r, inv_temperature=1.0, top_k=0, top_p=1.0, min_p=0.0):
        self._note("draft_sample_min_p", ())
        thr = min_p_thresholds(logits, inv_temperature, top_k, top_p, min_p)
        tok, lp, _ = StageOracleOps.draft_sample(self, _masked_tensor(logits, thr), r, inv_temperature, 1.0)
        return tok, lp, torch.from_numpy(thr)

    def verify_accept_min_p(self, logits, tok, lp_d, u, inv_temperature=1.0, top_k=0, top_p=1.0, min_p=0.0):
        self._note("verify_accept_min_p", ())
        Bv, Kv, _ = logits.shape
        thr = min_p_thresholds(logits, inv_temperature, top_k, top_p, min_p)
        lp_t, acc, n_acc, bits = StageOracleOps.verify_accept(self, _masked_tensor(logits, thr), tok, lp_d, u, inv_temperature)
        return (lp_t, acc, n_acc, bits, torch.from_numpy(thr.reshape(Bv, Kv).copy()),
                torch.from_numpy(_leading_finite(lp_t.numpy())))

    def residual_sample_lp(self, t_logits, d_logits, n_acc, r, bonus, inv_temperature=1.0, d_threshold=None, t_threshold=None,
                           top_k=0, top_p=1.0, **kw):
        self._note("residual_sample_lp", kw)
        if "min_p" not in kw:
            return super().residual_sample_lp(t_logits, d_logits, n_acc, r, bonus, inv_temperature, d_threshold, t_threshold,
                                              top_k, top_p)
        self.calls["residual_sample_lp"] += 1
        b_thr = min_p_thresholds(bonus, inv_temperature, top_k, top_p, kw["min_p"])
        tok = self.residual_sample(_masked_tensor(t_logits, t_threshold.numpy()), d_logits, n_acc, r,
                                   _masked_tensor(bonus, b_thr), inv_temperature, d_threshold)
        K = t_logits.shape[1]
        lp = np.full(tok.shape[0], np.nan, np.float32)
        for b, t in enumerate(tok.tolist()):
            if t >= 0:
                j = int(n_acc[b])
                row, thr = (t_logits[b, j], float(t_threshold[b, j])) if 0 <= j < K else (bonus[b], float(b_thr[b]))
                lp[b] = ref_logprob(row.float().numpy(), t, inv_temperature, thr)
        return tok, torch.from_numpy(lp)

    def bonus_threshold(self, bonus, inv_temperature, top_k, top_p, min_p):
        return min_p_thresholds(bonus, inv_temperature, top_k, top_p, min_p)
