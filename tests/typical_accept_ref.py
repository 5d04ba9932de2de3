"""Typical acceptance (serving/stages.py, TYPICAL ACCEPTANCE; include/asd_hip.h, asd_typical_accept): the numpy f64 reference on
the stored logits, written from the header's text, and the CPU twin of the op for the tiny stages.

TEST INFRASTRUCTURE: never importable from the package."""
from types import SimpleNamespace

import numpy as np
import torch

from tests.tail_free_ref import TailFreeOracleOps


def ref_typical_accept(x, tok, table):
    """x: [B, K, V] stored values; tok: [B, K]; table: B records (inv_t, ln_eps, ln_alpha) -> (lp_t f64 [B, K], H f64 [B, K],
    threshold f64 [B, K], accept bool [B, K], bits uint64 [B], n_acc int32 [B])."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    B, K, V = x.shape
    lp, H, thr = (np.full((B, K), np.nan) for _ in range(3))
    acc = np.zeros((B, K), bool)
    for b, (inv_t, ln_eps, ln_alpha) in enumerate(table):
        inv_t, ln_eps, ln_alpha = (float(np.float32(v)) for v in (inv_t, ln_eps, ln_alpha))
        if not (0.0 < inv_t < 3.0e38 and np.isfinite(ln_eps) and np.isfinite(ln_alpha)):
            continue                                                             # a damaged record rejects its sequence
        for k in range(K):
            row, fin = x[b, k], np.isfinite(x[b, k])
            if np.isnan(row).any() or np.isposinf(row).any() or not fin.any():
                continue                                                         # NaN, NaN, reject
            y = row[fin] * inv_t
            m = y.max()
            e = np.exp(y - m)
            L = m + np.log(e.sum())
            H[b, k] = max(L - float((y * e).sum() / e.sum()), 0.0)
            t = int(tok[b, k])
            lp[b, k] = row[t] * inv_t - L if 0 <= t < V and fin[t] else -np.inf
            thr[b, k] = min(ln_eps, ln_alpha - H[b, k])
            acc[b, k] = lp[b, k] > thr[b, k]
    bits = (acc.astype(np.uint64) << np.arange(K, dtype=np.uint64)).sum(axis=1).astype(np.uint64)
    n_acc = np.array([K if r.all() else int(np.argmin(r)) for r in acc], dtype=np.int32)
    return lp, H, thr, acc, bits, n_acc


class TypicalAcceptOracleOps(TailFreeOracleOps):
    """TailFreeOracleOps + pack_typical_accept and typical_accept on the reference above: the tiny stages run without a GPU."""

    def pack_typical_accept(self, inv_t, eps, alpha, device):
        self._note("pack_typical_accept", ())
        table = [(float(np.float32(t)), float(np.float32(np.log(e))), float(np.float32(np.log(a)))) for t, e, a in zip(inv_t, eps, alpha)]
        assert all(t > 0 and 0 < e <= 1 and 0 < a <= 100 for t, e, a in zip(inv_t, eps, alpha))
        return SimpleNamespace(table=table, B=len(table))

    def typical_accept(self, logits, tok, packed, workspace=None, splits=0):
        self._note("typical_accept", ())
        assert logits.shape[0] == packed.B and tuple(tok.shape) == tuple(logits.shape[:2]) and logits.shape[1] <= 16
        lp, H, _, _, bits, n_acc = ref_typical_accept(logits.float().numpy(), tok.numpy(), packed.table)
        return (torch.from_numpy(lp.astype(np.float32)), torch.from_numpy(H.astype(np.float32)),
                torch.from_numpy(bits.view(np.int64)), torch.from_numpy(n_acc))
