"""Tail-free sampling (serving/stages.py, TAIL-FREE; include/asd_hip.h, asd_tail_free_rows): the numpy f64 reference of one row
under one record, written from the header's text, and the boundary window that says which decisions the kernel's arithmetic may
flip.  Everything outside the window must match exactly.

THE WINDOW W on |c_i - z S| / S, from csrc/tail_free.hip's stated arithmetic, e = 2^-52 (one f64 ulp, relative):
  w        y = inv_t * (x - x_max) is the same two f64 operations here and there: the same bits.  The device's f64 exp and
           numpy's are each documented within 1 ulp of the true value: the two w differ by at most 2 e w.
  d2_i     two differences of w and one of d1, one rounding each on either side: the two d2_i differ by at most
           2 e (w_i + 2 w_(i+1) + w_(i+2)) + e (|d1_i| + |d1_(i+1)|) + e d2_i <= 12 e w_(i); summed, 12 e Z with Z = sum w.
  sums     a d2 passes through at most C + 24 additions on the device (C = ceil(n / 1024) in the lane's chunk, 6 steps of the
           wave scan, 16 wave totals, the prefix and the partial) and n in numpy's sequential cumsum, each within e / 2:
           (C + 24 + n) (e / 2) S on any c_i and on S.
  z S      one rounding more: e S.
  W S = (1 + z) (12 e Z + (C + 24 + n) (e / 2) S) + e S.
A row whose margin is inside W has candidates i* from the first i with c_i > z S - W S to the first with c_i > z S + W S; only
tokens whose value lies between the two candidates' values are undecided, and equal stored values still share their fate.
Every test asserts the cap (tests/entropy_cut_ref.py: 2 % of its rows) on the reference alone before it looks at the kernel.

TEST INFRASTRUCTURE: never importable from the package."""
from types import SimpleNamespace

import numpy as np
import torch

from tests.entropy_cut_ref import assert_cap  # noqa: F401
from tests.mirostat_ref import MirostatOracleOps

E = 2.0 ** -52


def tfs_row(row, rec):
    """One row under rec = (inv_t, z), f64 -> SimpleNamespace(keep bool [V]: the element stays as it is; undecided bool [V]: the
    window; touched: False where the header leaves the row bit for bit; kept: the number of finite tokens that survive)."""
    x = np.asarray(row, dtype=np.float32).astype(np.float64)
    V = x.shape[0]
    fin = np.isfinite(x)
    out = SimpleNamespace(keep=np.ones(V, bool), undecided=np.zeros(V, bool), touched=False, kept=int(fin.sum()))
    inv_t, z = float(np.float32(rec[0])), float(np.float32(rec[1]))
    n = int(fin.sum())
    if not (0.0 < z < 1.0 and 0.0 < inv_t < 3.0e38) or np.isnan(x).any() or np.isposinf(x).any() or n < 3:
        return out
    xs = np.sort(x[fin])[::-1]
    w = np.exp(inv_t * (xs - xs[0]))
    d1 = w[:-1] - w[1:]
    d2 = np.abs(d1[:-1] - d1[1:])
    c = np.cumsum(d2)
    S = float(c[-1])
    if not S > 0.0:
        return out
    thr = z * S
    WS = (1.0 + z) * (12.0 * E * float(w.sum()) + (np.ceil(n / 1024.0) + 24.0 + n) * (E / 2.0) * S) + E * S
    first = lambda t: int(np.argmax(c > t)) if (c > t).any() else n - 3      # noqa: E731
    i_star, i_lo, i_hi = first(thr), first(thr - WS), first(thr + WS)
    out.keep = ~(fin & (x < xs[i_star]))
    out.undecided = fin & (x < xs[i_lo]) & (x >= xs[i_hi])
    out.touched = True
    out.kept = int((fin & out.keep).sum())
    return out


def ref_tail_free(x, table):
    """x: [B, V] or [B, K1, V] stored values (f32); table: B records (inv_t, z) -> (keep, undecided like x; touched [B, K1])."""
    x = np.asarray(x, dtype=np.float32)
    x3 = x[:, None] if x.ndim == 2 else x
    B, K1, V = x3.shape
    keep, und, touched = np.ones((B, K1, V), bool), np.zeros((B, K1, V), bool), np.zeros((B, K1), bool)
    for b, rec in enumerate(table):
        for j in range(K1):
            r = tfs_row(x3[b, j], rec)
            keep[b, j], und[b, j], touched[b, j] = r.keep, r.undecided, r.touched
    return keep.reshape(x.shape), und.reshape(x.shape), touched


def check_tail_free(before, after, table, what=""):
    """`after` is `before` behind the kernel (f32 values): every element has its old bits or is -inf; outside the window exactly
    the reference's cut elements are -inf; equal stored values of a row share their fate; an untouched row is bit-equal."""
    bx, ax = np.ascontiguousarray(before, np.float32), np.ascontiguousarray(after, np.float32)
    keep, und, touched = ref_tail_free(bx, table)
    same = bx.view(np.uint32) == ax.view(np.uint32)
    cut = np.isneginf(ax)
    assert (same | cut).all(), (what, "an element is neither its old bits nor -inf")
    bad = ~und & (cut != (~keep | np.isneginf(bx)))
    assert not bad.any(), (what, np.argwhere(bad)[:5])
    V = bx.shape[-1]
    b2, c2, u2 = bx.reshape(-1, V), cut.reshape(-1, V), und.reshape(-1, V)
    for r in np.nonzero(u2.any(axis=1))[0]:
        for v in np.unique(b2[r][u2[r]]):
            assert len(set(c2[r][b2[r] == v].tolist())) == 1, (what, r, v)
    assert same.reshape(-1, V)[~touched.reshape(-1)].all(), (what, "an untouched row changed")
    return keep, und, touched


class TailFreeOracleOps(MirostatOracleOps):
    """MirostatOracleOps + pack_tail_free and tail_free_rows on the reference above: the tiny stages run without a GPU."""

    def pack_tail_free(self, inv_t, z, device):
        self._note("pack_tail_free", ())
        table = [(float(np.float32(t)), float(np.float32(v))) for t, v in zip(inv_t, z)]
        assert all(t > 0 and 0 < v <= 1 for t, v in table)
        return SimpleNamespace(table=table, B=len(table))

    def tail_free_rows(self, logits, packed, workspace=None):
        self._note("tail_free_rows", ())
        assert logits.shape[0] == packed.B
        keep = ref_tail_free(logits.float().numpy(), packed.table)[0]
        logits[torch.from_numpy(~keep)] = float("-inf")
        return logits
