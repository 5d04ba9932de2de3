"""Relative cuts (serving/stages.py, RELATIVE CUTS; include/asd_hip.h, asd_relative_cut_rows): the numpy f64 reference of one
row under one record and coin, written from the header's text, and the boundary window that says which decisions the kernel's
f32 arithmetic may flip.  Everything outside the window must match exactly: XTC's minimum and its ties, |A| < 2, coin >= q,
ties at the maximum, -inf elements outside mu, sigma and |fin|.

THE WINDOW, from csrc/relative_cut.hip, u = 2^-24, N = 4 (f32) or 8 (16-bit) elements per vector:
  D        = ceil(V / (1024 N)) + 2 + log2 N + 6 + 16: the additions a term of an f32 sum passes through (a lane's vectors in a
             chain with its head and tail element, the tree inside a vector, 6 DPP steps, 16 waves).
  mu       f32 sum of signed terms, divided in f64, rounded once: |mu' - mu| <= dmu = D u mean|x| + u |mu|.
  sigma    sum (x - mu')^2 = sum (x - mu)^2 + |fin| (mu' - mu)^2 exactly; each term carries 3u (the difference rounds once,
             the square doubles it and rounds), the sum D u: sigma' within sigma (D + 3) u / 2 + dmu of sigma.  The quotient,
             the root and n sigma are f64; the threshold rounds once to f32: u |thr|.
             TOP-N-SIGMA: undecided iff |x_v - thr| <= n (sigma (D + 3) u / 2 + dmu) + u |thr|.
  log2 p_v = fma(x_v, c2, -L.hi) - L.lo: 2u xs + 2u |log2 p_v| + dL, with xs, R and dL of tests/entropy_cut_ref.py (the same
             (m2, s) recurrences, merges and log2_split).
  TOP-A    bound = float(log2_split(a) + 2 (x_max c2 - L)) in f64: 1e-7 + 2 (2u xs + dL) + u |bound|.
  XTC      bound = float(log2_split(t)): 1e-7 + u |log2 t|.  A token whose membership is undecided can move |A| and x_lo, so
             a row with one marks every token of A and every undecided one.
With N(0, 3^2) logits rounded to bf16 a threshold falls between stored values almost always; every test asserts the cap
(tests/entropy_cut_ref.py: 2 % of its rows) on the reference alone before it looks at the kernel.

TEST INFRASTRUCTURE: never importable from the package."""
from types import SimpleNamespace

import numpy as np

from tests.entropy_cut_ref import LN2, U, assert_cap  # noqa: F401

OFF, TOP_N_SIGMA, TOP_A, XTC = 0, 1, 2, 3


def rel_cut_row(row, rec, coin=0.0, dtype_bytes=4):
    """One row under rec = (inv_t, mode, a, b) and its coin, f64 -> SimpleNamespace(keep, undecided, touched): keep bool [V]
    (True where the element stays as it is), undecided bool [V] (the window), touched: False where the header leaves the row
    bit for bit (off, damaged record, coin >= q, |A| < 2, no distribution)."""
    x = np.asarray(row, dtype=np.float32).astype(np.float64)
    V = x.shape[0]
    out = SimpleNamespace(keep=np.ones(V, bool), undecided=np.zeros(V, bool), touched=False)
    inv_t, mode, a, q = float(np.float32(rec[0])), int(rec[1]), float(np.float32(rec[2])), float(np.float32(rec[3]))
    fin = np.isfinite(x)
    ok = 0.0 < inv_t < 3.0e38 and ((mode == TOP_N_SIGMA and 0.0 < a < np.inf) or (mode in (TOP_A, XTC) and 0.0 < a <= 1.0))
    if not ok or np.isnan(x).any() or np.isposinf(x).any() or not fin.any():
        return out
    if mode == XTC and not (0.0 < q <= 1.0 and float(np.float32(coin)) < q):
        return out
    N = 4 if dtype_bytes == 4 else 8
    xf, x_max = x[fin], x[fin].max()
    if mode == TOP_N_SIGMA:
        mu = xf.mean()
        sigma = np.sqrt(((xf - mu) ** 2).mean())
        thr = x_max - a * sigma
        D = np.ceil(V / (1024.0 * N)) + 2 + np.log2(N) + 6 + 16
        dmu = D * U * np.abs(xf).mean() + U * abs(mu)
        w = a * (sigma * (D + 3) * U / 2 + dmu) + U * abs(thr)
        out.keep = ~(fin & (x < thr))
        out.undecided = fin & (np.abs(x - thr) <= w)
        out.touched = True
        return out
    z = x * inv_t
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = z[fin].max() + np.log(np.exp(z[fin] - z[fin].max()).sum())
        log2p = np.where(fin, (z - lse) / LN2, -np.inf)
    xs = np.abs(xf).max() * inv_t / LN2
    R = U * (np.ceil(V / (1024.0 * N)) + 75.0 + np.log2(max(V, 2)))
    dL = R / LN2 + 1e-7
    with np.errstate(invalid="ignore"):
        e_key = 2.0 * U * xs + 2.0 * U * np.abs(log2p) + dL
    if mode == TOP_A:
        t2 = np.log2(a) + 2.0 * log2p[fin].max()
        e_thr = 1e-7 + 2.0 * (2.0 * U * xs + dL) + U * abs(t2)
        below = x < x_max
        out.keep = ~(fin & below & (log2p < t2))
        with np.errstate(invalid="ignore"):
            out.undecided = fin & below & (np.abs(log2p - t2) <= e_key + e_thr)
        out.touched = True
        return out
    t2 = np.log2(a)
    member = fin & (log2p >= t2)
    with np.errstate(invalid="ignore"):
        unsure = fin & (np.abs(log2p - t2) <= e_key + 1e-7 + U * abs(t2))
    if unsure.any():
        out.undecided = member | unsure
    if member.sum() >= 2:
        out.keep = ~(member & (x > x[member].min()))
    out.touched = bool(member.sum() >= 2 or unsure.any())
    return out


def ref_relative_cut(x, table, coins=None, dtype_bytes=4):
    """asd_relative_cut_rows in numpy f64.  x: [B, V] or [B, K1, V] stored values (f32); table: B records (inv_t, mode, a, b);
    coins: [B, K1] or None -> (keep, undecided: bool like x; touched bool [B, K1])."""
    x = np.asarray(x, dtype=np.float32)
    x3 = x[:, None] if x.ndim == 2 else x
    B, K1, V = x3.shape
    keep, und, touched = np.ones((B, K1, V), bool), np.zeros((B, K1, V), bool), np.zeros((B, K1), bool)
    for b, rec in enumerate(table):
        for j in range(K1):
            r = rel_cut_row(x3[b, j], rec, 0.0 if coins is None else coins[b][j], dtype_bytes)
            keep[b, j], und[b, j], touched[b, j] = r.keep, r.undecided, r.touched
    return keep.reshape(x.shape), und.reshape(x.shape), touched


def check_rel_cut(before, after, table, coins=None, dtype_bytes=4, what=""):
    """`after` is `before` behind the kernel (both f32 values of the stored elements): every element has its old bits or is
    -inf; outside the window exactly the reference's cut elements are -inf; equal stored values of a row share their fate;
    an untouched row is bit-equal.  -> (keep, undecided, touched)."""
    bx, ax = np.ascontiguousarray(before, np.float32), np.ascontiguousarray(after, np.float32)
    keep, und, touched = ref_relative_cut(bx, table, coins, dtype_bytes)
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

