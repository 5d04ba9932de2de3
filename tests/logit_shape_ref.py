"""Shaping (serving/stages.py, SHAPING; include/asd_hip.h, asd_logit_shape_rows): the numpy f64 reference of one row under one
record, written from the header's text.  For every element it returns the INTERVAL of dtype values the kernel's f32 arithmetic
may land on, [round_dtype(lo), round_dtype(hi)] around the f64 result y; no element is skipped.

THE BOUND is derived in DESIGN.md §5 (Shaping) from csrc/logit_shape.hip, u = 2^-24.  Dynatemp: R, the relative error of s and u,
from V; dH2 and dh from R, log2_split's 1e-7 and c2's rounding; g evaluated in f64 at clamp(h -+ dh), rounded once, x g once
more -- a relative 2e-6 to 9e-6 on N(0, 3^2) rows at V = 64 ... 8203.  Quadratic: |y' - y| <= 8u (|x_max| + k d^2 + s |d|^3), a
relative 8u where x_max <= 0; above 0 the two sides can cancel and only this absolute form holds.  Both ends are then moved one
f32 ulp outwards (the f64 -> f32 -> dtype conversion of the reference itself rounds twice).

TEST INFRASTRUCTURE: never importable from the package."""
import numpy as np
import torch

OFF, DYNATEMP, QUADRATIC = 0, 1, 2
U = 2.0 ** -24
LN2 = float(np.log(2.0))
FMAX = float(np.finfo(np.float32).max)


def round_dtype(y, dtype):
    """f64 -> the dtype's value (as f32), nearest even through f32, clamped to the dtype's finite range."""
    t = torch.from_numpy(np.clip(y, -FMAX, FMAX).astype(np.float32)).to(dtype).float().numpy()
    m = float(torch.finfo(dtype).max)
    return np.clip(t, -m, m)


def value_steps(lo, hi, dtype):
    """The number of steps between two values of a 16-bit dtype (0: equal, 1: adjacent)."""
    def key(v):
        b = torch.from_numpy(v).to(dtype).view(torch.int16).numpy().astype(np.int64)
        return np.where(b >= 0, b, -(b & 0x7FFF))
    return key(hi) - key(lo)


def shape_row(row, rec, dtype):
    """One row (stored values, f32) under rec = (mode, T, a, b) -> (lo, hi, touched, sharp): the kernel's value of an element
    must lie in [lo, hi] (f32 [V]; both the input on a row the header leaves bit for bit -- touched False -- and on -inf).
    sharp bool [V]: every dynatemp element, and a quadratic element whose bound is <= 2^-13 |y| (outside the cancellation of
    x_max against k d^2): there a 16-bit interval holds at most two adjacent values, asserted on the reference alone."""
    x32 = np.asarray(row, dtype=np.float32)
    x = x32.astype(np.float64)
    V = x.shape[0]
    mode, T, a, b = int(rec[0]), float(np.float32(rec[1])), float(np.float32(rec[2])), float(np.float32(rec[3]))
    fin = np.isfinite(x)
    n = int(fin.sum())
    ok = (mode == DYNATEMP and 0.0 < a < T < np.inf and 0.0 < b < np.inf) or (mode == QUADRATIC and 0.0 < a < np.inf and 1.0 <= b <= 3.0)
    if not ok or np.isnan(x).any() or np.isposinf(x).any() or n == 0 or (mode == DYNATEMP and n < 2):
        return x32.copy(), x32.copy(), False, np.ones(V, bool)
    xf = x[fin]
    if mode == DYNATEMP:
        z = xf - xf.max()
        p = np.exp(z) / np.exp(z).sum()
        H2 = -(p[p > 0] * np.log2(p[p > 0])).sum()
        N = 4 if dtype == torch.float32 else 8
        R = U * (np.ceil(V / (1024.0 * N)) + 75.0 + np.log2(max(V, 2)))
        w = abs((p * z).sum()) / LN2
        var = (p * (xf - (p * xf).sum()) ** 2).sum()
        dH2 = R / LN2 + 1e-7 + w * (2.0 * R + 2.0 * U) + U * var / LN2
        h = H2 / np.log2(n)
        dh = (dH2 + 1e-7 * h) / np.log2(n)
        g = [T / ((T - a) + 2.0 * a * float(np.clip(hh, 0.0, 1.0)) ** b) for hh in (h + dh, h - dh)]      # (g falls with h)
        ends = np.stack([xf * g[0] * (1 - 2 * U), xf * g[0] * (1 + 2 * U), xf * g[1] * (1 - 2 * U), xf * g[1] * (1 + 2 * U)])
        ylo, yhi = ends.min(axis=0), ends.max(axis=0)
        well = np.ones(n, bool)
    else:
        k, s = float(np.float32(a * (3.0 - b) * 0.5)), float(np.float32(a * (b - 1.0) * 0.5))
        d = xf - xf.max()
        y = xf.max() - k * d * d + s * d ** 3
        delta = 8.0 * U * (abs(xf.max()) + k * d * d + s * np.abs(d) ** 3)
        ylo, yhi = y - delta, y + delta
        well = delta <= 2.0 ** -13 * np.abs(y)
    lo32 = np.nextafter(np.clip(ylo, -FMAX, FMAX).astype(np.float32), np.float32(-np.inf))
    hi32 = np.nextafter(np.clip(yhi, -FMAX, FMAX).astype(np.float32), np.float32(np.inf))
    lo, hi = x32.copy(), x32.copy()
    lo[fin], hi[fin] = round_dtype(lo32.astype(np.float64), dtype), round_dtype(hi32.astype(np.float64), dtype)
    sharp = np.ones(V, bool)
    sharp[fin] = well
    return lo, hi, True, sharp


def ref_logit_shape(x, table, dtype):
    """x: [B, K1, V] stored values (f32); table: B records -> (lo, hi: f32 like x; touched bool [B, K1]; sharp: bool like x)."""
    x = np.asarray(x, dtype=np.float32)
    lo, hi, touched, sharp = x.copy(), x.copy(), np.zeros(x.shape[:2], bool), np.ones(x.shape, bool)
    for b, rec in enumerate(table):
        for j in range(x.shape[1]):
            lo[b, j], hi[b, j], touched[b, j], sharp[b, j] = shape_row(x[b, j], rec, dtype)
    return lo, hi, touched, sharp
