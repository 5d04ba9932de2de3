"""The rule of asd_cfg_rows (include/asd_hip.h, CLASSIFIER-FREE GUIDANCE) in numpy f64 from the input bits, and its CPU twin.

TEST INFRASTRUCTURE, like tests/lookup_ref.py: never importable from the package."""
from types import SimpleNamespace

import numpy as np
import torch

from tests.watermark_ref import WatermarkOracleOps


def log_softmax(x):
    fin = x[np.isfinite(x)]
    return x - (fin.max() + np.log(np.exp(fin - fin.max()).sum()))


def guide(c, u, s):
    """One row pair (f64 arrays of the stored values) under scale s -> (the guided row in f64, the terms s c' and (1 - s) u'),
    or None where the pair is left as it is: a NaN or +inf element, no finite element, or an element whose x log2 e lies
    above f32's range, in either row."""
    if any(np.isnan(x).any() or (x == np.inf).any() or not np.isfinite(x).any() or
           (x[np.isfinite(x)] * np.log2(np.e) > np.finfo(np.float32).max).any() for x in (c, u)):
        return None
    cp, up = log_softmax(c), log_softmax(u)
    with np.errstate(invalid="ignore"):                  # (0 * -inf where c or u is -inf: replaced below)
        a, b = s * cp, (1.0 - s) * up
        g = np.where(np.isneginf(c), -np.inf, np.where(np.isneginf(u), cp, a + b))
    return g, a, np.where(np.isneginf(u), 0.0, b)


def live(scale, q, Bu):
    """Does a record {scale, uncond_seq} guide its rows?  Off: q < 0 or scale 1; damaged: scale outside [0, 100], q >= Bu."""
    return 0 <= q < Bu and scale != 1.0 and 0.0 <= scale <= 100.0


class CfgOracleOps(WatermarkOracleOps):
    """WatermarkOracleOps + pack_cfg and cfg_rows on the reference above: the tiny stages run guided without a GPU."""

    def pack_cfg(self, scales, uncond, device):
        return SimpleNamespace(recs=[(float(np.float32(s)), int(q)) for s, q in zip(scales, uncond)])

    def cfg_rows(self, cond, uncond, packed):
        self.calls["cfg_rows"] += 1
        lo = torch.finfo(cond.dtype)
        for b, (s, q) in enumerate(packed.recs):
            for j in range(cond.shape[1]) if live(s, q, uncond.shape[0]) else ():
                out = guide(cond[b, j].double().numpy(), uncond[q, j].double().numpy(), s)
                if out is not None:
                    cond[b, j] = torch.from_numpy(np.where(np.isneginf(out[0]), -np.inf, out[0].clip(lo.min, lo.max))).to(cond.dtype)
        return cond
