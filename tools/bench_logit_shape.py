#!/usr/bin/env python3
"""Time the shaping pass (asd_logit_shape_rows) against the relative-cut pass in top-a mode, on one bf16 tensor [32, K1, 152064]
for K1 = 9 (a verifying step's output at B = 32, K = 8: 88 MB) and K1 = 1 (stage 0), all variants of a K1 in the same process
on copies of the same values:

  top_a       asd_relative_cut_rows, a = 0.2 on every row           -- the baseline: reads the row once, writes almost nothing
  dynatemp    asd_logit_shape_rows, r = 0.3, e = 1, T = 0.7         -- (m2, s, u) sweep, then every vector rewritten
  quadratic   asd_logit_shape_rows, f = 0.3, c = 1                  -- maximum sweep, then every vector rewritten
  unchanged   asd_logit_shape_rows, f = 0.3 on FLAT rows            -- both sweeps, every vector compares equal: no store issued
  g_is_one    asd_logit_shape_rows, r = 1e-9, e = 1, T = 0.7        -- float(T / T_dyn) == 1: the statistics sweep, no write sweep

    python tools/bench_logit_shape.py [--out profiles/logit_shape.json] [--repeats 30]

A full-row rewrite moves up to twice the baseline's bytes, so a ratio near 2 when every vector changes is the expectation to
compare against, not a threshold.  The passes work in place, so every round restores the tensor from a pristine copy before
each launch (the copies are torch kernels and are not counted).  Kernel time comes from a `rocprofv3 --kernel-trace --stats` run
OF ITS OWN per K1 (no counters, no other tracing): this script starts itself once more under the profiler as a fresh child
process (`--worker`) before it touches the GPU; each child is one GPU step under its own time limit, and a failure ends the
tool.  A child launches the five in alternation, `--repeats` times after 3 warm-up rounds; the four asd_logit_shape_rows
dispatches of a round are told apart by their position in it.  Reported per K1 and variant: the median, minimum, maximum and
quartiles over the repeats, the ratio of each median to the baseline's, and the baseline's spread ((max - min) / median and
(p75 - p25) / median).  This is a measurement, not a pass mark.  Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_entropy_cut import WARMUP, _column, run_step  # noqa: E402,F401

VARIANTS = ("top_a", "dynatemp", "quadratic", "unchanged", "g_is_one")
TOP_A, RANGE, EXPONENT, FACTOR, CURVE, TEMPERATURE, TINY_RANGE = 0.2, 0.3, 1.0, 0.3, 1.0, 0.7, 1e-9
STEP_LIMIT_S = 300


def worker(a) -> int:
    import torch
    from asd_amd import kernels as K
    B, K1, V = a.batch, a.rows, a.vocab
    g = torch.Generator(device="cuda").manual_seed(1)
    x0 = (torch.randn((B, K1, V), generator=g, device="cuda") * 3.0).to(torch.bfloat16)
    flat0 = torch.full((B, K1, V), 1.5, dtype=torch.bfloat16, device="cuda")
    x, y, flat = x0.clone(), x0.clone(), flat0.clone()
    top_a = K.pack_relative_cut([1.0 / TEMPERATURE] * B, [K.RELCUT_TOP_A] * B, [TOP_A] * B, [0.0] * B, "cuda")
    dyn = K.pack_logit_shape([TEMPERATURE] * B, [K.SHAPE_DYNATEMP] * B, [RANGE] * B, [EXPONENT] * B, "cuda")
    quad = K.pack_logit_shape([TEMPERATURE] * B, [K.SHAPE_QUADRATIC] * B, [FACTOR] * B, [CURVE] * B, "cuda")
    one = K.pack_logit_shape([TEMPERATURE] * B, [K.SHAPE_DYNATEMP] * B, [TINY_RANGE] * B, [EXPONENT] * B, "cuda")   # |T_dyn - T| <= 1e-9: g rounds to 1
    # sane answers before any timing: the quadratic map against torch on two sequences, to one bf16 step (and 1e-3 where
    # x_max and f d^2 cancel)
    K.logit_shape_rows(y, quad)
    r = x0[:2].float()
    want = (r.amax(-1, keepdim=True) - FACTOR * (r - r.amax(-1, keepdim=True)) ** 2).to(torch.bfloat16).float()
    assert bool(((y[:2].float() - want).abs() <= want.abs() * 2.0 ** -7 + 1e-3).all())
    torch.cuda.synchronize()
    for _ in range(WARMUP + a.repeats):
        x.copy_(x0)
        K.relative_cut_rows(x, top_a)
        for t, t0, packed in ((y, x0, dyn), (y, x0, quad), (flat, flat0, quad), (y, x0, one)):
            t.copy_(t0)
            K.logit_shape_rows(t, packed)
    assert torch.equal(flat, flat0) and torch.equal(y, x0)                   # the flat rows and the g == 1 rows kept their bits
    torch.cuda.synchronize()
    return 0


def parse_trace(directory, repeats):
    """The kernel-trace CSV(s) under `directory` -> {variant: [kernel time in us of the last `repeats` dispatches]}."""
    import csv
    import glob
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rd = csv.DictReader(f)
            kn = _column(rd.fieldnames, "kernel_name")
            t0, t1 = _column(rd.fieldnames, "start_timestamp"), _column(rd.fieldnames, "end_timestamp")
            rows += [(int(r[t0]), int(r[t1]), r[kn]) for r in rd]
    if not rows:
        raise RuntimeError(f"no kernel trace under {directory}")
    rows.sort()
    base = [(e - s) / 1e3 for s, e, name in rows if "k_relative_cut_rows" in name.replace(" ", "")]
    shaped = [(e - s) / 1e3 for s, e, name in rows if "k_logit_shape_rows" in name.replace(" ", "")]
    rounds = WARMUP + repeats
    if len(base) != rounds or len(shaped) != 1 + 4 * rounds:                 # the check ahead of the loop launches one pass
        raise RuntimeError(f"{len(base)} asd_relative_cut_rows and {len(shaped)} asd_logit_shape_rows dispatches in the trace, "
                           f"expected {rounds} and {1 + 4 * rounds}")
    out = {"top_a": base}
    out.update({v: shaped[1 + i::4] for i, v in enumerate(VARIANTS[1:])})
    return {v: t[-repeats:] for v, t in out.items()}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logit_shape.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rows", type=int, default=9, help=argparse.SUPPRESS)
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)

    res = {"what": "asd_logit_shape_rows (dynatemp r = 0.3, e = 1, T = 0.7; quadratic f = 0.3, c = 1; the quadratic on flat rows, "
                   "which it leaves unchanged; dynatemp r = 1e-9, where g == 1 and no write sweep runs; N(0, 3^2) logits) vs asd_relative_cut_rows (top_a = 0.2) on copies of one "
                   "[B, K1, V] bf16 tensor: kernel time from a rocprofv3 --kernel-trace --stats run of its own per K1, the five "
                   "launched in alternation in one process, the tensor restored before every pass",
           "B": a.batch, "V": a.vocab, "dtype": "bf16", "repeats": a.repeats, "warmup_rounds": WARMUP}
    for K1 in (9, 1):
        entry = res[f"K1={K1}"] = {"rows": a.batch * K1, "logit_bytes": a.batch * K1 * a.vocab * 2}
        directory = tempfile.mkdtemp(prefix="logit_shape_trace_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", directory, "--", sys.executable,
               os.path.abspath(__file__), "--worker", "--batch", str(a.batch), "--rows", str(K1), "--vocab", str(a.vocab),
               "--repeats", str(a.repeats)]
        try:
            run_step(cmd, STEP_LIMIT_S)                                      # one GPU step, under its own limit
            times = parse_trace(directory, a.repeats)
            for v in VARIANTS:
                t = times[v]
                q = statistics.quantiles(t, n=4)
                entry[v] = {"us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                            "us_p25": round(q[0], 2), "us_p75": round(q[2], 2)}
            base = entry["top_a"]
            entry["baseline_spread"] = round((base["us_max"] - base["us_min"]) / base["us_median"], 4)
            entry["baseline_quartile_spread"] = round((base["us_p75"] - base["us_p25"]) / base["us_median"], 4)
            for v in VARIANTS[1:]:
                entry[f"{v}_over_baseline"] = round(entry[v]["us_median"] / base["us_median"], 4)
        except (OSError, subprocess.SubprocessError, RuntimeError, KeyError) as e:
            res["trace_error"] = f"K1={K1}: {type(e).__name__}: {e}"
            break                                                            # a step failed: nothing more is started on the GPU
        finally:
            shutil.rmtree(directory, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 1 if "trace_error" in res else 0


if __name__ == "__main__":
    sys.exit(main())
