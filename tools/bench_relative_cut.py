#!/usr/bin/env python3
"""Time the relative-cut pass (asd_relative_cut_rows) against the entropy-cut pass in epsilon mode, on one bf16 tensor
[32, K1, 152064] for K1 = 9 (a verifying step's output at B = 32, K = 8: 88 MB) and K1 = 1 (stage 0), all variants of a K1 in
the same process on copies of the same values:

  entropy_cut_eps   asd_entropy_cut_rows, epsilon_cutoff = 3e-4 on every row   -- the baseline: a statistics sweep and a cut sweep
  top_n_sigma       asd_relative_cut_rows, n = 1 on every row                  -- mean, deviation and cut sweeps
  top_a             asd_relative_cut_rows, a = 0.2 on every row                -- (m2, s) and cut sweeps
  xtc_on            XTC, t = 0.02, every row's coin under q                    -- (m2, s), count / minimum and cut sweeps
  xtc_off           XTC, every row's coin above q                              -- a row leaves behind its record and coin

    python tools/bench_relative_cut.py [--out profiles/relative_cut.json] [--repeats 30]

The cuts work in place, so every round restores the tensor from a pristine copy before each launch (the copies are torch
kernels and are not counted).  Kernel time comes from a `rocprofv3 --kernel-trace --stats` run OF ITS OWN per K1 (no counters,
no other tracing): this script starts itself once more under the profiler as a fresh child process (`--worker`) before it
touches the GPU; each child is one GPU step under its own time limit, and a failure ends the tool.  A child launches the five
in alternation, `--repeats` times after 3 warm-up rounds; the four asd_relative_cut_rows dispatches of a round are told apart by
their position in it.  Reported per K1 and variant: the median, minimum, maximum and quartiles over the repeats, the ratio of
each median to the baseline's, and the baseline's spread ((max - min) / median and (p75 - p25) / median).  This is a
measurement, not a pass mark.  Needs a GPU: there is no fallback."""
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

VARIANTS = ("entropy_cut_eps", "top_n_sigma", "top_a", "xtc_on", "xtc_off")
EPSILON, N_SIGMA, TOP_A, XTC_T, XTC_Q, TEMPERATURE = 3e-4, 1.0, 0.2, 0.02, 0.5, 0.7
STEP_LIMIT_S = 300


def worker(a) -> int:
    import torch
    from asd_amd import kernels as K
    B, K1, V = a.batch, a.rows, a.vocab
    g = torch.Generator(device="cuda").manual_seed(1)
    x0 = (torch.randn((B, K1, V), generator=g, device="cuda") * 3.0).to(torch.bfloat16)
    x = x0.clone()
    inv_t = 1.0 / TEMPERATURE
    eps = K.pack_entropy_cut([inv_t] * B, [K.CUT_EPSILON] * B, [EPSILON] * B, "cuda")
    rel = [K.pack_relative_cut([inv_t] * B, [m] * B, [v] * B, [q] * B, "cuda")
           for m, v, q in ((K.RELCUT_TOP_N_SIGMA, N_SIGMA, 0.0), (K.RELCUT_TOP_A, TOP_A, 0.0), (K.RELCUT_XTC, XTC_T, XTC_Q))]
    under = torch.zeros((B, K1), dtype=torch.float32, device="cuda")
    above = torch.full((B, K1), 0.75, dtype=torch.float32, device="cuda")
    launches = [(rel[0], None), (rel[1], None), (rel[2], under), (rel[2], above)]
    # sane answers before any timing: top-n-sigma's kept set against torch on two sequences, away from the threshold
    K.relative_cut_rows(x, *launches[0])
    r = x0[:2].double()
    thr = r.amax(-1, keepdim=True) - N_SIGMA * r.std(-1, unbiased=False, keepdim=True)
    sure = (r - thr).abs() > 1e-3
    assert torch.equal((~torch.isinf(x[:2]))[sure], (r >= thr)[sure])
    torch.cuda.synchronize()
    for _ in range(WARMUP + a.repeats):
        x.copy_(x0)
        K.entropy_cut_rows(x, eps)
        for packed, coins in launches:
            x.copy_(x0)
            K.relative_cut_rows(x, packed, coins)
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
    base = [(e - s) / 1e3 for s, e, name in rows if "k_entropy_cut_rows" in name.replace(" ", "")]
    cuts = [(e - s) / 1e3 for s, e, name in rows if "k_relative_cut_rows" in name.replace(" ", "")]
    rounds = WARMUP + repeats
    if len(base) != rounds or len(cuts) != 1 + 4 * rounds:                   # the check ahead of the loop launches one cut
        raise RuntimeError(f"{len(base)} asd_entropy_cut_rows and {len(cuts)} asd_relative_cut_rows dispatches in the trace, "
                           f"expected {rounds} and {1 + 4 * rounds}")
    out = {"entropy_cut_eps": base}
    out.update({v: cuts[1 + i::4] for i, v in enumerate(VARIANTS[1:])})
    return {v: t[-repeats:] for v, t in out.items()}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relative_cut.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rows", type=int, default=9, help=argparse.SUPPRESS)
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)

    res = {"what": "asd_relative_cut_rows (top_n_sigma = 1; top_a = 0.2; XTC t = 0.02 with every coin under / above q; T = 0.7; "
                   "N(0, 3^2) logits) vs asd_entropy_cut_rows (epsilon_cutoff = 3e-4) on copies of one [B, K1, V] bf16 tensor: "
                   "kernel time from a rocprofv3 --kernel-trace --stats run of its own per K1, the five launched in alternation "
                   "in one process, the tensor restored before every cut",
           "B": a.batch, "V": a.vocab, "dtype": "bf16", "repeats": a.repeats, "warmup_rounds": WARMUP}
    for K1 in (9, 1):
        entry = res[f"K1={K1}"] = {"rows": a.batch * K1, "logit_bytes": a.batch * K1 * a.vocab * 2}
        directory = tempfile.mkdtemp(prefix="relative_cut_trace_")
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
            base = entry["entropy_cut_eps"]
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
