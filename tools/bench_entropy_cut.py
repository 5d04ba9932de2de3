#!/usr/bin/env python3
"""Time the entropy-cut pass (asd_entropy_cut_rows) against the one-sweep pass that forms the same sums, on one bf16 tensor
[32, 9, 152064] (a verifying step's output at B = 32, K = 8: 88 MB), all in the same process on the same values:

  token_stats_n0     asd_token_stats, N = 0, every row live   -- the baseline: one sweep, (m2, s, u) and the arg-max
  entropy_cut_eps    asd_entropy_cut_rows, epsilon_cutoff = 3e-4 on every row   -- sweep 1 and one compare-and-store sweep
  entropy_cut_typ    asd_entropy_cut_rows, typical_p = 0.9 on every row         -- sweep 1, three histogram sweeps, one store sweep

    python tools/bench_entropy_cut.py [--out profiles/entropy_cut.json] [--repeats 30]

The cut works in place, so every round restores the tensor from a pristine copy before each of the two launches (the copies are
torch kernels and are not counted).  Kernel time comes from a `rocprofv3 --kernel-trace --stats` run OF ITS OWN (no counters, no
other tracing): this script starts itself once more under the profiler as a fresh child process (`--worker`) before it touches
the GPU; the child is the tool's one GPU step and runs under its own time limit; a failure of it ends the tool.  The child
launches the three in alternation, `--repeats` times after 3 warm-up rounds; the two asd_entropy_cut_rows dispatches of a round
are told apart by their position in it.  Reported per variant: the median, minimum, maximum and quartiles over the repeats, the
two ratios of the medians to the baseline's, and the baseline's spread ((max - min) / median and (p75 - p25) / median).  This is
a measurement, not a pass mark.  Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import shutil
import signal
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP = 3
VARIANTS = ("token_stats_n0", "entropy_cut_eps", "entropy_cut_typ")
EPSILON, TYPICAL_P, TEMPERATURE = 3e-4, 0.9, 0.7
STEP_LIMIT_S = 600


def worker(a) -> int:
    import torch
    from asd_amd import kernels as K
    B, K1, V = a.batch, a.rows, a.vocab
    g = torch.Generator(device="cuda").manual_seed(1)
    x0 = (torch.randn((B, K1, V), generator=g, device="cuda") * 3.0).to(torch.bfloat16)
    x = x0.clone()
    tok = torch.randint(0, V, (B, K1 - 1), generator=g, device="cuda", dtype=torch.int32)
    drawn = torch.randint(0, V, (B,), generator=g, device="cuda", dtype=torch.int32)
    full = torch.full((B,), K1 - 1, device="cuda", dtype=torch.int32)
    inv_t = 1.0 / TEMPERATURE
    s0 = K.TokenStats(B, K1, V, torch.bfloat16, 0)
    eps = K.pack_entropy_cut([inv_t] * B, [K.CUT_EPSILON] * B, [EPSILON] * B, "cuda")
    typ = K.pack_entropy_cut([inv_t] * B, [K.CUT_TYPICAL] * B, [TYPICAL_P] * B, "cuda")
    # sane answers before any timing: epsilon's kept set against torch on two sequences (away from the bound), and typical-p keeps
    # at least the mass it was asked for
    p = torch.softmax(x0[:2].double() * inv_t, -1)
    K.entropy_cut_rows(x, eps)
    kept = ~torch.isinf(x[:2])
    sure = ((p / EPSILON).log().abs() > 1e-3)
    assert torch.equal(kept[sure], (p >= EPSILON)[sure])
    x.copy_(x0)
    K.entropy_cut_rows(x, typ)
    mass = (p * ~torch.isinf(x[:2])).sum(-1)
    assert bool((mass >= TYPICAL_P - 1e-4).all()) and bool((mass < 1.0 - 1e-6).all())
    s0(x0, tok, full, drawn)
    torch.cuda.synchronize()
    for _ in range(WARMUP + a.repeats):
        s0(x0, tok, full, drawn)
        x.copy_(x0)
        K.entropy_cut_rows(x, eps)
        x.copy_(x0)
        K.entropy_cut_rows(x, typ)
    torch.cuda.synchronize()
    return 0


def _column(fields, *names):
    low = {f.lower(): f for f in fields}
    for n in names:
        if n in low:
            return low[n]
    raise KeyError(f"none of {names} among the trace's columns {fields}")


def parse_trace(directory, repeats):
    """The kernel-trace CSV(s) under `directory` -> {variant: [kernel time in us of the last `repeats` dispatches]}."""
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
    stats = [(e - s) / 1e3 for s, e, name in rows if "k_token_stats" in name.replace(" ", "")]
    cuts = [(e - s) / 1e3 for s, e, name in rows if "k_entropy_cut_rows" in name.replace(" ", "")]
    rounds = WARMUP + repeats
    # the checks ahead of the loop launch the baseline once and the cut twice; a round launches stats, eps, typ
    if len(stats) != 1 + rounds or len(cuts) != 2 + 2 * rounds:
        raise RuntimeError(f"{len(stats)} asd_token_stats and {len(cuts)} asd_entropy_cut_rows dispatches in the trace, expected "
                           f"{1 + rounds} and {2 + 2 * rounds}")
    out = {"token_stats_n0": stats[1:], "entropy_cut_eps": cuts[2::2], "entropy_cut_typ": cuts[3::2]}
    return {v: t[-repeats:] for v, t in out.items()}


def run_step(cmd, limit_s) -> None:
    """One GPU step in a session of its own: when the limit runs out the whole process group is ended -- the profiler AND the
    worker under it that holds the GPU -- not the profiler alone.  A non-zero exit raises like subprocess.run(check=True)."""
    proc = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, start_new_session=True)
    try:
        rc = proc.wait(timeout=limit_s)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        proc.wait()
        raise
    if rc != 0:
        raise subprocess.CalledProcessError(rc, cmd)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "entropy_cut.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rows", type=int, default=9, help="K1: rows per sequence (draft_len + 1)")
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--trace-dir", default=None, help="keep the profiler's output here (default: a temporary directory)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)

    res = {"what": "asd_entropy_cut_rows (epsilon_cutoff = 3e-4; typical_p = 0.9; T = 0.7; N(0, 3^2) logits) vs asd_token_stats "
                   "(N = 0, every row live) on one [B, K1, V] bf16 tensor: kernel time from a rocprofv3 --kernel-trace --stats run "
                   "of its own, the three launched in alternation in one process, the tensor restored before every cut",
           "B": a.batch, "K1": a.rows, "V": a.vocab, "dtype": "bf16", "rows": a.batch * a.rows,
           "logit_bytes": a.batch * a.rows * a.vocab * 2, "repeats": a.repeats, "warmup_rounds": WARMUP}
    keep = a.trace_dir is not None
    directory = os.path.abspath(a.trace_dir) if keep else tempfile.mkdtemp(prefix="entropy_cut_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", directory, "--", sys.executable,
           os.path.abspath(__file__), "--worker", "--batch", str(a.batch), "--rows", str(a.rows), "--vocab", str(a.vocab),
           "--repeats", str(a.repeats)]
    try:
        run_step(cmd, STEP_LIMIT_S)                                          # the one GPU step, under its own limit
        times = parse_trace(directory, a.repeats)
        for v in VARIANTS:
            t = times[v]
            med = statistics.median(t)
            q = statistics.quantiles(t, n=4)
            res[v] = {"us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                      "us_p25": round(q[0], 2), "us_p75": round(q[2], 2)}
        base = res["token_stats_n0"]
        res["token_stats_n0_spread"] = round((base["us_max"] - base["us_min"]) / base["us_median"], 4)
        res["token_stats_n0_quartile_spread"] = round((base["us_p75"] - base["us_p25"]) / base["us_median"], 4)
        res["eps_over_token_stats_n0"] = round(res["entropy_cut_eps"]["us_median"] / base["us_median"], 4)
        res["typ_over_token_stats_n0"] = round(res["entropy_cut_typ"]["us_median"] / base["us_median"], 4)
    except (OSError, subprocess.SubprocessError, RuntimeError, KeyError) as e:
        res["trace_error"] = f"{type(e).__name__}: {e}"
    finally:
        if not keep:
            shutil.rmtree(directory, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 1 if "trace_error" in res else 0


if __name__ == "__main__":
    sys.exit(main())
