#!/usr/bin/env python3
"""Time Mirostat v2 (asd_mirostat_rows: k_mirostat_lse + k_mirostat_chain) against the existing one-HBM-sweep in-place pass,
asd_entropy_cut_rows in epsilon mode, on bf16 tensors [32, 9, 152064] (a verifying step's output at B = 32, K = 8: 88 MB) and
[32, 1, 152064] (stage 0), N(0, 3^2) logits at T = 0.7, tau = 5, eta = 0.1, all in the same process on the same values:

  entropy_cut_eps_k9 / _k1   asd_entropy_cut_rows, epsilon_cutoff = 3e-4 on every row   -- the baseline
  mirostat_lse_k9 / _k1      k_mirostat_lse: the sweep over all B * K1 rows (the HBM read)
  mirostat_chain_k9 / _k1    k_mirostat_chain: B workgroups walk their K1 rows in order (proposals: each row's arg-max, so
                             that no chain ends early)
  mirostat_k9 / _k1          the two together, dispatch by dispatch

    python tools/bench_mirostat.py [--out profiles/mirostat.json] [--repeats 30]

Both passes work in place, so every round restores the tensor from a pristine copy before each launch (the copies are torch
kernels and are not counted).  Kernel time comes from a `rocprofv3 --kernel-trace --stats` run OF ITS OWN (no counters, no other
tracing): this script starts itself once more under the profiler as a fresh child process (`--worker`) before it touches the
GPU; the child is the tool's one GPU step and runs under its own time limit; a failure of it ends the tool.  The child launches
the four calls in alternation, `--repeats` times after 3 warm-up rounds.  Reported per variant: the median, minimum, maximum and
quartiles over the repeats, the ratios of the medians to the baseline's, and the baseline's spread ((max - min) / median and
(p75 - p25) / median).  This is a measurement, not a pass mark.  Needs a GPU: there is no fallback."""
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
SHAPES = ("k9", "k1")
VARIANTS = tuple(f"{v}_{s}" for s in SHAPES for v in ("entropy_cut_eps", "mirostat_lse", "mirostat_chain", "mirostat"))
EPSILON, TEMPERATURE, TAU, ETA = 3e-4, 0.7, 5.0, 0.1
STEP_LIMIT_S = 600


def worker(a) -> int:
    import torch
    from asd_amd import kernels as K
    B, K1, V = a.batch, a.rows, a.vocab
    g = torch.Generator(device="cuda").manual_seed(1)
    x9_0 = (torch.randn((B, K1, V), generator=g, device="cuda") * 3.0).to(torch.bfloat16)
    x1_0 = x9_0[:, 0].clone()
    x9, x1 = x9_0.clone(), x1_0.clone()
    tok = x9_0[:, :K1 - 1].float().argmax(-1).to(torch.int32).contiguous()
    inv_t = 1.0 / TEMPERATURE
    eps = K.pack_entropy_cut([inv_t] * B, [K.CUT_EPSILON] * B, [EPSILON] * B, "cuda")
    miro = K.pack_mirostat([inv_t] * B, [TAU] * B, [ETA] * B, "cuda")
    # a sane answer before any timing: row 0's kept set against torch on two sequences (away from the bound), a live chain
    s = -torch.log_softmax(x9_0[:2, 0].double() * inv_t, -1) / 0.6931471805599453
    path = K.mirostat_rows(x9, miro, tok)
    kept = ~torch.isinf(x9[:2, 0])
    sure = (s - 2 * TAU).abs() > 1e-3
    assert torch.equal(kept[sure], (s <= 2 * TAU)[sure])
    assert bool((path[:, 1:] != path[:, :-1]).all())
    torch.cuda.synchronize()
    for _ in range(WARMUP + a.repeats):
        x9.copy_(x9_0)
        K.entropy_cut_rows(x9, eps)
        x9.copy_(x9_0)
        K.mirostat_rows(x9, miro, tok)
        x1.copy_(x1_0)
        K.entropy_cut_rows(x1, eps)
        x1.copy_(x1_0)
        K.mirostat_rows(x1, miro)
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
    by = lambda key: [(e - s) / 1e3 for s, e, name in rows if key in name.replace(" ", "")]      # noqa: E731
    cuts, lse, chain = by("k_entropy_cut_rows"), by("k_mirostat_lse"), by("k_mirostat_chain")
    rounds = WARMUP + repeats
    # the check ahead of the loop launches Mirostat once; a round launches eps, Mirostat (K1 rows), eps, Mirostat (one row)
    if len(cuts) != 2 * rounds or len(lse) != 1 + 2 * rounds or len(chain) != 1 + 2 * rounds:
        raise RuntimeError(f"{len(cuts)} asd_entropy_cut_rows, {len(lse)} k_mirostat_lse and {len(chain)} k_mirostat_chain dispatches "
                           f"in the trace, expected {2 * rounds}, {1 + 2 * rounds} and {1 + 2 * rounds}")
    out = {}
    for i, s in enumerate(SHAPES):
        out[f"entropy_cut_eps_{s}"], out[f"mirostat_lse_{s}"], out[f"mirostat_chain_{s}"] = cuts[i::2], lse[1 + i::2], chain[1 + i::2]
        out[f"mirostat_{s}"] = [p + q for p, q in zip(out[f"mirostat_lse_{s}"], out[f"mirostat_chain_{s}"])]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mirostat.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rows", type=int, default=9, help="K1: rows per sequence (draft_len + 1)")
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--trace-dir", default=None, help="keep the profiler's output here (default: a temporary directory)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)

    res = {"what": "asd_mirostat_rows (tau = 5, eta = 0.1; T = 0.7; N(0, 3^2) logits; proposals: the rows' arg-max) vs "
                   "asd_entropy_cut_rows (epsilon_cutoff = 3e-4) on [B, K1, V] and [B, 1, V] bf16 tensors: kernel time from a "
                   "rocprofv3 --kernel-trace --stats run of its own, the four calls launched in alternation in one process, the "
                   "tensor restored before every call",
           "B": a.batch, "K1": a.rows, "V": a.vocab, "dtype": "bf16", "rows": a.batch * a.rows,
           "logit_bytes": a.batch * a.rows * a.vocab * 2, "repeats": a.repeats, "warmup_rounds": WARMUP}
    keep = a.trace_dir is not None
    directory = os.path.abspath(a.trace_dir) if keep else tempfile.mkdtemp(prefix="mirostat_trace_")
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
        for s in SHAPES:
            base = res[f"entropy_cut_eps_{s}"]
            res[f"entropy_cut_eps_{s}_spread"] = round((base["us_max"] - base["us_min"]) / base["us_median"], 4)
            res[f"entropy_cut_eps_{s}_quartile_spread"] = round((base["us_p75"] - base["us_p25"]) / base["us_median"], 4)
            res[f"mirostat_over_entropy_cut_eps_{s}"] = round(res[f"mirostat_{s}"]["us_median"] / base["us_median"], 4)
            res[f"chain_over_entropy_cut_eps_{s}"] = round(res[f"mirostat_chain_{s}"]["us_median"] / base["us_median"], 4)
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
