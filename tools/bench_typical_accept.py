#!/usr/bin/env python3
"""Time typical acceptance (asd_typical_accept: the sweep and the finish) against the lossless verify (asd_verify_accept) on the
same bf16 logits [B, 8, 152064] in the same process, for B = 32, 8 and 1 -- the two read the same bytes once, so the verify
kernel's stream is the floor for this one:

  verify_accept         asd_verify_accept_ex, its own heuristic geometry        -- the baseline
  typical_auto          asd_typical_accept, splits = 0 (chosen from the CU count)
  typical_splits1       asd_typical_accept, splits = 1

    python tools/bench_typical_accept.py [--out profiles/typical_accept.json] [--repeats 30]

Neither call writes the logits, so nothing is restored between launches.  Kernel time comes from a `rocprofv3 --kernel-trace
--stats` run OF ITS OWN per B (no counters, no other tracing): this script starts itself once more under the profiler as a fresh
child process (`--worker`) before it touches the GPU; each child is one GPU step under its own time limit, and a failure ends
the tool.  A child launches the three in alternation, `--repeats` times after 3 warm-up rounds; a call's time is the sum of its
kernels' times.  Reported per B and variant: the median, minimum, maximum and quartiles over the repeats, the ratios of the
medians to the baseline's and the baseline's spread ((max - min) / median and (p75 - p25) / median); and, in a child process of
its own without the profiler, 64 sampled tokens at B = 8 at the Qwen2.5-7B shape under prompt lookup (K = 8) with typical
acceptance off and on: wall time, steps per call and typical_accepted / typical_proposed.  This is a measurement, not a pass
mark.  Needs a GPU: there is no fallback."""
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

VARIANTS = ("verify_accept", "typical_auto", "typical_splits1")
K, EPS, ALPHA, TEMPERATURE = 8, 0.09, 0.3, 0.7
STEP_LIMIT_S, WALL_LIMIT_S, TOKENS, WALL_B = 300, 900, 64, 8


def worker(a) -> int:
    import torch
    from asd_amd import kernels as Kn
    B, V = a.batch, a.vocab
    g = torch.Generator(device="cuda").manual_seed(1)
    x = (torch.randn((B, K, V), generator=g, device="cuda") * 3.0).to(torch.bfloat16)
    tok = torch.randint(0, V, (B, K), generator=g, device="cuda").to(torch.int32)
    lp_d = torch.full((B, K), -5.0, device="cuda")
    u = torch.rand((B, K), generator=g, device="cuda")
    inv_t = 1.0 / TEMPERATURE
    ws = Kn.VerifyWorkspace(B, K, V, torch.bfloat16)
    packed = Kn.pack_typical_accept([inv_t] * B, [EPS] * B, [ALPHA] * B, "cuda")
    # a sane answer before any timing: row (0, 0) of both geometries against torch in f64
    y = x[0, 0].double() * float(torch.tensor(inv_t, dtype=torch.float32))
    lsm = torch.log_softmax(y, 0)
    for splits in (0, 1):
        lp, H, _, _ = Kn.typical_accept(x, tok, packed, splits=splits)
        assert abs(float(lp[0, 0]) - float(lsm[tok[0, 0]])) < 2e-5 and abs(float(H[0, 0]) + float((lsm.exp() * lsm).sum())) < 1e-4
    torch.cuda.synchronize()
    for _ in range(WARMUP + a.repeats):
        Kn.verify_accept(x, tok, lp_d, u, ws, inv_temperature=inv_t)
        Kn.typical_accept(x, tok, packed, splits=0)
        Kn.typical_accept(x, tok, packed, splits=1)
    torch.cuda.synchronize()
    return 0


def wall_worker(a) -> int:
    import torch
    from asd_amd.serving.stages import StageConfig, StageManager
    stage = StageManager([StageConfig(model_name="qwen2.5-7b", model_size="8b", cost_per_token=1.0)]).get_stage("8b")
    prompts = [f"request {i} : the quick brown fox jumps over the lazy dog . the quick brown fox jumps" for i in range(WALL_B)]
    base = dict(prompts=prompts, temperature=TEMPERATURE, seed=list(range(WALL_B)), top_p=1.0, prompt_lookup_num_tokens=K)
    calls = (("typical_off", {}), ("typical_on", dict(typical_acceptance_threshold=EPS, typical_acceptance_alpha=ALPHA)))
    out = {"B": WALL_B, "tokens": TOKENS, "temperature": TEMPERATURE, "eps": EPS, "alpha": ALPHA, "prompt_lookup_num_tokens": K}
    for name, kw in calls:                                                   # warm both routes: code objects, library plans
        stage.generate(max_tokens=4, **base, **kw)
    for name, kw in calls * 3:
        texts, _, stats = stage.generate(max_tokens=TOKENS, **base, **kw)
        torch.cuda.synchronize()
        assert [len(t.split()) for t in texts] == [TOKENS] * WALL_B
        out.setdefault(name, []).append(round(stats["generation_time_ms"], 1))
        out[name + "_steps"] = stats["steps"]
        if "typical_accepted" in stats:
            out["typical_accepted"], out["typical_proposed"] = sum(stats["typical_accepted"]), sum(stats["typical_proposed"])
    out = {k: ({"ms_median": statistics.median(v), "ms_all": v} if isinstance(v, list) else v) for k, v in out.items()}
    out["on_over_off"] = round(out["typical_on"]["ms_median"] / out["typical_off"]["ms_median"], 4)
    out["accepted_over_proposed"] = round(out["typical_accepted"] / max(out["typical_proposed"], 1), 4)
    with open(a.wall_out, "w") as f:
        json.dump(out, f)
    return 0


def parse_trace(directory, repeats):
    """The kernel-trace CSV(s) under `directory` -> {variant: [time in us of the last `repeats` calls, a call's kernels summed]}."""
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
    times = lambda kernel: [(e - s) / 1e3 for s, e, name in rows if kernel in name.replace(" ", "")]   # noqa: E731
    n = WARMUP + repeats
    verify = [t for t in (times("k_verify"), times("k_accept_from_partials")) if t]      # the second only where the rows are split
    if not verify or any(len(t) != n for t in verify):
        raise RuntimeError(f"{[len(t) for t in verify]} verify dispatches in the trace, expected {n}")
    sweep, finish = times("k_typical_sweep"), times("k_typical_finish")
    if len(sweep) != 2 * (n + 1) or len(finish) != 2 * (n + 1):                          # (the check ahead of the loop: one pair)
        raise RuntimeError(f"{len(sweep)} / {len(finish)} typical-acceptance dispatches in the trace, expected {2 * (n + 1)}")
    both = [s + f for s, f in zip(sweep, finish)]
    return {"verify_accept": [sum(t) for t in zip(*verify)][-repeats:], "typical_auto": both[0::2][-repeats:],
            "typical_splits1": both[1::2][-repeats:], "typical_auto_sweep_only": sweep[0::2][-repeats:]}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "typical_accept.json"))
    ap.add_argument("--batch", type=int, default=32, help=argparse.SUPPRESS)
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--wall-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--wall-out", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if a.wall_worker:
        return wall_worker(a)

    res = {"what": "asd_typical_accept (eps 0.09, alpha 0.3, T = 0.7; N(0, 3^2) logits; sweep + finish summed) vs asd_verify_accept_ex "
                   "on one [B, 8, V] bf16 tensor: kernel time from a rocprofv3 --kernel-trace --stats run of its own per B, the "
                   "three launched in alternation in one process",
           "K": K, "V": a.vocab, "dtype": "bf16", "repeats": a.repeats, "warmup_rounds": WARMUP}
    for B in (32, 8, 1):
        entry = res[f"B={B}"] = {"rows": B * K, "logit_bytes": B * K * a.vocab * 2}
        directory = tempfile.mkdtemp(prefix="typical_accept_trace_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", directory, "--", sys.executable,
               os.path.abspath(__file__), "--worker", "--batch", str(B), "--vocab", str(a.vocab), "--repeats", str(a.repeats)]
        try:
            run_step(cmd, STEP_LIMIT_S)                                      # one GPU step, under its own limit
            for v, t in parse_trace(directory, a.repeats).items():
                q = statistics.quantiles(t, n=4)
                entry[v] = {"us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                            "us_p25": round(q[0], 2), "us_p75": round(q[2], 2)}
            base = entry[VARIANTS[0]]
            entry["baseline_spread"] = round((base["us_max"] - base["us_min"]) / base["us_median"], 4)
            entry["baseline_quartile_spread"] = round((base["us_p75"] - base["us_p25"]) / base["us_median"], 4)
            for v in VARIANTS[1:]:
                entry[v + "_over_baseline"] = round(entry[v]["us_median"] / base["us_median"], 4)
            entry["auto_over_splits1"] = round(entry["typical_auto"]["us_median"] / entry["typical_splits1"]["us_median"], 4)
        except (OSError, subprocess.SubprocessError, RuntimeError, KeyError) as e:
            res["trace_error"] = f"B={B}: {type(e).__name__}: {e}"
            break                                                            # a step failed: nothing more is started on the GPU
        finally:
            shutil.rmtree(directory, ignore_errors=True)
    if "trace_error" not in res:                                             # the end-to-end call: its own process, no profiler
        fd, path = tempfile.mkstemp(prefix="typical_accept_wall_", suffix=".json")
        os.close(fd)
        try:
            run_step([sys.executable, os.path.abspath(__file__), "--wall-worker", "--wall-out", path], WALL_LIMIT_S)
            with open(path) as f:
                res["wall_64_tokens_B8"] = json.load(f)
        except (OSError, subprocess.SubprocessError, ValueError) as e:
            res["trace_error"] = f"wall: {type(e).__name__}: {e}"
        finally:
            os.unlink(path)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 1 if "trace_error" in res else 0


if __name__ == "__main__":
    sys.exit(main())
