#!/usr/bin/env python3
"""Time the tail-free pass (asd_tail_free_rows: a per-row radix sort and a scan over the sorted row) against the entropy-cut pass
in typical mode -- the costliest existing cut -- on one bf16 tensor [32, K1, 152064] for K1 = 9 (a verifying step's output at
B = 32, K = 8: 88 MB) and K1 = 1 (stage 0), both in the same process on copies of the same values:

  entropy_cut_typical   asd_entropy_cut_rows, typical_p = 0.9 on every row   -- the baseline: three histogram sweeps and a cut sweep
  tail_free             asd_tail_free_rows, tfs = 0.95 on every row          -- statistics, two sort passes, the f64 scan, the cut sweep

    python tools/bench_tail_free.py [--out profiles/tail_free.json] [--repeats 30]

The cuts work in place, so every round restores the tensor from a pristine copy before each launch (the copies are torch
kernels and are not counted).  Kernel time comes from a `rocprofv3 --kernel-trace --stats` run OF ITS OWN per K1 (no counters,
no other tracing): this script starts itself once more under the profiler as a fresh child process (`--worker`) before it
touches the GPU; each child is one GPU step under its own time limit, and a failure ends the tool.  A child launches the two in
alternation, `--repeats` times after 3 warm-up rounds.  Reported per K1 and variant: the median, minimum, maximum and quartiles
over the repeats, the ratio of the medians, the baseline's spread ((max - min) / median and (p75 - p25) / median) and the
workspace's size; and the wall time of a 64-token sampled stage-0 call at B = 8 at the Qwen2.5-7B shape with tfs off and on
(a child process of its own, without the profiler).  This is a measurement, not a pass mark.  Needs a GPU: there is no fallback."""
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

VARIANTS = ("entropy_cut_typical", "tail_free")
KERNELS = ("k_entropy_cut_rows", "k_tail_free_rows")
TYPICAL_P, TFS, TEMPERATURE = 0.9, 0.95, 0.7
STEP_LIMIT_S, WALL_LIMIT_S, TOKENS, WALL_B = 300, 900, 64, 8


def worker(a) -> int:
    import torch
    from asd_amd import kernels as K
    B, K1, V = a.batch, a.rows, a.vocab
    g = torch.Generator(device="cuda").manual_seed(1)
    x0 = (torch.randn((B, K1, V), generator=g, device="cuda") * 3.0).to(torch.bfloat16)
    x = x0.clone()
    inv_t = 1.0 / TEMPERATURE
    typ = K.pack_entropy_cut([inv_t] * B, [K.CUT_TYPICAL] * B, [TYPICAL_P] * B, "cuda")
    tfs = K.pack_tail_free([inv_t] * B, [TFS] * B, "cuda")
    # a sane answer before any timing: row (0, 0) against torch in f64
    K.tail_free_rows(x, tfs)
    r = x0[0, 0].double().sort(descending=True).values
    w = ((r - r[0]) * float(torch.tensor(inv_t, dtype=torch.float32))).exp()
    d2 = (w[:-1] - w[1:]).diff().abs()
    c = d2.cumsum(0)
    i_star = int((c > float(torch.tensor(TFS, dtype=torch.float32)) * c[-1]).nonzero()[0])
    assert torch.equal(~torch.isinf(x[0, 0]), x0[0, 0].double() >= r[i_star])
    torch.cuda.synchronize()
    for _ in range(WARMUP + a.repeats):
        x.copy_(x0)
        K.entropy_cut_rows(x, typ)
        x.copy_(x0)
        K.tail_free_rows(x, tfs)
    torch.cuda.synchronize()
    return 0


def wall_worker(a) -> int:
    import torch
    from asd_amd.serving.stages import StageConfig, StageManager
    stage = StageManager([StageConfig(model_name="qwen2.5-7b", model_size="8b", cost_per_token=1.0)]).get_stage("8b")
    prompts = [f"request {i} : the quick brown fox jumps over the lazy dog ." for i in range(WALL_B)]
    calls = (("tfs_off", {}), ("tfs_on", dict(tfs=TFS)))
    out = {"B": WALL_B, "tokens": TOKENS, "temperature": TEMPERATURE, "tfs": TFS}
    for name, kw in calls:                                                   # warm both routes: code objects, library plans
        stage.generate(prompts=prompts, max_tokens=4, temperature=TEMPERATURE, seed=list(range(WALL_B)), **kw)
    for name, kw in calls * 3:
        texts, _, stats = stage.generate(prompts=prompts, max_tokens=TOKENS, temperature=TEMPERATURE, seed=list(range(WALL_B)), **kw)
        torch.cuda.synchronize()
        assert [len(t.split()) for t in texts] == [TOKENS] * WALL_B
        out.setdefault(name, []).append(round(stats["generation_time_ms"], 1))
    out = {k: ({"ms_median": statistics.median(v), "ms_all": v} if isinstance(v, list) else v) for k, v in out.items()}
    out["on_over_off"] = round(out["tfs_on"]["ms_median"] / out["tfs_off"]["ms_median"], 4)
    with open(a.wall_out, "w") as f:
        json.dump(out, f)
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
    out = {}
    for v, kernel, extra in zip(VARIANTS, KERNELS, (0, 1)):                  # the check ahead of the loop launches one tail-free cut
        t = [(e - s) / 1e3 for s, e, name in rows if kernel in name.replace(" ", "")]
        if len(t) != WARMUP + repeats + extra:
            raise RuntimeError(f"{len(t)} {kernel} dispatches in the trace, expected {WARMUP + repeats + extra}")
        out[v] = t[-repeats:]
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tail_free.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rows", type=int, default=9, help=argparse.SUPPRESS)
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

    res = {"what": "asd_tail_free_rows (tfs = 0.95; T = 0.7; N(0, 3^2) logits) vs asd_entropy_cut_rows (typical_p = 0.9) on copies "
                   "of one [B, K1, V] bf16 tensor: kernel time from a rocprofv3 --kernel-trace --stats run of its own per K1, the "
                   "two launched in alternation in one process, the tensor restored before every cut",
           "B": a.batch, "V": a.vocab, "dtype": "bf16", "repeats": a.repeats, "warmup_rounds": WARMUP,
           "kernel": {"threads": 1024, "vgprs": 54, "lds_bytes": 16776, "scratch_bytes": 0}}
    for K1 in (9, 1):
        key_bytes = (a.vocab * 2 + 255) // 256 * 256
        entry = res[f"K1={K1}"] = {"rows": a.batch * K1, "logit_bytes": a.batch * K1 * a.vocab * 2,
                                   "workspace_bytes": a.batch * K1 * 2 * key_bytes}
        directory = tempfile.mkdtemp(prefix="tail_free_trace_")
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
            base = entry[VARIANTS[0]]
            entry["baseline_spread"] = round((base["us_max"] - base["us_min"]) / base["us_median"], 4)
            entry["baseline_quartile_spread"] = round((base["us_p75"] - base["us_p25"]) / base["us_median"], 4)
            entry["tail_free_over_baseline"] = round(entry["tail_free"]["us_median"] / base["us_median"], 4)
        except (OSError, subprocess.SubprocessError, RuntimeError, KeyError) as e:
            res["trace_error"] = f"K1={K1}: {type(e).__name__}: {e}"
            break                                                            # a step failed: nothing more is started on the GPU
        finally:
            shutil.rmtree(directory, ignore_errors=True)
    if "trace_error" not in res:                                             # the end-to-end call: its own process, no profiler
        fd, path = tempfile.mkstemp(prefix="tail_free_wall_", suffix=".json")
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
