#!/usr/bin/env python3
"""Time the guidance pass (asd_cfg_rows, scale 1.5, every sequence guided) on bf16 tensors [B, K1, 152064] -- B conditional and B
unconditional sequences, N(0, 3^2) logits -- for B in (1, 32) and K1 in (1, 9), beside
  quadratic   asd_logit_shape_rows, f = 0.3, c = 1, on a copy of the conditional tensor -- the closest existing kernel: one
              1024-lane workgroup per row, one row read and one written.  asd_cfg_rows moves 1.5 x its bytes (two reads, one
              write): that is the ratio to hold the medians against, not a threshold
  torch       log_softmax(c) and log_softmax(u) in the tensors' dtype, then u' + s (c' - u'): the expression it replaces; the
              SUM of the kernel times of its dispatches, the gaps between them not counted
And the wall time of a 64-token greedy stage-0 call at B = 8 at the Qwen2.5-7B shape with guidance on every row and with
guidance off: what the doubled batch costs in the model passes themselves.

    python tools/bench_cfg.py [--out profiles/cfg.json] [--repeats 30]

Kernel time comes from a `rocprofv3 --kernel-trace --stats` run OF ITS OWN per (B, K1) (no counters, no other tracing): this
script starts itself once more under the profiler as a fresh child process (`--worker`) before it touches the GPU; each child is
one GPU step under its own time limit, and a failure ends the tool.  A child runs, `--repeats` times after 3 warm-up rounds:
the torch expression, a restore of the conditional tensor, asd_cfg_rows, a restore, asd_logit_shape_rows.  The wall times are a
child of their own without the profiler (`--wall-worker`).  Reported per shape: the median, minimum, maximum and quartiles of the
three, the ratios of the medians, the baseline's spread and the bytes each kernel must move.  This is a measurement, not a pass
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

from bench_entropy_cut import WARMUP, _column, run_step  # noqa: E402

V, SCALE, FACTOR, CURVE, TEMPERATURE = 152064, 1.5, 0.3, 1.0, 0.7
SHAPES = tuple((b, k1) for b in (1, 32) for k1 in (1, 9))
STEP_LIMIT_S, WALL_LIMIT_S, TOKENS, WALL_B = 300, 900, 64, 8
CFG, QUAD = "k_cfg_rows", "k_logit_shape_rows"


def worker(a) -> int:
    import torch
    from asd_amd import kernels as K
    B, K1 = a.batch, a.rows
    g = torch.Generator(device="cuda").manual_seed(1)
    c0, u = ((torch.randn((B, K1, V), generator=g, device="cuda") * 3.0).to(torch.bfloat16) for _ in range(2))
    x, y = c0.clone(), c0.clone()
    cfg = K.pack_cfg([SCALE] * B, list(range(B)), "cuda")
    quad = K.pack_logit_shape([TEMPERATURE] * B, [K.SHAPE_QUADRATIC] * B, [FACTOR] * B, [CURVE] * B, "cuda")
    torch.cuda.synchronize()
    for _ in range(WARMUP + a.repeats):
        lc, lu = torch.log_softmax(c0, -1), torch.log_softmax(u, -1)
        ref = lu + SCALE * (lc - lu)
        x.copy_(c0)                                                                  # (the last dispatch in front of asd_cfg_rows)
        K.cfg_rows(x, u, cfg)
        y.copy_(c0)
        K.logit_shape_rows(y, quad)
    torch.cuda.synchronize()
    # a sane answer behind the timing: bf16 rounds each of torch's five passes, the kernel rounds once
    err = float((x.float() - ref.float()).abs().max())
    assert err <= 0.5, err
    return 0


def wall_worker(a) -> int:
    import torch
    from asd_amd.serving.stages import StageConfig, StageManager
    stage = StageManager([StageConfig(model_name="qwen2.5-7b", model_size="8b", cost_per_token=1.0)]).get_stage("8b")
    prompts = [f"request {i} : the quick brown fox jumps over the lazy dog ." for i in range(WALL_B)]
    calls = (("guidance_off", {}), ("guidance_on", dict(guidance_scale=2.0, negative_prompt="a dull and repetitive answer")))
    out = {"B": WALL_B, "tokens": TOKENS}
    for name, kw in calls:                                                           # warm both routes: code objects, library plans
        stage.generate(prompts=prompts, max_tokens=4, temperature=0.0, **kw)
    for name, kw in calls * 3:
        texts, _, stats = stage.generate(prompts=prompts, max_tokens=TOKENS, temperature=0.0, **kw)
        torch.cuda.synchronize()
        assert [len(t.split()) for t in texts] == [TOKENS] * WALL_B
        out.setdefault(name, []).append(round(stats["generation_time_ms"], 1))
    out = {k: ({"ms_median": statistics.median(v), "ms_all": v} if isinstance(v, list) else v) for k, v in out.items()}
    out["on_over_off"] = round(out["guidance_on"]["ms_median"] / out["guidance_off"]["ms_median"], 4)
    with open(a.wall_out, "w") as f:
        json.dump(out, f)
    return 0


def parse_trace(directory, repeats):
    """The kernel-trace CSV(s) under `directory` -> {"cfg" | "quadratic" | "torch": [kernel time in us of the last `repeats`
    rounds]}.  A round's torch time: every dispatch between the previous round's asd_logit_shape_rows and this round's
    asd_cfg_rows but the last, which is the restore."""
    import csv
    import glob
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rd = csv.DictReader(f)
            kn = _column(rd.fieldnames, "kernel_name")
            t0, t1 = _column(rd.fieldnames, "start_timestamp"), _column(rd.fieldnames, "end_timestamp")
            rows += [(int(r[t0]), int(r[t1]), r[kn].replace(" ", "")) for r in rd]
    if not rows:
        raise RuntimeError(f"no kernel trace under {directory}")
    rows.sort()
    at = {sym: [i for i, r in enumerate(rows) if sym in r[2]] for sym in (CFG, QUAD)}
    if any(len(v) != WARMUP + repeats for v in at.values()):
        raise RuntimeError(f"{len(at[CFG])} {CFG} and {len(at[QUAD])} {QUAD} dispatches in the trace, expected {WARMUP + repeats} each")
    us = lambda i: (rows[i][1] - rows[i][0]) / 1e3                                   # noqa: E731
    torch_us = [sum(us(i) for i in range(q + 1, c - 1)) for q, c in zip(at[QUAD][:-1], at[CFG][1:])]
    return {"cfg": [us(i) for i in at[CFG]][-repeats:], "quadratic": [us(i) for i in at[QUAD]][-repeats:], "torch": torch_us[-repeats:]}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cfg.json"))
    ap.add_argument("--batch", type=int, default=32, help=argparse.SUPPRESS)
    ap.add_argument("--rows", type=int, default=9, help=argparse.SUPPRESS)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--wall-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--wall-out", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if a.wall_worker:
        return wall_worker(a)

    res = {"what": "asd_cfg_rows (scale 1.5, every sequence guided, bf16 [B, K1, 152064] conditional and unconditional tensors, "
                   "N(0, 3^2) logits) vs asd_logit_shape_rows (quadratic, f = 0.3, c = 1) on a copy of the conditional tensor and vs "
                   "the torch expression (two log_softmax and the combine; the sum of its kernels' times): kernel time from a "
                   "rocprofv3 --kernel-trace --stats run of its own per shape, the three in alternation in one process, the "
                   "tensors restored before every pass; and the wall time of 64 greedy tokens at B = 8 at the Qwen2.5-7B shape "
                   "with guidance on every row and off",
           "V": V, "scale": SCALE, "repeats": a.repeats, "warmup_rounds": WARMUP,
           "resource_usage": {"k_cfg_rows resident bf16 / f16 / f32": "122 / 125 / 121 VGPRs, 72 SGPRs, 0 scratch, 268 B LDS, 4 waves/SIMD",
                              "k_cfg_rows streaming bf16 / f16 / f32": "46 / 49 / 47 VGPRs, 48 SGPRs, 0 scratch, 268 B LDS, 8 waves/SIMD"}}
    try:
        for B, K1 in SHAPES:
            row_bytes = B * K1 * V * 2
            entry = res[f"B={B},K1={K1}"] = {"cfg_bytes": 3 * row_bytes, "quadratic_bytes": 2 * row_bytes}
            directory = tempfile.mkdtemp(prefix="cfg_trace_")
            try:
                run_step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", directory, "--", sys.executable,
                          os.path.abspath(__file__), "--worker", "--batch", str(B), "--rows", str(K1), "--repeats", str(a.repeats)],
                         STEP_LIMIT_S)                                       # one GPU step, under its own limit
                for k, t in parse_trace(directory, a.repeats).items():
                    q = statistics.quantiles(t, n=4)
                    entry[k] = {"us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                                "us_p25": round(q[0], 2), "us_p75": round(q[2], 2)}
                base = entry["quadratic"]
                entry["baseline_spread"] = round((base["us_max"] - base["us_min"]) / base["us_median"], 4)
                entry["cfg_over_quadratic"] = round(entry["cfg"]["us_median"] / base["us_median"], 4)
                entry["cfg_over_torch"] = round(entry["cfg"]["us_median"] / entry["torch"]["us_median"], 4)
                entry["cfg_TB_per_s"] = round(entry["cfg_bytes"] / entry["cfg"]["us_median"] / 1e6, 3)
                print(f"B={B},K1={K1}: {json.dumps(entry)}", flush=True)
            finally:
                shutil.rmtree(directory, ignore_errors=True)
        fd, path = tempfile.mkstemp(prefix="cfg_wall_", suffix=".json")
        os.close(fd)
        try:
            run_step([sys.executable, os.path.abspath(__file__), "--wall-worker", "--wall-out", path], WALL_LIMIT_S)
            with open(path) as f:
                res["wall_64_tokens_B8"] = json.load(f)
        finally:
            os.unlink(path)
    except (OSError, subprocess.SubprocessError, RuntimeError, KeyError) as e:   # a step failed: nothing more is started on the GPU
        res["trace_error"] = f"{type(e).__name__}: {e}"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 1 if "trace_error" in res else 0


if __name__ == "__main__":
    sys.exit(main())
