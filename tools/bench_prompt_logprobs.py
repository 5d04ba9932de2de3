#!/usr/bin/env python3
"""Time the prompt-scoring pass (asd_prompt_logprobs) against the pass it shares its body with (asd_top_logprobs, the baseline),
on one bf16 tensor [32, 64, 152064] (623 MB: larger than the last-level cache, so every call streams it from HBM):

  top_logprobs_n5       asd_top_logprobs, N = 5                 -- the 5 most likely tokens of every row
  prompt_logprobs_n5    asd_prompt_logprobs, N = 5              -- the same table, plus the log-prob and rank of one token per row
  prompt_logprobs_n0    asd_prompt_logprobs, N = 0              -- log-prob and rank alone: no list is kept

    python tools/bench_prompt_logprobs.py [--out profiles/prompt_logprobs.json] [--repeats 30] [--no-trace] [--no-stage]

Kernel time comes from a `rocprofv3 --kernel-trace --stats` run OF ITS OWN (no counters, no other tracing): this script starts
itself once more under the profiler as a fresh child process (`--worker`) before it touches the GPU; the child launches the
three in alternation, `--repeats` times after 3 warm-up rounds, and the dispatches are attributed by kernel name.  Reported per
variant: the median, minimum and maximum over the repeats, the bytes the pass must read (the logits) over the median against
the HBM peak, the spread of the baseline ((max - min) / median, which one slow dispatch decides, and (p75 - p25) / median), and the ratios of the two new medians to the baseline's.
This is a measurement, not a pass mark.

Stage level (profiler off, host clock around a call that ends in a device-to-host copy): one Stage.generate call at B = 32,
P = 512, V = 152064, 4 tokens, with prompt_logprobs = 5, = 0 and off, alternating; the extra time is the difference of medians.
Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TBPS = 8.0            # HBM3E peak of the MI355X (specification); about 6.3 TB/s is achievable by a streaming copy
HBM_COPY_TBPS = 6.3
WARMUP = 3
VARIANTS = ("top_logprobs_n5", "prompt_logprobs_n5", "prompt_logprobs_n0")


def worker(a) -> int:
    import torch
    from asd_amd import kernels as K
    B, T, V = a.batch, a.rows, a.vocab
    g = torch.Generator(device="cuda").manual_seed(1)
    x = (torch.randn((B, T, V), generator=g, device="cuda") * 4.0).to(torch.bfloat16)
    target = torch.randint(0, V, (B, T), generator=g, device="cuda", dtype=torch.int32)
    top = K.TopLogprobs(B, T, V, torch.bfloat16, 5)
    p5 = K.PromptLogprobs(B, T, V, torch.bfloat16, 5)
    p0 = K.PromptLogprobs(B, T, V, torch.bfloat16, 0)
    # same answers before any timing: the table bit for bit, the log-prob against log_softmax, the rank against a count
    ids, lps = top(x, out=top.out)
    lp, rank, pid, plp = p5(x, target)
    lp0, rank0, _, _ = p0(x, target)
    xf = x[:2].float()
    ref = torch.log_softmax(xf, -1).gather(-1, target[:2].long()[..., None])[..., 0]
    xg = xf.gather(-1, target[:2].long()[..., None])
    idx = torch.arange(V, device="cuda")
    cnt = 1 + ((xf > xg) | ((xf == xg) & (idx < target[:2].long()[..., None]))).sum(-1)
    torch.cuda.synchronize()
    assert torch.equal(ids, pid) and torch.equal(lps.view(torch.int32), plp.view(torch.int32))
    assert torch.equal(rank, rank0) and torch.equal(lp.view(torch.int32), lp0.view(torch.int32))
    assert float((lp[:2] - ref).abs().max()) < 1e-4 and torch.equal(rank[:2].long(), cnt)
    for _ in range(WARMUP + a.repeats):
        top(x, out=top.out)
        p5(x, target)
        p0(x, target)
    torch.cuda.synchronize()
    return 0


def _column(fields, *names):
    low = {f.lower(): f for f in fields}
    for n in names:
        if n in low:
            return low[n]
    raise KeyError(f"none of {names} among the trace's columns {fields}")


def _variant(kernel_name: str):
    """The variant a dispatch belongs to, from its (demangled or mangled) kernel name; None for anything else."""
    name = kernel_name.replace(" ", "")
    if "k_top_logprobs" in name:
        return VARIANTS[0]
    m = re.search(r"k_prompt_logprobs(?:<\d+,(\d+)>|ILi\d+ELi(\d+)E)", name)
    if m:
        return VARIANTS[1] if (m.group(1) or m.group(2)) == "1" else VARIANTS[2]
    return None


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
    out = {v: [] for v in VARIANTS}
    for s, e, name in rows:
        v = _variant(name)
        if v is not None:
            out[v].append((e - s) / 1e3)
    for v, t in out.items():
        if len(t) < repeats:
            raise RuntimeError(f"{v}: {len(t)} dispatches in the trace, expected at least {repeats}")
        out[v] = t[-repeats:]
    return out


def stage_level(a):
    """One generate call at B = batch, P = prompt tokens with the feature at 5, at 0 and off: host clock, alternating."""
    import torch
    from asd_amd.serving.stages import StageConfig, StageManager
    from asd_amd.serving.synthetic_lm import tiny
    cfg = StageConfig(model_name="tiny-0", model_size="s0", cost_per_token=1.0, shape=tiny(vocab=a.vocab), model_seed=0,
                      logit_scale=3.0, max_prompt_tokens=a.prompt_tokens)
    stage = StageManager([cfg]).get_stage("s0")
    prompts = [" ".join(f"w{(7 * b + 13 * i) % 997}" for i in range(a.prompt_tokens)) for b in range(a.stage_batch)]
    kw = dict(prompts=prompts, max_tokens=4, temperature=0.0)
    settings = {"off": {}, "n5": {"prompt_logprobs": 5}, "n0": {"prompt_logprobs": 0}}
    times = {k: [] for k in settings}
    for rnd in range(a.stage_rounds + 1):                   # round 0: warm-up
        for name, extra in settings.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stage.generate(**kw, **extra)
            torch.cuda.synchronize()
            if rnd:
                times[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(t) for k, t in times.items()}
    return {"what": "one Stage.generate call (stage 0, tiny model, greedy, 4 tokens), host clock, profiler off",
            "B": a.stage_batch, "P": a.prompt_tokens, "V": a.vocab, "rounds": a.stage_rounds,
            "prefill_logit_bytes": a.stage_batch * (a.prompt_tokens - 1) * a.vocab * 2,
            **{f"{k}_ms": {"median": round(med[k], 3), "min": round(min(times[k]), 3), "max": round(max(times[k]), 3)} for k in times},
            "extra_ms_n5": round(med["n5"] - med["off"], 3), "extra_ms_n0": round(med["n0"] - med["off"], 3)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prompt_logprobs.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rows", type=int, default=64, help="T: rows per sequence of the kernel-level tensor")
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--stage-batch", type=int, default=32)
    ap.add_argument("--prompt-tokens", type=int, default=512)
    ap.add_argument("--stage-rounds", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run")
    ap.add_argument("--no-stage", action="store_true", help="skip the stage-level timing")
    ap.add_argument("--trace-dir", default=None, help="keep the profiler's output here (default: a temporary directory)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)

    nbytes = a.batch * a.rows * a.vocab * 2
    res = {"what": "asd_prompt_logprobs (N = 5, N = 0) vs asd_top_logprobs (N = 5) on one [B, T, V] bf16 tensor: kernel time from a "
                   "rocprofv3 --kernel-trace --stats run of its own, the three launched in alternation",
           "B": a.batch, "T": a.rows, "V": a.vocab, "dtype": "bf16", "rows": a.batch * a.rows, "logit_bytes": nbytes,
           "repeats": a.repeats, "warmup_rounds": WARMUP, "hbm_peak_tbps": HBM_PEAK_TBPS, "hbm_copy_tbps": HBM_COPY_TBPS}
    # 1. kernel times: a fresh child under the profiler, before this process touches the GPU
    if not a.no_trace:
        keep = a.trace_dir is not None
        directory = os.path.abspath(a.trace_dir) if keep else tempfile.mkdtemp(prefix="prompt_logprobs_trace_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", directory, "--", sys.executable,
               os.path.abspath(__file__), "--worker", "--batch", str(a.batch), "--rows", str(a.rows), "--vocab", str(a.vocab),
               "--repeats", str(a.repeats)]
        try:
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
            times = parse_trace(directory, a.repeats)
            for v, t in times.items():
                med = statistics.median(t)
                tbps = nbytes / (med * 1e-6) / 1e12
                q = statistics.quantiles(t, n=4)
                res[v] = {"us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                          "us_p25": round(q[0], 2), "us_p75": round(q[2], 2),
                          "logit_tbps": round(tbps, 3), "share_of_hbm_peak": round(tbps / HBM_PEAK_TBPS, 3),
                          "share_of_hbm_copy_rate": round(tbps / HBM_COPY_TBPS, 3)}
            base = res[VARIANTS[0]]
            res["baseline_spread"] = round((base["us_max"] - base["us_min"]) / base["us_median"], 4)
            res["baseline_quartile_spread"] = round((base["us_p75"] - base["us_p25"]) / base["us_median"], 4)
            res["n5_over_baseline"] = round(res[VARIANTS[1]]["us_median"] / base["us_median"], 4)
            res["n0_over_baseline"] = round(res[VARIANTS[2]]["us_median"] / base["us_median"], 4)
            res["n0_over_n5"] = round(res[VARIANTS[2]]["us_median"] / res[VARIANTS[1]]["us_median"], 4)
            res["ratios_inside_baseline_spread"] = bool(max(res["n5_over_baseline"], res["n0_over_baseline"]) - 1.0
                                                        <= res["baseline_spread"])
            res["ratios_inside_baseline_quartile_spread"] = bool(max(res["n5_over_baseline"], res["n0_over_baseline"]) - 1.0
                                                                 <= res["baseline_quartile_spread"])
        except (OSError, subprocess.SubprocessError, RuntimeError, KeyError) as e:
            res["trace_error"] = f"{type(e).__name__}: {e}"
        finally:
            if not keep:
                shutil.rmtree(directory, ignore_errors=True)
    # 2. the stage-level figure, profiler off
    if not a.no_stage:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_prompt_logprobs.py needs a GPU (no fallback)")
        from asd_amd import kernels as K
        res["device"], res["cus"] = torch.cuda.get_device_name(0), K.device_cu_count(0)
        res["stage"] = stage_level(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 1 if "trace_error" in res else 0


if __name__ == "__main__":
    sys.exit(main())
