#!/usr/bin/env python3
"""Time the dense token mask (asd_logit_mask_rows) at the verify loop's shape, B = 32, K = 8, V = 152064, bf16, with allow-lists
of 4 and of V / 2 ids, next to what a caller has without it, in the same process and on the same tensors:

  logit_mask_N          one call on the target's [B, K+1, V] output, every row on its own list of N ids (R = B masks)
  logit_mask_N_draft    one call on one proposal's [B, V] draft logits (a verifying step makes K of these)
  masked_fill_N[_draft] torch.Tensor.masked_fill_(mask, -inf) with a bool [B, 1, V] ([B, V]) mask of the same lists: it reads
                        the mask and every element and writes every element
  fill[_draft]          torch.Tensor.fill_(-inf) of the same bytes: the write-only floor

    python tools/bench_token_mask.py [--out profiles/token_mask_step.json] [--rounds 15] [--calls 40] [--no-trace]

Two figures per variant.  `kernel_us`: the kernel's own time, from a `rocprofv3 --kernel-trace` run OF ITS OWN (no counters, no
other tracing): this script starts itself once more under the profiler as a fresh child process (`--worker`) before it touches
the GPU, the child runs every variant `--calls` times, and the dispatches are attributed by position: a one-word f32 launch of
the mask kernel (another template instance, so another kernel name) is the separator between variants.  `us_median`: the
per-call time from Python with the profiler off -- one device-event pair around `--calls` back-to-back calls, the variants in
alternation, `--rounds` rounds after a warm-up round; min .. max is the spread.  `ratio_to_masked_fill` and `ratio_to_fill` are
quotients of kernel_us (of us_median where the trace is missing).  Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEPARATOR = ("k_logit_mask_rows<0>", "k_logit_mask_rowsILi0E")     # the f32 instance, demangled or not: the timed launches are bf16 (<1>)


def build_variants(a):
    """-> (variants: name -> callable, separator: callable, info).  Everything the timed calls touch is made here."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_token_mask.py needs a GPU (no fallback)")
    from asd_amd import kernels as K

    B, Kd, V = a.batch, a.draft_len, a.vocab
    g = torch.Generator(device="cuda").manual_seed(1)
    x = (torch.randn((B, Kd + 1, V), generator=g, device="cuda") * 4.0).to(torch.bfloat16)
    y, yd = x.clone(), x[:, 0].clone()                       # what every variant writes to
    rng = np.random.default_rng(1)
    ninf = float("-inf")
    variants = {}
    for n in a.allowed:
        lists = [tuple(sorted(int(t) for t in rng.choice(V, n, replace=False))) for _ in range(B)]
        packed = K.pack_token_masks(lists, V, "cuda")
        assert packed.R == B
        ban = torch.ones((B, 1, V), dtype=torch.bool, device="cuda")
        for b, ids in enumerate(lists):
            ban[b, 0, list(ids)] = False
        ban2 = ban[:, 0].contiguous()
        # the same answer before any timing: the kernel and masked_fill_ agree bit for bit
        K.logit_mask_rows(y, packed)
        want = x.clone().masked_fill_(ban, ninf)
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int16), want.view(torch.int16)) and int((~torch.isneginf(y)).sum()) == B * (Kd + 1) * n
        del want
        y.copy_(x)
        variants[f"logit_mask_{n}"] = lambda p=packed: K.logit_mask_rows(y, p)
        variants[f"logit_mask_{n}_draft"] = lambda p=packed: K.logit_mask_rows(yd, p)
        variants[f"masked_fill_{n}"] = lambda m=ban: y.masked_fill_(m, ninf)
        variants[f"masked_fill_{n}_draft"] = lambda m=ban2: yd.masked_fill_(m, ninf)
    variants["fill"] = lambda: y.fill_(ninf)
    variants["fill_draft"] = lambda: yd.fill_(ninf)
    tiny = torch.zeros((1, 1, 32), dtype=torch.float32, device="cuda")
    tiny_mask = K.pack_token_masks([(0,)], 32, "cuda")
    info = {"B": B, "K": Kd, "V": V, "dtype": "bf16", "device": torch.cuda.get_device_name(0), "cus": K.device_cu_count(0),
            "bytes": {"target": B * (Kd + 1) * V * 2, "draft": B * V * 2}}
    return variants, (lambda: K.logit_mask_rows(tiny, tiny_mask)), info


def worker(a) -> int:
    """Under the profiler: a warm-up call of everything, then per variant one separator launch and `--calls` calls."""
    import torch
    variants, separator, _ = build_variants(a)
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    for fn in variants.values():
        separator()
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
    separator()
    torch.cuda.synchronize()
    return 0


def _column(fields, *names):
    low = {f.lower(): f for f in fields}
    for n in names:
        if n in low:
            return low[n]
    raise KeyError(f"none of {names} among the trace's columns {fields}")


def parse_trace(directory, names, calls, separator=SEPARATOR, trailing=0):
    """The kernel-trace CSV(s) under `directory` -> {variant: [per-call kernel time in us]}: dispatches in start order, cut at
    the separator kernel; the last len(names) + 1 separators delimit the variants in order (the warm-up has none).  `trailing`:
    dispatches at the end of every segment that prepare the NEXT variant and are left out."""
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
    cuts = [i for i, r in enumerate(rows) if any(s in r[2] for s in separator)]
    if len(cuts) < len(names) + 1:
        raise RuntimeError(f"{len(cuts)} separator launches in the trace, expected {len(names) + 1}")
    cuts = cuts[-(len(names) + 1):]
    out = {}
    for name, lo, hi in zip(names, cuts, cuts[1:]):
        seg = rows[lo + 1:hi - trailing]
        if not seg or len(seg) % calls:
            raise RuntimeError(f"{name}: {len(seg)} dispatches for {calls} calls")
        m = len(seg) // calls                               # kernels per call (1 for every variant here, but counted, not assumed)
        out[name] = {"us": [sum(e - s for s, e, _ in seg[i * m:(i + 1) * m]) / 1e3 for i in range(calls)], "kernels_per_call": m,
                     "kernel": seg[0][2][:120]}
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_mask_step.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--draft-len", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--allowed", type=int, nargs="*", default=None, help="list sizes (default: 4 and V / 2)")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run (kernel_us is then missing)")
    ap.add_argument("--trace-dir", default=None, help="keep the profiler's output here (default: a temporary directory)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.allowed is None:
        a.allowed = [4, a.vocab // 2]
    if a.worker:
        return worker(a)

    # 1. the kernel trace, in a fresh child process and before this one opens the GPU
    trace, trace_error = None, None
    if not a.no_trace:
        keep = a.trace_dir is not None
        directory = os.path.abspath(a.trace_dir) if keep else tempfile.mkdtemp(prefix="token_mask_trace_")
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", directory, "--", sys.executable, os.path.abspath(__file__),
               "--worker", "--batch", str(a.batch), "--draft-len", str(a.draft_len), "--vocab", str(a.vocab), "--calls", str(a.calls),
               "--allowed", *map(str, a.allowed)]
        try:
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        except (OSError, subprocess.SubprocessError) as e:
            trace_error = f"{type(e).__name__}: {e}"
    # 2. the per-call figures from Python, profiler off
    import torch
    variants, _, info = build_variants(a)
    if not a.no_trace and trace_error is None:
        try:
            trace = parse_trace(directory, list(variants), a.calls)
        except (RuntimeError, KeyError, ValueError) as e:
            trace_error = f"{type(e).__name__}: {e}"
    times = {k: [] for k in variants}
    for rnd in range(a.rounds + 1):                         # round 0: warm-up
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            if rnd:
                times[name].append(1e3 * e0.elapsed_time(e1) / a.calls)
    res = {"what": "asd_logit_mask_rows next to masked_fill_ (bool mask) and fill_ on the same tensors, one call each",
           **info, "rounds": a.rounds, "calls_per_round": a.calls}
    if trace_error is not None:
        res["trace_error"] = trace_error
    for name, t in times.items():
        res[name] = {"us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2)}
        if trace is not None:
            k = trace[name]
            res[name].update(kernel_us=round(statistics.median(k["us"]), 2), kernel_us_min=round(min(k["us"]), 2),
                             kernel_us_max=round(max(k["us"]), 2), kernels_per_call=k["kernels_per_call"], kernel=k["kernel"])
    key = "kernel_us" if trace is not None else "us_median"
    for n in a.allowed:
        for tail in ("", "_draft"):
            own = res[f"logit_mask_{n}{tail}"]
            own["ratio_to_masked_fill"] = round(own[key] / res[f"masked_fill_{n}{tail}"][key], 3)
            own["ratio_to_fill"] = round(own[key] / res[f"fill{tail}"][key], 3)
            own["write_gb_per_s"] = round(info["bytes"]["draft" if tail else "target"] * (1 - n / a.vocab) / own[key] / 1e3, 1)
    res["ratios_from"] = key
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
