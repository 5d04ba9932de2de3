#!/usr/bin/env python3
"""Time the DRY kernel (asd_dry_rows) at the verify loop's shape, B = 32, K1 = 9, V = 152064, bf16, at history lengths of 128,
2048 and 16384 tokens, next to the no-repeat-n-gram kernel (asd_no_repeat_ngram_rows, n = 3), which reads the same histories and
writes a tensor of the same shape and values, in the same process.  Each kernel has its OWN copy of the logits: the ban's -inf
would otherwise sit exactly where DRY penalises, and DRY leaves -inf alone:

  dry_L_natural / ngram_L_natural    every row's history holds random ids over 300 distinct tokens: a handful of candidates per
                                     position, short walks, a few penalised tokens
  dry_L_equal / ngram_L_equal        the all-equal history: every position is a candidate for ONE token and walks CAP steps

    python tools/bench_dry.py [--out profiles/dry.json] [--rounds 15] [--calls 20] [--no-trace]

Two figures per variant, as in tools/bench_no_repeat_ngram.py.  `kernel_us`: the kernels' own time, from a
`rocprofv3 --kernel-trace` run OF ITS OWN (no counters, no other tracing): this script starts itself once more under the profiler
as a fresh child process (`--worker`) before it touches the GPU, the child runs every variant `--calls` times, and the
dispatches are attributed by position: a one-row f32 launch of the n-gram kernel (another template instance, so another kernel
name) is the separator between variants.  `us_median`: the per-call time from Python with the profiler off -- one device-event
pair around `--calls` back-to-back calls, the variants in alternation, `--rounds` rounds after a warm-up round.  A repeated DRY
call subtracts again; the elements stay finite (the clamp), so every call does the same work.  `ratio_to_ngram` is the quotient
of kernel_us (of us_median where the trace is missing); `ngram_spread` is (max - min) / median of the baseline's own per-call
figures: what a ratio has to exceed to mean anything.  Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_token_mask import parse_trace  # noqa: E402  (the kernel-trace reader: dispatches cut at a separator kernel)

SEPARATOR = ("k_no_repeat_ngram_rows<0>", "k_no_repeat_ngram_rowsILi0E")   # the f32 instance, demangled or not: the timed launches are bf16
PROMPT = 24
DISTINCT = 300


def build_variants(a):
    """-> (variants: name -> callable, separator: callable, info).  Everything the timed calls touch is made here."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_dry.py needs a GPU (no fallback)")
    from asd_amd import kernels as K

    B, Kd, V = a.batch, a.draft_len, a.vocab
    g = torch.Generator(device="cuda").manual_seed(1)
    y = (torch.randn((B, Kd + 1, V), generator=g, device="cuda") * 4.0).to(torch.bfloat16)
    y_ban = y.clone()                                            # the n-gram kernel's own copy: its -inf would switch DRY's stores off
    rng = np.random.default_rng(1)
    ids = rng.choice(V, DISTINCT, replace=False).astype(np.int32)
    dry = K.pack_dry([a.multiplier] * B, [a.base] * B, [a.allowed_length] * B, [0] * B, (), [PROMPT] * B, PROMPT, "cuda")
    ngram = K.pack_no_repeat_ngram([3] * B, [PROMPT] * B, PROMPT, "cuda")
    variants = {}
    for L in a.lengths:
        cap = L + 64
        for kind in ("natural", "equal"):
            tokens_h = ids[rng.integers(0, DISTINCT, (B, cap))] if kind == "natural" else np.full((B, cap), int(ids[0]), dtype=np.int32)
            step_h = tokens_h[:, :Kd].copy()                         # the proposals continue with ids of the same kind
            tokens, step_tok = torch.from_numpy(tokens_h).cuda(), torch.from_numpy(step_h).cuda()
            seq_len = torch.full((B,), L, dtype=torch.int32, device="cuda")
            variants[f"dry_{L}_{kind}"] = lambda t=tokens, s=seq_len, c=cap, p=step_tok: K.dry_rows(y, dry, t, s, c, p, 0)
            variants[f"ngram_{L}_{kind}"] = lambda t=tokens, s=seq_len, c=cap, p=step_tok: K.no_repeat_ngram_rows(y_ban, ngram, t, s, c, p, 0)
    tiny = torch.zeros((1, 1, 32), dtype=torch.float32, device="cuda")
    tiny_n = K.pack_no_repeat_ngram([1], [0], 0, "cuda")
    tiny_tokens, tiny_len = torch.zeros((1, 4), dtype=torch.int32, device="cuda"), torch.ones((1,), dtype=torch.int32, device="cuda")
    info = {"B": B, "K1": Kd + 1, "V": V, "dtype": "bf16", "device": torch.cuda.get_device_name(0), "cus": K.device_cu_count(0),
            "prompt": PROMPT, "distinct_ids_natural": DISTINCT, "dry_multiplier": a.multiplier, "dry_base": a.base,
            "dry_allowed_length": a.allowed_length, "ngram_n": 3}
    return variants, (lambda: K.no_repeat_ngram_rows(tiny, tiny_n, tiny_tokens, tiny_len, 4)), info


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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dry.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--draft-len", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--multiplier", type=float, default=0.8)
    ap.add_argument("--base", type=float, default=1.75)
    ap.add_argument("--allowed-length", type=int, default=2)
    ap.add_argument("--lengths", type=int, nargs="*", default=[128, 2048, 16384], help="history lengths (prompt plus generated)")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run (kernel_us is then missing)")
    ap.add_argument("--trace-dir", default=None, help="keep the profiler's output here (default: a temporary directory)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)

    # 1. the kernel trace, in a fresh child process and before this one opens the GPU
    trace, trace_error = None, None
    if not a.no_trace:
        directory = os.path.abspath(a.trace_dir) if a.trace_dir is not None else tempfile.mkdtemp(prefix="dry_trace_")
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", directory, "--", sys.executable, os.path.abspath(__file__),
               "--worker", "--batch", str(a.batch), "--draft-len", str(a.draft_len), "--vocab", str(a.vocab), "--calls", str(a.calls),
               "--multiplier", str(a.multiplier), "--base", str(a.base), "--allowed-length", str(a.allowed_length),
               "--lengths", *map(str, a.lengths)]
        try:
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        except (OSError, subprocess.SubprocessError) as e:
            trace_error = f"{type(e).__name__}: {e}"
    # 2. the per-call figures from Python, profiler off
    import torch
    variants, _, info = build_variants(a)
    if not a.no_trace and trace_error is None:
        try:
            trace = parse_trace(directory, list(variants), a.calls, SEPARATOR)
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
    res = {"what": "asd_dry_rows next to asd_no_repeat_ngram_rows (n = 3) on two copies of one [B, K1, V] tensor and the same histories, "
                   "one call each: random ids over a few hundred distinct tokens, and the all-equal worst case",
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
    for L in a.lengths:
        for kind in ("natural", "equal"):
            own, base = res[f"dry_{L}_{kind}"], res[f"ngram_{L}_{kind}"]
            own["ratio_to_ngram"] = round(own[key] / base[key], 3)
            own["ngram_spread"] = round((base[key + "_max" if trace is not None else "us_max"] -
                                         base[key + "_min" if trace is not None else "us_min"]) / base[key], 3)
    res["ratios_from"] = key
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
