#!/usr/bin/env python3
"""Time the multi-token bad-words kernel (asd_bad_words_rows) at the verify loop's shape, B = 32, K = 8, V = 152064, bf16, with
16 and 256 words per row, next to the sparse logit edit (asd_logit_edit_rows, unchanged since it was added) with the same number
of entries, in the same process and on the same tensors:

  bad_words_N          one call on the target's [B, K+1, V] output, n_prev = 0: every row with its own N words -- a quarter of
                       them one token long (always stored), a quarter bigrams that the row's last committed token completes at
                       position 0, a quarter trigrams that straddle the committed tokens and the step's proposals, a quarter
                       8-token words that match nowhere (seven history loads, no store)
  bad_words_N_draft    one call on one proposal's [B, V] draft logits, n_prev = K / 2 (a verifying step makes K of these)
  edit_N[_draft]       asd_logit_edit_rows with N permanent bans per row on the same tensors: the yardstick -- one workgroup per
                       (b, j) as well, N stores per logits row and no history loads

    python tools/bench_bad_words.py [--out profiles/bad_words_step.json] [--rounds 15] [--calls 20] [--no-trace] [--no-stage]

Two figures per variant.  `kernel_us`: the kernels' own time, from a `rocprofv3 --kernel-trace` run OF ITS OWN (no counters, no
other tracing): this script starts itself once more under the profiler as a fresh child process (`--worker`) before it touches
the GPU, the child runs every variant `--calls` times, and the dispatches are attributed by position: a one-word f32 launch of
the bad-words kernel (another template instance, so another kernel name) is the separator between variants.  `us_median`: the
per-call time from Python with the profiler off -- one device-event pair around `--calls` back-to-back calls, the variants in
alternation, `--rounds` rounds after a warm-up round.  Both operations only store -inf, so a repeated call stores the same
bits again and nothing has to be restored.  `ratio_to_edit` is the quotient of kernel_us (of us_median where the trace is
missing).

`stage_step`: for information, the wall time per verifying step of Stage.generate on two tiny stages at the full vocabulary,
B = 32, with and without 16 bad words for the batch.  The run without them makes exactly the ops calls the stage made before bad
words existed.  Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_token_mask import parse_trace  # noqa: E402  (the kernel-trace reader: dispatches cut at a separator kernel)

SEPARATOR = ("k_bad_words_rows<0>", "k_bad_words_rowsILi0E")   # the f32 instance, demangled or not: the timed launches are bf16 (<1>)
EDIT_FOREVER = 2 ** 31 - 1


def build_variants(a):
    """-> (variants: name -> callable, separator: callable, info).  Everything the timed calls touch is made here."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bad_words.py needs a GPU (no fallback)")
    from asd_amd import kernels as K

    B, Kd, V = a.batch, a.draft_len, a.vocab
    g = torch.Generator(device="cuda").manual_seed(1)
    y = (torch.randn((B, Kd + 1, V), generator=g, device="cuda") * 4.0).to(torch.bfloat16)
    yd = y[:, 0].clone()
    rng = np.random.default_rng(1)
    start, cap = 24, 64
    tokens_h = rng.integers(0, V, (B, cap)).astype(np.int32)
    seq_h = np.full((B,), 40, dtype=np.int32)
    step_h = rng.integers(0, V, (B, Kd)).astype(np.int32)
    tokens, seq_len, step_tok = (torch.from_numpy(t).cuda() for t in (tokens_h, seq_h, step_h))
    variants = {}
    for n in a.words:
        rows, bans = [], []
        for b in range(B):
            last = [int(t) for t in rng.choice(V, n, replace=False)]
            end, prop = int(tokens_h[b, seq_h[b] - 1]), int(step_h[b, 0])
            words = []
            for i, t in enumerate(last):
                words.append(((t,), (end, t), (end, prop, t), tuple(int(v) for v in rng.integers(0, V, 7)) + (t,))[i % 4])
            rows.append(words)
            bans.append([(t, 0.0, EDIT_FOREVER) for t in sorted(last)])
        words, edits = K.pack_bad_words(rows, "cuda"), K.pack_logit_edits(bans, "cuda")
        variants[f"bad_words_{n}"] = lambda w=words: K.bad_words_rows(y, w, tokens, seq_len, start, cap, step_tok, 0)
        variants[f"bad_words_{n}_draft"] = lambda w=words: K.bad_words_rows(yd, w, tokens, seq_len, start, cap, step_tok, Kd // 2)
        variants[f"edit_{n}"] = lambda e=edits: K.logit_edit_rows(y, e, seq_len, start, 0)
        variants[f"edit_{n}_draft"] = lambda e=edits: K.logit_edit_rows(yd, e, seq_len, start, Kd // 2)
    tiny = torch.zeros((1, 1, 32), dtype=torch.float32, device="cuda")
    tiny_words = K.pack_bad_words([[(0,)]], "cuda")
    tiny_tokens, tiny_len = torch.zeros((1, 4), dtype=torch.int32, device="cuda"), torch.zeros((1,), dtype=torch.int32, device="cuda")
    info = {"B": B, "K": Kd, "V": V, "dtype": "bf16", "device": torch.cuda.get_device_name(0), "cus": K.device_cu_count(0),
            "history": {"start": start, "seq_len": int(seq_h[0]), "max_len": cap}}
    return variants, (lambda: K.bad_words_rows(tiny, tiny_words, tiny_tokens, tiny_len, 0, 4)), info


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


def stage_step(a):
    """Wall time per verifying step of Stage.generate, two tiny stages at the full vocabulary, with and without bad words."""
    import torch
    from asd_amd.serving.stages import StageConfig, StageManager
    from asd_amd.serving.synthetic_lm import tiny
    cfgs = [StageConfig(model_name=f"tiny-{i}", model_size=name, shape=tiny(vocab=a.vocab), model_seed=i, logit_scale=3.0,
                        draft_len=a.draft_len, seed=11 + i) for i, name in enumerate(("8b", "13b"))]
    stage = StageManager(cfgs).get_stage("13b")
    prompts = [f"request number {i} of the batch" for i in range(a.batch)]
    kw = dict(prompts=prompts, max_tokens=32, temperature=0.7, seed=list(range(a.batch)))
    words = dict(bad_words=[(i,) if i % 2 else (i, i + 1, i + 2) for i in range(100, 116)])
    runs = (("without", {}), ("with", words))
    per_step = {name: [] for name, _ in runs}
    for rnd in range(5):                                     # round 0: warm-up; the two in alternation
        for name, extra in runs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stage.generate(**kw, **extra)
            torch.cuda.synchronize()
            if rnd:
                per_step[name].append((1e3 * (time.perf_counter() - t0) / stage.last_steps, stage.last_steps))
    out = {name: {"ms_per_step_median": round(statistics.median(t for t, _ in v), 3), "ms_per_step_min": round(min(t for t, _ in v), 3),
                  "ms_per_step_max": round(max(t for t, _ in v), 3), "steps": v[-1][1]} for name, v in per_step.items()}
    out["what"] = ("Stage.generate, stage 1 of two tiny(vocab) stages, B prompts, 32 tokens, temperature 0.7, seeded: wall time of the "
                   "whole call divided by its steps; `with`: 16 bad words for the batch; `without` makes exactly the ops calls made "
                   "before bad words existed")
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bad_words_step.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--draft-len", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--words", type=int, nargs="*", default=[16, 256], help="words (and edit entries) per row")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run (kernel_us is then missing)")
    ap.add_argument("--no-stage", action="store_true", help="skip the stage-step timing")
    ap.add_argument("--trace-dir", default=None, help="keep the profiler's output here (default: a temporary directory)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)

    # 1. the kernel trace, in a fresh child process and before this one opens the GPU
    trace, trace_error = None, None
    if not a.no_trace:
        keep = a.trace_dir is not None
        directory = os.path.abspath(a.trace_dir) if keep else tempfile.mkdtemp(prefix="bad_words_trace_")
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", directory, "--", sys.executable, os.path.abspath(__file__),
               "--worker", "--batch", str(a.batch), "--draft-len", str(a.draft_len), "--vocab", str(a.vocab), "--calls", str(a.calls),
               "--words", *map(str, a.words)]
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
    res = {"what": "asd_bad_words_rows next to asd_logit_edit_rows with as many entries per row as the other has words, on the same "
                   "tensors, one call each", **info, "rounds": a.rounds, "calls_per_round": a.calls}
    if trace_error is not None:
        res["trace_error"] = trace_error
    for name, t in times.items():
        res[name] = {"us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2)}
        if trace is not None:
            k = trace[name]
            res[name].update(kernel_us=round(statistics.median(k["us"]), 2), kernel_us_min=round(min(k["us"]), 2),
                             kernel_us_max=round(max(k["us"]), 2), kernels_per_call=k["kernels_per_call"], kernel=k["kernel"])
    key = "kernel_us" if trace is not None else "us_median"
    for n in a.words:
        for tail in ("", "_draft"):
            own = res[f"bad_words_{n}{tail}"]
            own["ratio_to_edit"] = round(own[key] / res[f"edit_{n}{tail}"][key], 4)
    res["ratios_from"] = key
    if not a.no_stage:
        del variants
        torch.cuda.empty_cache()
        res["stage_step"] = stage_step(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
