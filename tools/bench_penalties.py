#!/usr/bin/env python3
"""Time the stateful penalties (asd_penalty_rows, asd_penalty_commit) at the verify loop's shape, B = 32, K = 8, V = 152064, bf16,
with 16, 256 and 2048 distinct seen tokens per row, next to what a caller has without the kernels, in the same process and on
the same tensors:

  penalty_rows_N          one call on the target's [B, K+1, V] output: every row with its own state of N seen tokens (half of
                          them prompt-only, half with counts 1..4) and K proposals, n_prev = 0
  penalty_rows_N_draft    one call on one proposal's [B, V] draft logits, n_prev = K / 2 (a verifying step makes K of these)
  torch_N[_draft]         vLLM's `apply_penalties` written in torch on the same tensors: a dense bincount of the output tokens
                          (scatter_add_ into [B, V + 1]), the repetition penalty through `where`, then the frequency and the
                          presence term, in place.  It reads and writes every element; on [B, K+1, V] it uses ONE history for
                          all K + 1 positions (it has no per-position proposals: less work than the kernel does)
  penalty_commit          one call: K + 1 = 9 committed tokens per row enter the state

    python tools/bench_penalties.py [--out profiles/penalties_step.json] [--rounds 15] [--calls 20] [--no-trace] [--no-stage]

Two figures per variant.  `kernel_us`: the kernels' own time, from a `rocprofv3 --kernel-trace` run OF ITS OWN (no counters, no
other tracing): this script starts itself once more under the profiler as a fresh child process (`--worker`) before it touches
the GPU, the child runs every variant `--calls` times, and the dispatches are attributed by position: a one-word f32 launch of
the penalty kernel (another template instance, so another kernel name) is the separator between variants; the torch variants
are several kernels per call, summed.  `us_median`: the per-call time from Python with the profiler off -- one device-event pair
around `--calls` back-to-back calls, the variants in alternation, `--rounds` rounds after a warm-up round.  The logits are
restored in front of every timed batch (outside the timed region): the operation is not idempotent.  `ratio_to_torch` is the
quotient of kernel_us (of us_median where the trace is missing).

`stage_step`: for information, the wall time per verifying step of Stage.generate on two tiny stages at the full vocabulary,
B = 32, with and without penalties.  The run without them makes exactly the ops calls the stage made before the penalties
existed.  Needs a GPU: there is no fallback."""
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

SEPARATOR = ("k_penalty_rows<0>", "k_penalty_rowsILi0E")   # the f32 instance, demangled or not: the timed launches are bf16 (<1>)
RESTORE_KERNELS = 2                      # restore() is two copy kernels; under the profiler they end the segment in front of them


def torch_penalties(logits, out_tokens, prompt_mask, rep, pres, freq):
    """vLLM's apply_penalties in torch, in place: out_tokens int64 [B, T] padded with V; prompt_mask bool [B, V]; rep / pres /
    freq f32 [B]."""
    import torch
    Bv, V = prompt_mask.shape
    counts = torch.zeros((Bv, V + 1), dtype=torch.int64, device=logits.device)
    counts.scatter_add_(1, out_tokens, torch.ones_like(out_tokens))
    counts = counts[:, :V]
    out_mask = counts > 0
    r = torch.where(prompt_mask | out_mask, rep[:, None], torch.ones((), device=logits.device))
    f = freq[:, None] * counts
    p = pres[:, None] * out_mask
    if logits.dim() == 3:
        r, f, p = r[:, None], f[:, None], p[:, None]
    logits.copy_(torch.where(logits > 0, logits / r, logits * r))
    logits.sub_(f).sub_(p)
    return logits


def build_variants(a):
    """-> (variants: name -> callable, restore: callable, separator: callable, info).  Everything the timed calls touch is made
    here."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_penalties.py needs a GPU (no fallback)")
    from asd_amd import kernels as K

    B, Kd, V = a.batch, a.draft_len, a.vocab
    g = torch.Generator(device="cuda").manual_seed(1)
    x = (torch.randn((B, Kd + 1, V), generator=g, device="cuda") * 4.0).to(torch.bfloat16)
    y, yd = x.clone(), x[:, 0].clone()                       # what every variant writes to
    rng = np.random.default_rng(1)
    rep, pres, freq = [1.2] * B, [0.5] * B, [0.25] * B
    dev = lambda v: torch.tensor(v, dtype=torch.float32, device="cuda")         # noqa: E731
    step_tok = torch.from_numpy(rng.integers(0, V, (B, Kd)).astype(np.int32)).cuda()
    variants = {}
    for n in a.seen:
        prompts, outs = [], []
        for _ in range(B):
            ids = [int(t) for t in rng.choice(V, n, replace=False)]
            prompts.append(ids[: n // 2])
            outs.append([t for t in ids[n // 2:] for _ in range(int(rng.integers(1, 5)))])
        pen = K.pack_penalties(rep, pres, freq, [p + o for p, o in zip(prompts, outs)], V, "cuda")
        for b, o in enumerate(outs):                         # the counts of the output tokens, as penalty_commit would leave them
            pen.counts[b] = torch.bincount(torch.tensor(o, dtype=torch.int64), minlength=V).to(torch.int32).cuda()
        T = max(len(o) for o in outs)
        out_tokens = torch.tensor([o + [V] * (T - len(o)) for o in outs], dtype=torch.int64, device="cuda")
        prompt_mask = torch.zeros((B, V), dtype=torch.bool, device="cuda")
        for b, p in enumerate(prompts):
            prompt_mask[b, p] = True
        # the same elements before any timing: without proposals the kernel changes what the torch formulation changes
        K.penalty_rows(yd, pen)
        want = torch_penalties(x[:, 0].clone(), out_tokens, prompt_mask, dev(rep), dev(pres), dev(freq))
        torch.cuda.synchronize()
        changed = (yd.view(torch.int16) != x[:, 0].view(torch.int16))
        assert 0 < int(changed.sum()) <= B * n
        assert float((yd.float() - want.float()).abs().max()) <= 0.5           # (torch rounds to bf16 after every operator)
        del want
        yd.copy_(x[:, 0])
        variants[f"penalty_rows_{n}"] = lambda p=pen: K.penalty_rows(y, p, step_tok, 0)
        variants[f"penalty_rows_{n}_draft"] = lambda p=pen: K.penalty_rows(yd, p, step_tok, Kd // 2)
        args = (out_tokens, prompt_mask, dev(rep), dev(pres), dev(freq))
        variants[f"torch_{n}"] = lambda q=args: torch_penalties(y, *q)
        variants[f"torch_{n}_draft"] = lambda q=args: torch_penalties(yd, *q)
    cap = 64
    tokens = torch.from_numpy(rng.integers(0, V, (B, cap)).astype(np.int32)).cuda()
    seq_len = torch.full((B,), 40, dtype=torch.int32, device="cuda")
    n_commit = torch.full((B,), Kd + 1, dtype=torch.int32, device="cuda")
    cpen = K.pack_penalties(rep, pres, freq, [[0]] * B, V, "cuda")
    variants["penalty_commit"] = lambda: K.penalty_commit(tokens, seq_len, n_commit, cpen, cap)
    tiny = torch.zeros((1, 1, 32), dtype=torch.float32, device="cuda")
    tiny_pen = K.pack_penalties([1.5], [0.0], [0.0], [[0]], 32, "cuda")

    def restore():
        y.copy_(x)
        yd.copy_(x[:, 0])
    info = {"B": B, "K": Kd, "V": V, "dtype": "bf16", "device": torch.cuda.get_device_name(0), "cus": K.device_cu_count(0),
            "bytes": {"target": B * (Kd + 1) * V * 2, "draft": B * V * 2, "seen_bits": B * ((V + 31) // 32) * 4},
            "penalties": {"repetition": rep[0], "presence": pres[0], "frequency": freq[0]}}
    return variants, restore, (lambda: K.penalty_rows(tiny, tiny_pen)), info


def worker(a) -> int:
    """Under the profiler: a warm-up call of everything, then per variant a restore, one separator launch and `--calls` calls."""
    import torch
    variants, restore, separator, _ = build_variants(a)
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    for fn in variants.values():
        restore()
        separator()
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
    restore()
    separator()
    torch.cuda.synchronize()
    return 0


def stage_step(a):
    """Wall time per verifying step of Stage.generate, two tiny stages at the full vocabulary, with and without penalties."""
    import torch
    from asd_amd.serving.stages import StageConfig, StageManager
    from asd_amd.serving.synthetic_lm import tiny
    cfgs = [StageConfig(model_name=f"tiny-{i}", model_size=name, shape=tiny(vocab=a.vocab), model_seed=i, logit_scale=3.0,
                        draft_len=a.draft_len, seed=11 + i) for i, name in enumerate(("8b", "13b"))]
    stage = StageManager(cfgs).get_stage("13b")
    prompts = [f"request number {i} of the batch" for i in range(a.batch)]
    kw = dict(prompts=prompts, max_tokens=32, temperature=0.7, seed=list(range(a.batch)))
    pens = dict(repetition_penalty=1.2, presence_penalty=0.5, frequency_penalty=0.25)
    runs = (("without", {}), ("with", pens))
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
                   "whole call divided by its steps; `without` makes exactly the ops calls made before the penalties existed")
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "penalties_step.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--draft-len", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--seen", type=int, nargs="*", default=[16, 256, 2048], help="distinct seen tokens per row")
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
        directory = os.path.abspath(a.trace_dir) if keep else tempfile.mkdtemp(prefix="penalties_trace_")
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", directory, "--", sys.executable, os.path.abspath(__file__),
               "--worker", "--batch", str(a.batch), "--draft-len", str(a.draft_len), "--vocab", str(a.vocab), "--calls", str(a.calls),
               "--seen", *map(str, a.seen)]
        try:
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        except (OSError, subprocess.SubprocessError) as e:
            trace_error = f"{type(e).__name__}: {e}"
    # 2. the per-call figures from Python, profiler off
    import torch
    variants, restore, _, info = build_variants(a)
    if not a.no_trace and trace_error is None:
        try:
            trace = parse_trace(directory, list(variants), a.calls, SEPARATOR, trailing=RESTORE_KERNELS)
        except (RuntimeError, KeyError, ValueError) as e:
            trace_error = f"{type(e).__name__}: {e}"
    times = {k: [] for k in variants}
    for rnd in range(a.rounds + 1):                         # round 0: warm-up
        for name, fn in variants.items():
            restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            if rnd:
                times[name].append(1e3 * e0.elapsed_time(e1) / a.calls)
    res = {"what": "asd_penalty_rows / asd_penalty_commit next to vLLM's apply_penalties written in torch, on the same tensors, "
                   "one call each", **info, "rounds": a.rounds, "calls_per_round": a.calls}
    if trace_error is not None:
        res["trace_error"] = trace_error
    for name, t in times.items():
        res[name] = {"us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2)}
        if trace is not None:
            k = trace[name]
            res[name].update(kernel_us=round(statistics.median(k["us"]), 2), kernel_us_min=round(min(k["us"]), 2),
                             kernel_us_max=round(max(k["us"]), 2), kernels_per_call=k["kernels_per_call"], kernel=k["kernel"])
    key = "kernel_us" if trace is not None else "us_median"
    for n in a.seen:
        for tail in ("", "_draft"):
            own = res[f"penalty_rows_{n}{tail}"]
            own["ratio_to_torch"] = round(own[key] / res[f"torch_{n}{tail}"][key], 4)
    res["ratios_from"] = key
    if not a.no_stage:
        del variants, restore
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
