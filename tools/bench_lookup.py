#!/usr/bin/env python3
"""Time one prompt-lookup launch (asd_lookup_propose, K = 8, N = 3, n0 = 1, with bf16 one-hot rows at V = 152064) beside the
closest existing kernel, asd_no_repeat_ngram_rows with K1 = 1 and n = 3 -- one scan of a history per row -- on the same
histories, for B in (1, 32) and history lengths 512, 4096 and 32768: random token ids over the vocabulary whose last 64
tokens repeat an earlier stretch, so both kernels find one long match and few short ones.  And count the steps Stage.generate
takes for 128 greedy tokens on a self-repeating prompt at the Qwen2.5-7B shape with and without prompt_lookup_num_tokens = 8.

    python tools/bench_lookup.py [--out profiles/lookup.json] [--repeats 30]

Kernel time comes from a `rocprofv3 --kernel-trace --stats` run OF ITS OWN per (B, length) (no counters, no other tracing):
this script starts itself once more under the profiler as a fresh child process (`--worker`) before it touches the GPU; each
child is one GPU step under its own time limit, and a failure ends the tool.  A child launches the two kernels in alternation,
`--repeats` times after 3 warm-up rounds.  The step count is a child of its own without the profiler (`--steps-worker`).
Reported per shape: the median, minimum, maximum and quartiles of both kernels, the ratio of the medians and the baseline's
spread.  This is a measurement, not a pass mark.  Needs a GPU: there is no fallback."""
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

K, N, N0, V = 8, 3, 1, 152064
SHAPES = tuple((b, n) for b in (1, 32) for n in (512, 4096, 32768))
STEP_LIMIT_S, STEPS_LIMIT_S, TOKENS = 300, 600, 128
KERNELS = {"lookup": "k_lookup_propose", "ngram": "k_no_repeat_ngram_rows"}


def worker(a) -> int:
    import torch
    from asd_amd import kernels as Kn
    B, n = a.batch, a.length
    g = torch.Generator(device="cuda").manual_seed(1)
    tokens = torch.randint(0, V, (B, n + 8), generator=g, device="cuda", dtype=torch.int32)
    tokens[:, n - 64:n] = tokens[:, n // 4:n // 4 + 64]                      # the suffix occurred before
    seq_len = torch.full((B,), n, dtype=torch.int32, device="cuda")
    row_start = torch.zeros((B,), dtype=torch.int32, device="cuda")
    tok = torch.full((B, K), -1, dtype=torch.int32, device="cuda")
    matched, counter = (torch.zeros((B,), dtype=torch.int32, device="cuda") for _ in range(2))
    onehot = torch.full((B, K, V), float("-inf"), dtype=torch.bfloat16, device="cuda")
    logits = torch.zeros((B, V), dtype=torch.bfloat16, device="cuda")
    ngram = Kn.pack_no_repeat_ngram([N] * B, [n] * B, n, "cuda")
    torch.cuda.synchronize()
    for _ in range(WARMUP + a.repeats):
        Kn.lookup_propose(tokens, seq_len, n, n + 8, tok, matched, N, N0, row_start, counter, onehot)
        Kn.no_repeat_ngram_rows(logits, ngram, tokens, seq_len, n + 8)
    torch.cuda.synchronize()
    # sane answers behind the timing: the three-token match, and what followed it
    assert bool((matched == N).all()) and torch.equal(tok, tokens[:, n // 4 + 64:n // 4 + 64 + K]), (matched, tok)
    return 0


def steps_worker(a) -> int:
    import torch
    from asd_amd.serving.stages import StageConfig, StageManager
    stage = StageManager([StageConfig(model_name="qwen2.5-7b", model_size="8b", cost_per_token=1.0)]).get_stage("8b")
    prompt = " ".join(["the quick brown fox jumps over the lazy dog ."] * 6)
    out = {}
    for name, kw in (("plain", {}), ("lookup", dict(prompt_lookup_num_tokens=K))):
        texts, _, stats = stage.generate(prompts=[prompt], max_tokens=TOKENS, temperature=0.0, **kw)
        out[name] = {"steps": int(stats["steps"]), "tokens": len(texts[0].split()), "ms": round(stats["generation_time_ms"], 1),
                     "matched_steps": stats.get("lookup_matched_steps")}
        out.setdefault("texts", []).append(texts[0])
    out["same_text"] = out["texts"][0] == out.pop("texts")[1]
    torch.cuda.synchronize()
    with open(a.steps_out, "w") as f:
        json.dump(out, f)
    return 0


def parse_trace(directory, repeats):
    """The kernel-trace CSV(s) under `directory` -> {kernel: [kernel time in us of the last `repeats` dispatches]}."""
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
    out = {k: [(e - s) / 1e3 for s, e, name in rows if sym in name.replace(" ", "")] for k, sym in KERNELS.items()}
    for k, t in out.items():
        if len(t) != WARMUP + repeats:
            raise RuntimeError(f"{len(t)} {KERNELS[k]} dispatches in the trace, expected {WARMUP + repeats}")
    return {k: t[-repeats:] for k, t in out.items()}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup.json"))
    ap.add_argument("--batch", type=int, default=32, help=argparse.SUPPRESS)
    ap.add_argument("--length", type=int, default=4096, help=argparse.SUPPRESS)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--steps-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--steps-out", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if a.steps_worker:
        return steps_worker(a)

    res = {"what": "asd_lookup_propose (K = 8, max_ngram 3, min_ngram 1, bf16 one-hot rows at V = 152064) vs asd_no_repeat_ngram_rows "
                   "(K1 = 1, n = 3, bf16 logits) on the same histories (random ids, the last 64 tokens repeat an earlier stretch): "
                   "kernel time from a rocprofv3 --kernel-trace --stats run of its own per shape, the two launched in alternation "
                   "in one process; and the steps of 128 greedy tokens on a self-repeating prompt at the Qwen2.5-7B shape",
           "K": K, "max_ngram": N, "min_ngram": N0, "V": V, "repeats": a.repeats, "warmup_rounds": WARMUP}
    try:
        for B, n in SHAPES:
            entry = res[f"B={B},len={n}"] = {"history_bytes": B * n * 4}
            directory = tempfile.mkdtemp(prefix="lookup_trace_")
            try:
                run_step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", directory, "--", sys.executable,
                          os.path.abspath(__file__), "--worker", "--batch", str(B), "--length", str(n), "--repeats", str(a.repeats)],
                         STEP_LIMIT_S)                                       # one GPU step, under its own limit
                for k, t in parse_trace(directory, a.repeats).items():
                    q = statistics.quantiles(t, n=4)
                    entry[k] = {"us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                                "us_p25": round(q[0], 2), "us_p75": round(q[2], 2)}
                base = entry["ngram"]
                entry["baseline_spread"] = round((base["us_max"] - base["us_min"]) / base["us_median"], 4)
                entry["lookup_over_ngram"] = round(entry["lookup"]["us_median"] / base["us_median"], 4)
            finally:
                shutil.rmtree(directory, ignore_errors=True)
        fd, path = tempfile.mkstemp(prefix="lookup_steps_", suffix=".json")
        os.close(fd)
        try:
            run_step([sys.executable, os.path.abspath(__file__), "--steps-worker", "--steps-out", path], STEPS_LIMIT_S)
            with open(path) as f:
                res["steps_per_128_tokens"] = json.load(f)
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
