#!/usr/bin/env python3
"""Time the per-token statistics pass (asd_token_stats) against the passes it shares its body with, on one bf16 tensor
[32, 9, 152064] (a verifying step's output at B = 32, K = 8: 88 MB), all in the same process on the same tensor:

  top_logprobs_n5        asd_top_logprobs, N = 5                   -- the baseline of the N = 5 variants
  prompt_logprobs_n0     asd_prompt_logprobs, N = 0, every row     -- the baseline of the N = 0 variants (rank and log-prob, no list)
  token_stats_n5_all     asd_token_stats, N = 5, n_acc = K         -- all rows live: the table, the rank, the arg-max, the entropy
  token_stats_n0_all     asd_token_stats, N = 0, n_acc = K         -- no table: the arg-max alone beside the rank and the entropy
  token_stats_n5_mixed   asd_token_stats, N = 5, n_acc uniform in 0..K   -- rows behind n_acc are not streamed
  token_stats_n0_mixed   asd_token_stats, N = 0, n_acc uniform in 0..K

    python tools/bench_token_stats.py [--out profiles/token_stats.json] [--repeats 30] [--no-trace]

Kernel time comes from a `rocprofv3 --kernel-trace --stats` run OF ITS OWN (no counters, no other tracing): this script starts
itself once more under the profiler as a fresh child process (`--worker`) before it touches the GPU; the child launches the six
in alternation, `--repeats` times after 3 warm-up rounds, and the dispatches are attributed by kernel name and, within a name,
by their position in the round.  Reported per variant: the median, minimum, maximum and quartiles over the repeats, the ratios
of the medians to their baselines', and the baselines' spread ((max - min) / median and (p75 - p25) / median).  This is a
measurement, not a pass mark.  Needs a GPU: there is no fallback."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP = 3
# the order of a round; the four asd_token_stats launches are told apart by it
VARIANTS = ("top_logprobs_n5", "prompt_logprobs_n0", "token_stats_n5_all", "token_stats_n0_all", "token_stats_n5_mixed",
            "token_stats_n0_mixed")


def worker(a) -> int:
    import torch
    from asd_amd import kernels as K
    B, K1, V = a.batch, a.rows, a.vocab
    g = torch.Generator(device="cuda").manual_seed(1)
    x = (torch.randn((B, K1, V), generator=g, device="cuda") * 4.0).to(torch.bfloat16)
    tok = torch.randint(0, V, (B, K1 - 1), generator=g, device="cuda", dtype=torch.int32)
    drawn = torch.randint(0, V, (B,), generator=g, device="cuda", dtype=torch.int32)
    full = torch.full((B,), K1 - 1, device="cuda", dtype=torch.int32)
    mixed = torch.randint(0, K1, (B,), generator=g, device="cuda", dtype=torch.int32)
    target = torch.cat([tok, drawn[:, None]], 1).contiguous()
    top = K.TopLogprobs(B, K1, V, torch.bfloat16, 5)
    p0 = K.PromptLogprobs(B, K1, V, torch.bfloat16, 0)
    s5 = K.TokenStats(B, K1, V, torch.bfloat16, 5)
    s0 = K.TokenStats(B, K1, V, torch.bfloat16, 0)
    # same answers before any timing: the table and the arg-max bit for bit, the rank against asd_prompt_logprobs', the entropy
    # against torch on two sequences
    ids, lps = top(x, out=top.out)
    _, rank, _, _ = p0(x, target)
    sid, sval, tid, tlp = s5(x, tok, full, drawn)
    sid0, sval0, _, _ = s0(x, tok, full, drawn)
    logp = torch.log_softmax(x[:2].double(), -1)
    ent = -(logp.exp() * logp).sum(-1)
    torch.cuda.synchronize()
    assert torch.equal(ids, tid) and torch.equal(lps.view(torch.int32), tlp.view(torch.int32))
    assert torch.equal(sid[..., 1], ids[..., 0]) and torch.equal(sval[..., 1].view(torch.int32), lps[..., 0].view(torch.int32))
    assert torch.equal(sid, sid0) and torch.equal(sval.view(torch.int32), sval0.view(torch.int32))
    assert torch.equal(sid[..., 0], rank) and float((sval[:2, :, 0].double() - ent).abs().max()) < 1e-4
    for _ in range(WARMUP + a.repeats):
        top(x, out=top.out)
        p0(x, target)
        s5(x, tok, full, drawn)
        s0(x, tok, full, drawn)
        s5(x, tok, mixed, drawn)
        s0(x, tok, mixed, drawn)
    torch.cuda.synchronize()
    return 0


def _column(fields, *names):
    low = {f.lower(): f for f in fields}
    for n in names:
        if n in low:
            return low[n]
    raise KeyError(f"none of {names} among the trace's columns {fields}")


def _kind(kernel_name: str):
    """top / prompt / stats5 / stats0 from the (demangled or mangled) kernel name; None for anything else."""
    name = kernel_name.replace(" ", "")
    if "k_top_logprobs" in name:
        return "top"
    if "k_prompt_logprobs" in name:
        return "prompt"
    m = re.search(r"k_token_stats(?:<\d+,\w+,(\d+)>|ILi\d+ELb\d+ELi(\d+)E)", name)
    if m:
        return "stats5" if (m.group(1) or m.group(2)) == "3" else "stats0"
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
    by_kind = {"top": [], "prompt": [], "stats5": [], "stats0": []}
    for s, e, name in rows:
        k = _kind(name)
        if k is not None:
            by_kind[k].append((e - s) / 1e3)
    rounds = WARMUP + repeats
    # the checks ahead of the loop launch each kernel once; a round then launches top, prompt, stats5, stats0, stats5, stats0
    need = {"top": 1 + rounds, "prompt": 1 + rounds, "stats5": 1 + 2 * rounds, "stats0": 1 + 2 * rounds}
    for k, n in need.items():
        if len(by_kind[k]) != n:
            raise RuntimeError(f"{k}: {len(by_kind[k])} dispatches in the trace, expected {n}")
    s5, s0 = by_kind["stats5"][1:], by_kind["stats0"][1:]
    out = {"top_logprobs_n5": by_kind["top"][1:], "prompt_logprobs_n0": by_kind["prompt"][1:],
           "token_stats_n5_all": s5[0::2], "token_stats_n0_all": s0[0::2],
           "token_stats_n5_mixed": s5[1::2], "token_stats_n0_mixed": s0[1::2]}
    return {v: t[-repeats:] for v, t in out.items()}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_stats.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rows", type=int, default=9, help="K1: rows per sequence (draft_len + 1)")
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--trace-dir", default=None, help="keep the profiler's output here (default: a temporary directory)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)

    nbytes = a.batch * a.rows * a.vocab * 2
    res = {"what": "asd_token_stats (N = 5, N = 0; all rows live, n_acc uniform in 0..K) vs asd_top_logprobs (N = 5) and "
                   "asd_prompt_logprobs (N = 0) on one [B, K1, V] bf16 tensor: kernel time from a rocprofv3 --kernel-trace --stats "
                   "run of its own, the six launched in alternation in one process",
           "B": a.batch, "K1": a.rows, "V": a.vocab, "dtype": "bf16", "rows": a.batch * a.rows, "logit_bytes": nbytes,
           "repeats": a.repeats, "warmup_rounds": WARMUP}
    keep = a.trace_dir is not None
    directory = os.path.abspath(a.trace_dir) if keep else tempfile.mkdtemp(prefix="token_stats_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", directory, "--", sys.executable,
           os.path.abspath(__file__), "--worker", "--batch", str(a.batch), "--rows", str(a.rows), "--vocab", str(a.vocab),
           "--repeats", str(a.repeats)]
    try:
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        times = parse_trace(directory, a.repeats)
        for v in VARIANTS:
            t = times[v]
            med = statistics.median(t)
            q = statistics.quantiles(t, n=4)
            res[v] = {"us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                      "us_p25": round(q[0], 2), "us_p75": round(q[2], 2)}
        med = lambda v: res[v]["us_median"]                                                   # noqa: E731
        for base in ("top_logprobs_n5", "prompt_logprobs_n0"):
            b = res[base]
            res[base + "_spread"] = round((b["us_max"] - b["us_min"]) / b["us_median"], 4)
            res[base + "_quartile_spread"] = round((b["us_p75"] - b["us_p25"]) / b["us_median"], 4)
        res["n5_all_over_top_logprobs_n5"] = round(med("token_stats_n5_all") / med("top_logprobs_n5"), 4)
        res["n0_all_over_prompt_logprobs_n0"] = round(med("token_stats_n0_all") / med("prompt_logprobs_n0"), 4)
        res["n0_all_over_top_logprobs_n5"] = round(med("token_stats_n0_all") / med("top_logprobs_n5"), 4)
        res["n5_mixed_over_n5_all"] = round(med("token_stats_n5_mixed") / med("token_stats_n5_all"), 4)
        res["n0_mixed_over_n0_all"] = round(med("token_stats_n0_mixed") / med("token_stats_n0_all"), 4)
        res["n0_all_slower_than_prompt_n0_beyond_its_spread"] = bool(
            res["n0_all_over_prompt_logprobs_n0"] - 1.0 > res["prompt_logprobs_n0_spread"])
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
