#!/usr/bin/env python3
"""Time the watermark pass (asd_watermark_rows) against the shaping pass in quadratic mode (asd_logit_shape_rows), the other
pass that rewrites whole rows, on one bf16 tensor [B, K1, 152064] for (B, K1) = (32, 9) (a verifying step's output at K = 8:
88 MB), (32, 1) (stage 0) and (1, 1) (the shape the row split exists for), all variants of a shape in the same process on copies
of the same values:

  quadratic   asd_logit_shape_rows, f = 0.3, c = 1                  -- the baseline: one 1024-lane workgroup per row, two sweeps
  wm_025      asd_watermark_rows, gamma 0.25, delta 2, context 1    -- one Philox call per 16-byte vector, 90 % of them stored
  wm_050      asd_watermark_rows, gamma 0.5                         -- 99.6 % of the vectors stored
  wm_025_mis  asd_watermark_rows, gamma 0.25, the base one element off a 16-byte boundary -- two Philox calls per vector

    python tools/bench_watermark.py [--out profiles/watermark.json] [--repeats 30]

The passes work in place, so every round restores the tensor from a pristine copy before each launch (the copies are torch
kernels and are not counted).  Kernel time comes from a `rocprofv3 --kernel-trace --stats` run OF ITS OWN per shape (no
counters, no other tracing): this script starts itself once more under the profiler as a fresh child process (`--worker`)
before it touches the GPU; each child is one GPU step under its own time limit, and a failure ends the tool.  A child launches
the four in alternation, `--repeats` times after 3 warm-up rounds; the three asd_watermark_rows dispatches of a round are told
apart by their position in it.  Reported per shape and variant: the median, minimum, maximum and quartiles over the repeats, the
ratio of each median to the baseline's, the baseline's spread, and the two floors of the pass computed from the shape: bytes
(the rows read once, and the share of vectors that hold a green element written once) and per-lane 32 x 32 -> 64 products (19
per Philox call).  This is a measurement, not a pass mark.  Needs a GPU: there is no fallback."""
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

VARIANTS = ("quadratic", "wm_025", "wm_050", "wm_025_mis")
FACTOR, CURVE, TEMPERATURE, DELTA, KEY = 0.3, 1.0, 0.7, 2.0, 0x0123456789ABCDEF
SHAPES = ((32, 9), (32, 1), (1, 1))
STEP_LIMIT_S = 300
PRODUCTS_PER_CALL = 19                           # ten rounds of two products; round 1's M1 * b is uniform


def worker(a) -> int:
    import torch
    from asd_amd import kernels as K
    B, K1, V = a.batch, a.rows, a.vocab
    g = torch.Generator(device="cuda").manual_seed(1)
    x0 = (torch.randn((B, K1, V), generator=g, device="cuda") * 3.0).to(torch.bfloat16)
    flat0 = torch.cat([x0.flatten(), x0.flatten()[:8]])                      # the same values one element off a 16-byte boundary
    x, y, flat = x0.clone(), x0.clone(), flat0.clone()
    off = flat[1:1 + B * K1 * V].view(B, K1, V)
    quad = K.pack_logit_shape([TEMPERATURE] * B, [K.SHAPE_QUADRATIC] * B, [FACTOR] * B, [CURVE] * B, "cuda")
    wm = {gamma: K.pack_watermark([KEY + b for b in range(B)], [DELTA] * B, [gamma] * B, [1] * B, [4] * B, 4, "cuda") for gamma in (0.25, 0.5)}
    tokens = torch.randint(0, V, (B, 16), generator=g, device="cuda", dtype=torch.int32)
    seq_len = torch.full((B,), 12, dtype=torch.int32, device="cuda")
    step_tok = torch.randint(0, V, (B, 8), generator=g, device="cuda", dtype=torch.int32) if K1 > 1 else None
    torch.cuda.synchronize()
    for _ in range(WARMUP + a.repeats):
        x.copy_(x0)
        K.logit_shape_rows(x, quad)
        for t, t0, view, packed in ((y, x0, y, wm[0.25]), (y, x0, y, wm[0.5]), (flat, flat0, off, wm[0.25])):
            t.copy_(t0)
            K.watermark_rows(view, packed, tokens, seq_len, 16, step_tok, 0)
    torch.cuda.synchronize()
    # sane answers behind the timing: gamma 0.5 raised half of the elements by delta, and the misaligned form found the same ones
    share = float((y != x0).float().mean())
    assert abs(share - 0.5) < 0.01, share
    assert torch.equal(flat[1:1 + B * K1 * V] != flat0[1:1 + B * K1 * V], (K.watermark_rows(x0.clone(), wm[0.25], tokens, seq_len, 16, step_tok, 0) != x0).flatten())
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
    base = [(e - s) / 1e3 for s, e, name in rows if "k_logit_shape_rows" in name.replace(" ", "")]
    marked = [(e - s) / 1e3 for s, e, name in rows if "k_watermark_rows" in name.replace(" ", "")]
    rounds = WARMUP + repeats
    if len(base) != rounds or len(marked) != 3 * rounds + 1:                 # the check behind the loop launches one pass
        raise RuntimeError(f"{len(base)} asd_logit_shape_rows and {len(marked)} asd_watermark_rows dispatches in the trace, "
                           f"expected {rounds} and {3 * rounds + 1}")
    out = {"quadratic": base}
    out.update({v: marked[i:3 * rounds:3] for i, v in enumerate(VARIANTS[1:])})
    return {v: t[-repeats:] for v, t in out.items()}


def floors(rows, vocab, gamma):
    """What the shape alone says the pass must move and multiply: bytes and per-lane products."""
    vectors = rows * vocab // 8
    written = 1.0 - (1.0 - gamma) ** 8                                       # the share of vectors that hold a green element
    return {"bytes": int(vectors * 16 * (1.0 + written)), "philox_calls": vectors, "lane_products": vectors * PRODUCTS_PER_CALL}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "watermark.json"))
    ap.add_argument("--batch", type=int, default=32, help=argparse.SUPPRESS)
    ap.add_argument("--rows", type=int, default=9, help=argparse.SUPPRESS)
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)

    res = {"what": "asd_watermark_rows (delta 2, context 1, a key per sequence; gamma 0.25, gamma 0.5, and gamma 0.25 with the base "
                   "one element off a 16-byte boundary: two Philox calls per vector; N(0, 3^2) logits) vs asd_logit_shape_rows "
                   "(quadratic, f = 0.3, c = 1) on copies of one [B, K1, V] bf16 tensor: kernel time from a rocprofv3 --kernel-trace "
                   "--stats run of its own per shape, the four launched in alternation in one process, the tensor restored before "
                   "every pass",
           "V": a.vocab, "dtype": "bf16", "repeats": a.repeats, "warmup_rounds": WARMUP}
    for B, K1 in SHAPES:
        entry = res[f"B={B},K1={K1}"] = {"rows": B * K1, "logit_bytes": B * K1 * a.vocab * 2,
                                         "floor_gamma_025": floors(B * K1, a.vocab, 0.25), "floor_gamma_050": floors(B * K1, a.vocab, 0.5)}
        directory = tempfile.mkdtemp(prefix="watermark_trace_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", directory, "--", sys.executable,
               os.path.abspath(__file__), "--worker", "--batch", str(B), "--rows", str(K1), "--vocab", str(a.vocab),
               "--repeats", str(a.repeats)]
        try:
            run_step(cmd, STEP_LIMIT_S)                                      # one GPU step, under its own limit
            times = parse_trace(directory, a.repeats)
            for v in VARIANTS:
                t = times[v]
                q = statistics.quantiles(t, n=4)
                entry[v] = {"us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                            "us_p25": round(q[0], 2), "us_p75": round(q[2], 2)}
            base = entry["quadratic"]
            entry["baseline_spread"] = round((base["us_max"] - base["us_min"]) / base["us_median"], 4)
            entry["baseline_quartile_spread"] = round((base["us_p75"] - base["us_p25"]) / base["us_median"], 4)
            for v in VARIANTS[1:]:
                entry[f"{v}_over_baseline"] = round(entry[v]["us_median"] / base["us_median"], 4)
        except (OSError, subprocess.SubprocessError, RuntimeError, KeyError) as e:
            res["trace_error"] = f"B={B},K1={K1}: {type(e).__name__}: {e}"
            break                                                            # a step failed: nothing more is started on the GPU
        finally:
            shutil.rmtree(directory, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 1 if "trace_error" in res else 0


if __name__ == "__main__":
    sys.exit(main())
