#!/usr/bin/env python3
"""Time the random numbers of one sampled verifying step at B = 32, K = 8, before and after per-request seeds, in one process:

  torch_rand      the seed=None path of serving/stages.py: K torch.rand((B,)) calls (one per proposal), one torch.rand((B, K))
                  (the accept uniforms) and one torch.rand((B,)) (the commit draw) on the stage's generator -- K + 2 launches
  step_uniforms   the seeded path: ONE HipOps.step_uniforms call (asd_step_uniforms, Philox4x32-10) into a preallocated buffer

    python tools/bench_step_uniforms.py [--out profiles/seeded_step.json] [--rounds 9] [--steps 300]

Per variant and round, `--steps` steps are issued back to back after a device synchronise.  Three figures per step:
  device_us   a device-event pair around the window / steps: what the stream is busy (or waiting for the host) per step
  issue_us    host wall time of the issuing loop / steps: the Python + launch cost the draft loop pays between model passes
  wall_us     host wall time until the window has drained (a synchronise at its end) / steps
The variants alternate within a round; round 0 is a warm-up; the figures are medians over the rounds with min .. max.
Nothing else runs on the stream, so these are the costs of the random numbers alone, not of a decoding step.
Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeded_step.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--draft-len", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=300)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_step_uniforms.py needs a GPU (no fallback)")
    from asd_amd import kernels as K
    from asd_amd.distributed import HipOps

    B, Kd = a.batch, a.draft_len
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    ops = HipOps()
    seeds = torch.arange(42, 42 + B, dtype=torch.int64, device=dev)
    buf = torch.empty(((2 * Kd + 1) * B,), dtype=torch.float32, device=dev)

    def torch_rand(step):
        for _ in range(Kd):
            torch.rand((B,), generator=gen, device=dev)
        torch.rand((B, Kd), generator=gen, device=dev)
        torch.rand((B,), generator=gen, device=dev)

    def step_uniforms(step):
        ops.step_uniforms(seeds, step, 1, Kd, Kd, out=buf)

    # the same call twice gives the same bits, another step does not, and everything lies in [0, 1)
    first = [t.clone() for t in ops.step_uniforms(seeds, 0, 1, Kd, Kd, out=buf)]
    again = [t.clone() for t in ops.step_uniforms(seeds, 0, 1, Kd, Kd, out=buf)]
    other = [t.clone() for t in ops.step_uniforms(seeds, 1, 1, Kd, Kd, out=buf)]
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(first, again)) and not any(torch.equal(x, y) for x, y in zip(first, other))
    assert all(float(x.min()) >= 0.0 and float(x.max()) < 1.0 for x in first)

    variants = {"torch_rand": torch_rand, "step_uniforms": step_uniforms}
    times = {k: {"device_us": [], "issue_us": [], "wall_us": []} for k in variants}
    for rnd in range(a.rounds + 1):                         # round 0: warm-up
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for step in range(a.steps):
                fn(step)
            e1.record()
            t1 = time.perf_counter()
            e1.synchronize()
            t2 = time.perf_counter()
            if rnd:
                times[name]["device_us"].append(1e3 * e0.elapsed_time(e1) / a.steps)
                times[name]["issue_us"].append(1e6 * (t1 - t0) / a.steps)
                times[name]["wall_us"].append(1e6 * (t2 - t0) / a.steps)
    res = {"what": "random numbers of one sampled verifying step: K + 2 torch.rand calls (seed=None) vs one asd_step_uniforms call",
           "B": B, "K": Kd, "launches_per_step": {"torch_rand": Kd + 2, "step_uniforms": 1}, "rounds": a.rounds,
           "steps_per_round": a.steps, "uniforms_per_step": (2 * Kd + 1) * B, "device": torch.cuda.get_device_name(0),
           "cus": K.device_cu_count(0)}
    for name, t in times.items():
        res[name] = {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                     for k, v in t.items()}
    for k in ("device_us", "issue_us", "wall_us"):
        res[f"{k}_ratio_before_over_after"] = round(res["torch_rand"][k]["median"] / res["step_uniforms"][k]["median"], 2)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
