#!/usr/bin/env python3
"""Time the top-N log-prob pass (asd_top_logprobs, N = 5) at B = 32, K = 8, V = 152064, bf16 against the greedy step on the
same tensor in the same process:

  top_logprobs   asd_top_logprobs on the target's [B, K+1, V] output, in place (the 5 most likely tokens and their log-probs)
  greedy         asd_verify_greedy on the same rows (arg-max, lp, accepted prefix, commit token)

    python tools/bench_top_logprobs.py [--out profiles/top_logprobs_step.json] [--rounds 15] [--calls 40] [--n 5]

Both kernels read the same bytes with the same geometry (rows x splits workgroups of 512 lanes, 16-byte loads, two batches in
flight), so their ratio is the price of keeping 8 sorted (value, id) pairs per lane beside the log-sum-exp.  The two are timed
in alternation (one device-event pair around `--calls` back-to-back calls, `--rounds` rounds, after a warm-up round); the figure
is the median per-call time over the rounds, the spread its min .. max.  The 88 MB tensor is re-read every call, so part of it
is served by the 256 MB last-level cache: that holds for both alike.  `--splits` sweeps explicit geometries as well.
Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "top_logprobs_step.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--draft-len", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--splits", type=int, nargs="*", default=[], help="explicit workgroups-per-row values to time as well")
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_top_logprobs.py needs a GPU (no fallback)")
    from asd_amd import kernels as K

    B, Kd, V = a.batch, a.draft_len, a.vocab
    g = torch.Generator(device="cuda").manual_seed(1)
    x = (torch.randn((B, Kd + 1, V), generator=g, device="cuda") * 4.0).to(torch.bfloat16)
    am = x.float().argmax(-1).to(torch.int32)
    tok = torch.where(torch.rand((B, Kd), generator=g, device="cuda") < 0.7, am[:, :Kd],
                      torch.randint(0, V, (B, Kd), generator=g, device="cuda", dtype=torch.int32)).contiguous()

    top = K.TopLogprobs(B, Kd + 1, V, torch.bfloat16, a.n)
    greedy = K.GreedyVerifier(B, Kd, V, torch.bfloat16)

    # same answers before any timing: the ids against torch.topk where the n + 1 largest values of a row are distinct (topk's
    # order among equal values is not the kernel's), the log-probs against log_softmax, slot 0 against the greedy step
    ids, lps = top(x, out=top.out)
    r = greedy(x, tok, out=greedy.out)
    ref = torch.log_softmax(x.float(), -1)
    tv, ti = x.float().topk(a.n + 1, -1)
    torch.cuda.synchronize()
    distinct = (tv[..., :-1] > tv[..., 1:]).all(-1)
    assert bool((ids.long()[distinct] == ti[..., :a.n][distinct]).all())
    assert float((lps - ref.gather(-1, ids.long())).abs().max()) < 1e-4
    assert bool((ids[..., 0] == r.argmax).all())

    variants = {"top_logprobs": lambda: top(x, out=top.out), "greedy": lambda: greedy(x, tok, out=greedy.out)}
    for s in a.splits:
        variants[f"top_logprobs_splits{s}"] = lambda s=s: top(x, splits=s, out=top.out)
        variants[f"greedy_splits{s}"] = lambda s=s: greedy(x, tok, splits=s, out=greedy.out)
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
    nbytes = x.numel() * x.element_size()
    res = {"what": "asd_top_logprobs vs asd_verify_greedy, one call each on the same [B, K+1, V] tensor",
           "B": B, "K": Kd, "V": V, "N": a.n, "dtype": "bf16", "rows": B * (Kd + 1), "logit_bytes": nbytes, "rounds": a.rounds,
           "calls_per_round": a.calls, "device": torch.cuda.get_device_name(0), "cus": K.device_cu_count(0)}
    for name, t in times.items():
        med = statistics.median(t)
        res[name] = {"us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                     "logit_gbps": round(nbytes / (med * 1e-6) / 1e9, 1)}
    res["top_logprobs_over_greedy"] = round(res["top_logprobs"]["us_median"] / res["greedy"]["us_median"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
