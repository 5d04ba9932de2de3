#!/usr/bin/env python3
"""Time the greedy step (asd_verify_greedy) at B = 32, K = 8, V = 152064, bf16 against two yardsticks on the same tensor:

  greedy   asd_verify_greedy on the target's [B, K+1, V] output, in place (arg-max, lp, accepted prefix, commit token)
  verify   the plain asd_verify_accept kernel over the same number of rows ([B, K+1, V] treated as K + 1 verify rows)
  torch    argmax + log_softmax (f32) + gather

    python tools/bench_greedy.py [--out profiles/greedy_step.json] [--rounds 15] [--calls 40]

The three are timed in alternation (one device-event pair around `--calls` back-to-back calls, `--rounds` rounds, after a
warm-up round of every shape); the figure is the median per-call time over the rounds, the spread its min .. max.  The 88 MB
tensor is re-read every call, so part of it is served by the 256 MB last-level cache: that holds for all three alike.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "greedy_step.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--draft-len", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=40)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_greedy.py needs a GPU (no fallback)")
    from asd_amd import kernels as K

    B, Kd, V = a.batch, a.draft_len, a.vocab
    g = torch.Generator(device="cuda").manual_seed(1)
    x = (torch.randn((B, Kd + 1, V), generator=g, device="cuda") * 4.0).to(torch.bfloat16)
    am = x.float().argmax(-1).to(torch.int32)
    tok = torch.where(torch.rand((B, Kd), generator=g, device="cuda") < 0.7, am[:, :Kd],
                      torch.randint(0, V, (B, Kd), generator=g, device="cuda", dtype=torch.int32)).contiguous()

    greedy = K.GreedyVerifier(B, Kd, V, torch.bfloat16)
    ws = K.VerifyWorkspace(B, Kd + 1, V, torch.bfloat16)
    tok_all = torch.cat([tok, am[:, Kd:]], 1).contiguous()
    lp_d = torch.zeros((B, Kd + 1), device="cuda")
    u = torch.full((B, Kd + 1), 0.5, device="cuda")
    v_out = K.verify_accept(x, tok_all, lp_d, u, ws)

    def run_greedy():
        return greedy(x, tok, out=greedy.out)

    def run_verify():
        return K.verify_accept(x, tok_all, lp_d, u, ws, v_out)

    def run_torch():
        idx = x.argmax(-1, keepdim=True)
        return idx, torch.log_softmax(x, -1, dtype=torch.float32).gather(-1, idx)

    # same answers before any timing: the arg-max against torch's where the row has one maximum, lp against its log_softmax
    r = run_greedy()
    idx, lp = run_torch()
    torch.cuda.synchronize()
    top2 = x.float().topk(2, -1).values
    single = (top2[..., 0] > top2[..., 1])
    assert bool((r.argmax.long()[single] == idx[..., 0][single]).all())
    assert float((r.lp_argmax - lp[..., 0])[single].abs().max()) < 1e-4

    variants = {"greedy": run_greedy, "verify": run_verify, "torch": run_torch}
    times = {k: [] for k in variants}
    for rnd in range(a.rounds + 1):                         # round 0: warm-up of every shape
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
    res = {"what": "greedy step vs the plain verify kernel vs torch argmax + log_softmax + gather, one call each on [B, K+1, V]",
           "B": B, "K": Kd, "V": V, "dtype": "bf16", "rows": B * (Kd + 1), "logit_bytes": nbytes, "rounds": a.rounds,
           "calls_per_round": a.calls, "device": torch.cuda.get_device_name(0), "cus": K.device_cu_count(0)}
    for name, t in times.items():
        med = statistics.median(t)
        res[name] = {"us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                     "logit_gbps": round(nbytes / (med * 1e-6) / 1e9, 1)}
    res["greedy_over_verify"] = round(res["greedy"]["us_median"] / res["verify"]["us_median"], 3)
    res["torch_over_greedy"] = round(res["torch"]["us_median"] / res["greedy"]["us_median"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
