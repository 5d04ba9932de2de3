#!/usr/bin/env python3
"""Time the sparse logit edit (asd_logit_edit_rows) at the verify loop's shape, B = 32, K = 8, V = 152064, bf16, with 16 and
with 1024 entries per row, next to the samplers of the same step in the same process:

  logit_edit_N          one call on the target's [B, K+1, V] output, every row with its own N entries (row_first form)
  logit_edit_N_draft    one call on one proposal's [B, V] draft logits (a verifying step makes K of these)
  draft_sample          asd_draft_sample on [B, V] (top-p 0.9)
  verify_accept         asd_verify_accept on the [B, K, V] score rows
  residual_sample_lp    asd_residual_sample_lp on the same rows
  top_logprobs          asd_top_logprobs (N = 5) on [B, K+1, V]

    python tools/bench_logit_edit.py [--out profiles/logit_edit_step.json] [--rounds 15] [--calls 40]

The samplers are not touched by the edit's pull request, so their figures are what the step cost before it.  Half of a row's
entries are permanent bans, half carry a bias small enough that repeating the call does not move the values (the store is made
all the same).  The edit is timed on a copy of the tensor the samplers read.  The variants are timed in alternation (one
device-event pair around `--calls` back-to-back calls, `--rounds` rounds after a warm-up round); the figure is the median
per-call time, the spread its min .. max.  Needs a GPU: there is no fallback."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logit_edit_step.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--draft-len", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--entries", type=int, nargs="*", default=[16, 1024])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=40)
    a = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_logit_edit.py needs a GPU (no fallback)")
    from asd_amd import kernels as K
    from asd_amd.distributed import HipOps

    B, Kd, V = a.batch, a.draft_len, a.vocab
    inv_t = float(np.float32(1 / 0.7))
    g = torch.Generator(device="cuda").manual_seed(1)
    x = (torch.randn((B, Kd + 1, V), generator=g, device="cuda") * 4.0).to(torch.bfloat16)
    d = (x[:, :Kd].float() + 0.5 * torch.randn((B, Kd, V), generator=g, device="cuda")).to(torch.bfloat16).contiguous()
    score, bonus, dl = x[:, :Kd].contiguous(), x[:, Kd].contiguous(), d[:, 0].contiguous()
    y, yd = x.clone(), dl.clone()                            # what the edit is timed on
    seq_len = torch.full((B,), 40, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(1)
    FOREVER = K.EDIT_FOREVER

    def pack(n):
        rows = [[(int(t), 0.0 if i % 2 else 2.0 ** -10, FOREVER if i % 2 else 0)
                 for i, t in enumerate(rng.choice(V, n, replace=False))] for _ in range(B)]
        return K.pack_logit_edits(rows, "cuda"), rows

    ops = HipOps()
    r = torch.rand((B,), generator=g, device="cuda")
    u = torch.rand((B, Kd), generator=g, device="cuda")
    toks, lpd, thr = [], [], []
    for k in range(Kd):
        t, lp, th = ops.draft_sample(d[:, k].contiguous(), r, inv_t, 0.9)
        toks.append(t), lpd.append(lp), thr.append(th)
    tok = torch.stack(toks, 1).to(torch.int32).contiguous()
    lp_d, d_thr = torch.stack(lpd, 1).contiguous(), torch.stack(thr, 1).contiguous()
    n_acc = ops.verify_accept(score, tok, lp_d, u, inv_t)[2]

    variants = {}
    for n in a.entries:
        packed, rows = pack(n)
        # the same answer before any timing: every banned element is -inf, nothing else became -inf
        K.logit_edit_rows(y, packed, seq_len, 32, 0)
        torch.cuda.synchronize()
        want = sum(1 for row in rows for e in row if e[2]) * (Kd + 1)
        assert int(torch.isneginf(y).sum()) == want, (n, int(torch.isneginf(y).sum()), want)
        y.copy_(x)
        variants[f"logit_edit_{n}"] = lambda p=packed: K.logit_edit_rows(y, p, seq_len, 32, 0)
        variants[f"logit_edit_{n}_draft"] = lambda p=packed: K.logit_edit_rows(yd, p, seq_len, 32, 3)
    variants["draft_sample"] = lambda: ops.draft_sample(dl, r, inv_t, 0.9)
    variants["verify_accept"] = lambda: ops.verify_accept(score, tok, lp_d, u, inv_t)
    variants["residual_sample_lp"] = lambda: ops.residual_sample_lp(score, d, n_acc, r, bonus, inv_t, d_threshold=d_thr)
    variants["top_logprobs"] = lambda: ops.top_logprobs(x, 5, inv_t)

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
    ops.check_status()
    res = {"what": "asd_logit_edit_rows next to the samplers of one sampled verifying step, one call each",
           "B": B, "K": Kd, "V": V, "dtype": "bf16", "rounds": a.rounds, "calls_per_round": a.calls,
           "device": torch.cuda.get_device_name(0), "cus": K.device_cu_count(0)}
    for name, t in times.items():
        res[name] = {"us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
