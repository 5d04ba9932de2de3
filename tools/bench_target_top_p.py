#!/usr/bin/env python3
"""Timing of the verify step against the TARGET's nucleus (asd_verify_accept_top_p) beside the plain verify
(asd_verify_accept_ex, full softmax) and the torch composition it replaces: HF's TemperatureLogitsWarper + TopPLogitsWarper on
the GPU, then log_softmax / gather / compare (the target side of HF's assisted generation with generate(temperature=0.7,
top_p=0.9), generate_training_data.py:110-119).  All three on the same rows; the inputs rotate over enough buffers that the
working set exceeds the 256 MB Infinity Cache, so every call reads its rows from HBM.

    python tools/bench_target_top_p.py [--out profiles/target_top_p.json] [--batches 8,32,128]
"""
import argparse
import json
import os
import platform
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from asd_amd import kernels as K  # noqa: E402


def timed(fn, reps, settle=20):
    for _ in range(settle):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "target_top_p.json"))
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--batches", default="8,32,128")
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--scale", type=float, default=3.0, help="logits = scale * N(0,1) (3: a nucleus of a few hundred tokens "
                    "at T = 0.7, top-p 0.9)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    V, T, TOP_P, Kd = 152064, 0.7, 0.9, a.K
    inv_t = float(torch.tensor(1.0 / T, dtype=torch.float32))
    try:
        from transformers.generation.logits_process import TemperatureLogitsWarper, TopPLogitsWarper
        warpers = (TemperatureLogitsWarper(T), TopPLogitsWarper(TOP_P))
    except ImportError:
        warpers = None
    res = dict(workload=dict(V=V, K=Kd, dtype="bf16", T=T, top_p=TOP_P, logits=f"{a.scale} * N(0,1)", reps=a.reps,
                             note="us per call, CUDA events over back-to-back calls; inputs rotate over >= 512 MB of logits"),
               device=torch.cuda.get_device_name(0), host=platform.node(), batches={})
    for B in [int(x) for x in a.batches.split(",")]:
        g = torch.Generator(device=dev).manual_seed(B)
        row_bytes = B * Kd * V * 2
        nb = max(2, min(16, -(-(512 << 20) // row_bytes)))
        lgs = [(torch.randn((B, Kd, V), generator=g, device=dev) * a.scale).to(torch.bfloat16) for _ in range(nb)]
        tok = torch.randint(0, V, (B, Kd), generator=g, device=dev, dtype=torch.int32)
        tok[:, : Kd // 2] = lgs[0][:, : Kd // 2].float().argmax(-1).to(torch.int32)      # half the drafts inside the nucleus
        lp_d = torch.full((B, Kd), -1.0, device=dev)
        u = torch.rand((B, Kd), generator=g, device=dev)
        ws = K.VerifyWorkspace(B, Kd, V, torch.bfloat16, dev)
        i = [0]
        out_n = [None]
        out_p = [None]

        def nucleus():
            i[0] += 1
            out_n[0] = K.verify_accept_top_p(lgs[i[0] % nb], tok, lp_d, u, None, inv_temperature=inv_t, top_p=TOP_P, out=out_n[0])

        def plain():
            i[0] += 1
            out_p[0] = K.verify_accept(lgs[i[0] % nb], tok, lp_d, u, ws, out_p[0], inv_temperature=inv_t)

        def composition():
            i[0] += 1
            x = lgs[i[0] % nb].view(B * Kd, V).float()
            for w in warpers:
                x = w(None, x)
            lp = torch.log_softmax(x, dim=-1).gather(1, tok.view(-1, 1).long()).view(B, Kd)
            acc = torch.log(u) <= lp - lp_d
            return acc.to(torch.int32).cumprod(1).sum(1)

        rec = dict(nucleus_verify_us=timed(nucleus, a.reps), plain_verify_us=timed(plain, a.reps), buffers=nb)
        rec["composition_us"] = timed(composition, max(10, a.reps // 5)) if warpers else None
        # the same rows agree: n_acc of the nucleus verify against the composition's (one buffer, outside the timing)
        i[0] = -1
        nucleus()
        i[0] = -1
        want = composition() if warpers else None
        torch.cuda.synchronize()
        if want is not None:
            rec["n_acc_agree_with_composition"] = float((out_n[0].n_acc.long() == want.long()).float().mean().item())
        if rec["composition_us"]:
            rec["speedup_vs_composition"] = rec["composition_us"] / rec["nucleus_verify_us"]
        res["batches"][str(B)] = rec
        print(f"B={B:4d} K={Kd} ({B * Kd} rows): nucleus {rec['nucleus_verify_us']:8.1f} us   plain {rec['plain_verify_us']:7.1f} us   "
              f"torch composition {rec['composition_us'] or float('nan'):8.1f} us", flush=True)
        del lgs, ws
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
