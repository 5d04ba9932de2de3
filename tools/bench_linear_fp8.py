"""X3, weight-only FP8: asd_linear_fp8 beside asd_linear on the bf16 original, on the decoder-layer projections of the Qwen2.5
shapes at the memory-bound row counts (M <= 64).  The two alternate within one run; weights rotate over enough copies to
exceed the 256 MB MALL, so the figures are HBM figures.  --pass-model 7b adds one B = 32, T = 1 pass through HipDecoder, bf16
against fp8, timed with device events.
    python tools/bench_linear_fp8.py [--out profiles/linear_fp8.json] [--models 7b,32b,72b] [--rows 1,8,32,64] [--repeats 3]"""
import argparse
import json
import sys
from importlib import import_module
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
K_ = import_module("adaptive-speculative-decoding_amd.kernels")
SL = import_module("adaptive-speculative-decoding_amd.serving.synthetic_lm")


def time_us(fn, n_rot, replays=8):
    """n_rot calls (one per rotating weight copy) captured in ONE hipGraph, replayed: no per-call host overhead in the figure."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(n_rot):
            fn(i)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(n_rot):
            fn(i)
    graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (replays * n_rot)


def pass_us(name, weights, repeats):
    """One B = 32, T = 1 pass of the model's decoder stack (hidden states out: the lm_head stays bf16 either way)."""
    lm = SL.SyntheticLM(SL.QWEN25_SHAPES[name], dtype=torch.bfloat16, device="cuda", seed=1)
    lm.enable_hip_layers(weights=weights)
    lm.alloc_ragged(32, 64)
    ids = torch.randint(0, 1000, (32, 1), device="cuda")
    pos = torch.full((32,), 8, dtype=torch.int64, device="cuda")
    times = []
    for _ in range(repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        lm.forward_ragged(ids, pos, 9, return_hidden=True)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    del lm
    torch.cuda.empty_cache()
    return [round(t, 1) for t in times[1:]]         # the first pass is the warm-up


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--models", default="7b,32b,72b")
    ap.add_argument("--rows", default="1,8,32,64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pass-model", default=None)
    a = ap.parse_args()
    lib = K_._lib()
    ws = K_.LinearWorkspace("cuda")
    res = []
    for name in [m for m in a.models.split(",") if m]:
        s = SL.QWEN25_SHAPES[name]
        kv = s.kv_heads * s.head_dim
        mats = {"qkv": (s.hidden + 2 * kv, s.hidden), "o": (s.hidden, s.hidden), "gate_up": (2 * s.intermediate, s.hidden),
                "down": (s.hidden, s.intermediate)}
        for mname, (N, D) in mats.items():
            n_rot = max(2, min(8, (600 << 20) // (N * D) + 1))          # the FP8 copies alone exceed the MALL
            W = [torch.randn(N, D, device="cuda", dtype=torch.bfloat16) * D ** -0.5 for _ in range(n_rot)]
            Q = [K_.quantize_fp8(w) for w in W]
            for M in [int(v) for v in a.rows.split(",")]:
                x = torch.randn(M, D, device="cuda", dtype=torch.bfloat16)
                out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
                t8, t16 = [], []
                for _ in range(a.repeats):                               # alternate: both see the same machine state
                    t8.append(time_us(lambda i: K_.linear_fp8(x, Q[i], N, workspace=ws, out=out), n_rot))
                    t16.append(time_us(lambda i: K_.linear(x, W[i], workspace=ws, out=out), n_rot))
                m8, m16 = sorted(t8)[len(t8) // 2], sorted(t16)[len(t16) // 2]
                r = {"model": name, "matrix": mname, "M": M, "N": N, "D": D,
                     "fp8_slices": max(1, (int(lib.asd_linear_fp8_workspace_bytes(M, N, D)) - 256) // (4 * M * N)),
                     "bf16_slices": int(lib.asd_linear_slices(M, N, D)),
                     "fp8_us": round(m8, 2), "bf16_us": round(m16, 2), "fp8_us_all": [round(t, 2) for t in t8],
                     "bf16_us_all": [round(t, 2) for t in t16], "fp8_TBps": round(N * D / m8 / 1e6, 3),
                     "bf16_TBps": round(N * D * 2 / m16 / 1e6, 3), "fp8_over_bf16": round(m8 / m16, 3)}
                res.append(r)
                print(r, flush=True)
            del W, Q
            torch.cuda.empty_cache()
    if a.pass_model:
        r = {"pass": a.pass_model, "B": 32, "T": 1, "bf16_us": pass_us(a.pass_model, "bf16", a.repeats),
             "fp8_us": pass_us(a.pass_model, "fp8", a.repeats)}
        res.append(r)
        print(r, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
