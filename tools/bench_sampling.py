#!/usr/bin/env python3
"""Timing of the proposal / commit draws: asd_draft_sample (X1) and asd_residual_sample_ex, beside the torch idiom
they replace (log_softmax + multinomial + gather per drafted token, serving/speculative.py of round 1).

    python tools/bench_sampling.py [--out gpurun_out/sampling.json]
    python tools/bench_sampling.py --lp [--out FILE]     # the log-prob forms beside their parents
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from asd_amd import kernels as K  # noqa: E402


def timed(fn, reps=200, settle=50):
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


def interleaved(fns, reps, rounds=11):
    """A/B/A/B ... in one process: `rounds` timings of every candidate, taken in turn so that clock and cache drift hit all of
    them alike -> {name: {"median_us", "min_us", "max_us"}}; max - min over the rounds is the run-to-run noise."""
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, reps, settle=20))
    return {k: {"median_us": sorted(v)[len(v) // 2], "min_us": min(v), "max_us": max(v)} for k, v in times.items()}


def bench_lp(a, dev):
    """asd_residual_sample_lp beside asd_residual_sample_ex (B = 32: group form, B = 128: one workgroup per sequence; V = 152064,
    bf16) and asd_commit_step_lp / asd_commit_step_stop / asd_commit_step_finish beside asd_commit_step (B = 32, K = 8)."""
    V, Kd = 152064, 8
    res = {}
    for B in (() if a.commit_only else (32, 128)):
        g = torch.Generator(device=dev).manual_seed(B)
        rows = [(torch.randn((B, V), generator=g, device=dev) * a.scale).to(torch.bfloat16) for _ in range(4)]
        t3 = torch.stack([rows[j % 4] for j in range(Kd)], 1).contiguous()
        d3 = torch.stack([rows[(j + 1) % 4] for j in range(Kd)], 1).contiguous()
        n_acc = torch.randint(0, Kd + 1, (B,), generator=g, device=dev, dtype=torch.int32)
        r = torch.rand((B,), generator=g, device=dev)
        rs = K.ResidualSampler(B, V, torch.bfloat16, dev)
        tok_out = torch.empty((B,), dtype=torch.int32, device=dev)
        lp_out = torch.empty((B,), dtype=torch.float32, device=dev)
        res[f"residual_B{B}"] = interleaved({
            "asd_residual_sample_ex": lambda: rs(t3, d3, n_acc, r, rows[0], 1 / 0.7, out=tok_out),
            "asd_residual_sample_lp": lambda: rs.lp(t3, d3, n_acc, r, rows[0], 1 / 0.7, out=tok_out, lp_out=lp_out),
        }, a.reps)
        print(B, res[f"residual_B{B}"], flush=True)
    B = 32
    g = torch.Generator(device=dev).manual_seed(7)
    tok = torch.randint(0, V, (B, Kd), generator=g, device=dev, dtype=torch.int32)
    lp_tok = -torch.rand((B, Kd), generator=g, device=dev)
    n_acc = torch.randint(0, Kd + 1, (B,), generator=g, device=dev, dtype=torch.int32)
    drawn = torch.randint(0, V, (B,), generator=g, device=dev, dtype=torch.int32)
    lp_drawn = -torch.rand((B,), generator=g, device=dev)
    seq_len = torch.zeros((B,), dtype=torch.int32, device=dev)
    out_tok = torch.zeros((B, 4096), dtype=torch.int32, device=dev)
    out_lp = torch.zeros((B, 4096), dtype=torch.float32, device=dev)
    nc = torch.zeros((B,), dtype=torch.int32, device=dev)

    def commit():
        seq_len.zero_()                             # (the length-reset fill of tools/bench_aux.py: both candidates pay it)
        K.commit_step(tok, n_acc, drawn, seq_len, out_tok, nc)

    def commit_lp():
        seq_len.zero_()
        K.commit_step_lp(tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, out_tok, out_lp, nc)

    # asd_commit_step_stop on the same inputs with a two-id stop set that no input token hits: no row ever finishes (the length
    # is reset every call, the rows are 4096 wide), so every call does the whole commit, like the two beside it
    present = set(tok.flatten().tolist()) | set(drawn.tolist())
    stop_ids = torch.tensor([i for i in range(V - 1, 0, -1) if i not in present][:2], dtype=torch.int32, device=dev)
    finished = torch.zeros((B,), dtype=torch.int32, device=dev)
    n_finished = torch.zeros((1,), dtype=torch.int32, device=dev)

    def commit_stop():
        seq_len.zero_()
        K.commit_step_stop(tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, out_tok, out_lp, finished, stop_ids=stop_ids,
                           n_finished=n_finished, n_commit=nc)

    # asd_commit_step_finish on the same inputs with 8 two-token sequences, owned by every row, that no input hits (their tokens
    # are absent from the inputs); its own flag and counter, so that neither kernel sees a row the other finished
    absent = [i for i in range(V - 3, 0, -1) if i not in present][:16]
    seq_tok, seq_n, _ = K.pack_stop_sequences([absent[2 * i:2 * i + 2] for i in range(8)], dev, shared=True)
    finished2 = torch.zeros((B,), dtype=torch.int32, device=dev)
    n_finished2 = torch.zeros((1,), dtype=torch.int32, device=dev)
    matched = torch.full((B,), -1, dtype=torch.int32, device=dev)

    def commit_finish():
        seq_len.zero_()
        K.commit_step_finish(tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, out_tok, out_lp, finished2, 0, seq_tok=seq_tok,
                             seq_n=seq_n, n_finished=n_finished2, matched=matched, n_commit=nc)

    res["commit_B32_K8"] = interleaved({"asd_commit_step": commit, "asd_commit_step_lp": commit_lp,
                                        "asd_commit_step_stop": commit_stop, "asd_commit_step_finish": commit_finish}, a.reps)
    if int(n_finished.item()) != 0 or int(n_finished2.item()) != 0:
        raise RuntimeError("a row finished during the timing: the candidates did not do the same work")
    print("commit", res["commit_B32_K8"], flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "gpurun_out", "sampling.json"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batches", default="8,32,128")
    ap.add_argument("--scale", type=float, default=3.0, help="logits = scale * N(0,1): 3 = a wide nucleus (hundreds of tokens at "
                    "T = 0.7, top-p 0.9), 8 = a peaked row (a handful of tokens), closer to a confident LLM step")
    ap.add_argument("--lp", action="store_true", help="time asd_residual_sample_lp / asd_commit_step_lp / asd_commit_step_stop / asd_commit_step_finish beside their parents, interleaved")
    ap.add_argument("--commit-only", action="store_true", help="with --lp: the commit kernels only")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.lp:
        res = bench_lp(a, dev)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        return
    V = 152064
    res = {}
    for B in [int(x) for x in a.batches.split(",")]:
        g = torch.Generator(device=dev).manual_seed(B)
        nb = 8
        rows = [(torch.randn((B, V), generator=g, device=dev) * a.scale).to(torch.bfloat16) for _ in range(nb)]
        r = torch.rand((B,), generator=g, device=dev)
        ds = K.DraftSampler(B, V, torch.bfloat16, dev)
        out = None
        i = [0]

        def draft(top_p):
            nonlocal out
            i[0] += 1
            out = ds(rows[i[0] % nb], r, 1 / 0.7, top_p, out)

        def torch_idiom():
            i[0] += 1
            lp = torch.log_softmax(rows[i[0] % nb].float() / 0.7, dim=-1)
            tok = torch.multinomial(lp.exp(), 1)[:, 0]
            return lp.gather(1, tok[:, None])

        Kd = 8
        t3 = torch.stack([rows[j % nb] for j in range(Kd)], 1).contiguous()
        d3 = torch.stack([rows[(j + 3) % nb] for j in range(Kd)], 1).contiguous()
        n_acc = torch.randint(0, Kd + 1, (B,), generator=g, device=dev, dtype=torch.int32)
        rs = K.ResidualSampler(B, V, torch.bfloat16, dev)
        thr = torch.full((B, Kd), 2.0, device=dev)
        tok_out = torch.empty((B,), dtype=torch.int32, device=dev)
        res[f"B{B}"] = {
            "asd_draft_sample_top_p_0.9_us": timed(lambda: draft(0.9), a.reps),
            "asd_draft_sample_no_top_p_us": timed(lambda: draft(1.0), a.reps),
            "torch_log_softmax_multinomial_gather_us": timed(torch_idiom, a.reps),
            "asd_residual_sample_us": timed(lambda: rs(t3, d3, n_acc, r, rows[0], 1 / 0.7, out=tok_out), a.reps),
            "asd_residual_sample_ex_truncated_draft_us": timed(lambda: rs(t3, d3, n_acc, r, rows[0], 1 / 0.7, out=tok_out, d_threshold=thr), a.reps),
            "row_bytes": V * 2, "rows": B,
        }
        print(B, res[f"B{B}"], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
