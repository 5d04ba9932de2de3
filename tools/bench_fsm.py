#!/usr/bin/env python3
"""Time the guided-decoding kernels at the verify loop's shape, B = 32, K = 8, V = 152064, bf16, next to the allow-list kernel
whose write stream asd_fsm_mask_rows shares, in the same process and on the same tensors:

  fsm_mask            one asd_fsm_mask_rows call on the target's [B, K+1, V] output: a 16-choice trie, row b at the nodes of choice
                      b % 16 (column 0 the root, which allows 16 tokens; every other column a node that allows one)
  fsm_mask_draft      one call on one proposal's [B, V] draft logits (a verifying step makes K of these), at a node of depth 4
  logit_mask[_draft]  asd_logit_mask_rows on the same tensors, every row on its own allow-list of as many ids as the states of
                      the call above allow on average (R = B masks): the yardstick -- the stream is the same code
  fsm_advance_1 / _V  one asd_fsm_advance call at B = 32, every row in a state of 1 edge / of V edges (a hit, found in the search's
                      third round at V = 152064)
  fsm_commit_1 / _V   one asd_fsm_commit call, likewise

    python tools/bench_fsm.py [--out profiles/fsm_step.json] [--rounds 15] [--calls 40] [--no-trace]

Two figures per variant, taken as tools/bench_token_mask.py takes them.  `kernel_us`: the kernel's own time, from a
`rocprofv3 --kernel-trace` run OF ITS OWN (no counters, no other tracing) in a fresh child process (`--worker`) started before this
one touches the GPU; dispatches are attributed by position, a one-word f32 launch of the mask kernel being the separator.
`us_median`: the per-call time from Python with the profiler off -- one device-event pair around `--calls` back-to-back calls, the
variants in alternation, `--rounds` rounds after a warm-up round; min .. max is the run-to-run spread.  The profile states the
ratio fsm_mask / logit_mask and whether the gap lies inside that spread.  If the traced worker fails, faults or runs into its
time limit, the tool stops there and starts nothing more on the card; only a missing profiler (and --no-trace) lets it go on
without a trace.  Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_token_mask import parse_trace  # noqa: E402  (the kernel-trace reader: dispatches cut at a separator kernel)

SEPARATOR = ("k_fsm_mask_rows<0>", "k_fsm_mask_rowsILi0E")     # the f32 instance, demangled or not: the timed launches are bf16 (<1>)
STOP = 2


def build_variants(a):
    """-> (variants: name -> callable, separator: callable, info).  Everything the timed calls touch is made here."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_fsm.py needs a GPU (no fallback)")
    from asd_amd import kernels as K
    from asd_amd.serving.guided import TokenFSM, compile_rows

    B, Kd, V = a.batch, a.draft_len, a.vocab
    g = torch.Generator(device="cuda").manual_seed(1)
    x = (torch.randn((B, Kd + 1, V), generator=g, device="cuda") * 4.0).to(torch.bfloat16)
    y, yd = x.clone(), x[:, 0].clone()                       # what every variant writes to
    rng = np.random.default_rng(1)
    ids = rng.choice(np.arange(3, V), (a.choices, Kd + 1), replace=False)           # distinct ids: distinct first tokens
    choices = [tuple(int(t) for t in row) for row in ids]
    trie = TokenFSM.from_choices(choices)
    comp = compile_rows([trie] * B, [[STOP]] * B, V)
    fsm = K.pack_fsm(comp, Kd + 1, "cuda")
    pos = np.zeros((B, Kd + 1), dtype=np.int32)
    for b in range(B):                                       # column j: the node behind the first j tokens of choice b % 16
        s = comp.starts[b]
        for j in range(Kd + 1):
            pos[b, j] = s
            s = comp.step(s, choices[b % a.choices][j])
    fsm.pos_state.copy_(torch.from_numpy(pos))
    allowed = np.array([[int(comp.allowed(int(s)).sum()) for s in row] for row in pos])
    depth = min(4, Kd)
    n_target, n_draft = max(1, round(float(allowed.mean()))), max(1, round(float(allowed[:, depth].mean())))
    lists = {n: K.pack_token_masks([tuple(sorted(int(t) for t in rng.choice(V, n, replace=False))) for _ in range(B)], V, "cuda")
             for n in {n_target, n_draft}}
    # the same answer before any timing: what stays finite is what the states allow
    K.fsm_mask_rows(y, fsm, 0)
    K.fsm_mask_rows(yd, fsm, depth)
    torch.cuda.synchronize()
    assert int((~torch.isneginf(y)).sum()) == int(allowed.sum()) and int((~torch.isneginf(yd)).sum()) == int(allowed[:, depth].sum())
    y.copy_(x)
    yd.copy_(x[:, 0])

    # the two small kernels: a state of one edge (0) and a state of V edges (1), every row in the same one; the token hits, and
    # at V = 152064 in the THIRD round of the cooperative search (probes 2376 apart, then 38 apart, then adjacent)
    hit = V // 2 + 198 if V > 400 else V // 2
    wide = SimpleNamespace(state_first=np.array([0, 1, 1 + V], dtype=np.int32), edge_tok=np.concatenate([[hit], np.arange(V)]).astype(np.int32),
                           edge_next=np.concatenate([[0], np.ones(V)]).astype(np.int32), state_other=np.array([-1, -1], dtype=np.int32),
                           starts=[0] * B, V=V)
    small = {n: K.pack_fsm(SimpleNamespace(**{**vars(wide), "starts": [s] * B}), Kd + 1, "cuda") for n, s in (("1", 0), ("V", 1))}
    step_tok = torch.full((B, Kd), hit, dtype=torch.int32, device="cuda")
    cap = 64
    tokens = torch.full((B, cap), hit, dtype=torch.int32, device="cuda")
    seq_len = torch.full((B,), 40, dtype=torch.int32, device="cuda")
    n_commit = torch.full((B,), Kd // 2 + 1, dtype=torch.int32, device="cuda")

    variants = {"fsm_mask": lambda: K.fsm_mask_rows(y, fsm, 0), "logit_mask": lambda p=lists[n_target]: K.logit_mask_rows(y, p),
                "fsm_mask_draft": lambda: K.fsm_mask_rows(yd, fsm, depth), "logit_mask_draft": lambda p=lists[n_draft]: K.logit_mask_rows(yd, p)}
    for n, f in small.items():
        variants[f"fsm_advance_{n}"] = lambda f=f: K.fsm_advance(f, step_tok, depth - 1)
        variants[f"fsm_commit_{n}"] = lambda f=f: K.fsm_commit(f, tokens, seq_len, n_commit, cap)
    tiny = torch.zeros((1, 1, 32), dtype=torch.float32, device="cuda")
    i32 = lambda v: np.array(v, dtype=np.int32)                                    # noqa: E731
    tiny_fsm = K.pack_fsm(SimpleNamespace(state_first=i32([0, 1]), edge_tok=i32([0]), edge_next=i32([0]), state_other=i32([-1]),
                                          starts=[0], V=32), 1, "cuda")
    info = {"B": B, "K": Kd, "V": V, "dtype": "bf16", "device": torch.cuda.get_device_name(0), "cus": K.device_cu_count(0),
            "choices": a.choices, "states": fsm.S, "edges": fsm.E, "allowed_per_position_mean": round(float(allowed.mean()), 2),
            "allow_list_ids": {"target": n_target, "draft": n_draft}, "bytes": {"target": B * (Kd + 1) * V * 2, "draft": B * V * 2}}
    return variants, (lambda: K.fsm_mask_rows(tiny, tiny_fsm, 0)), info


def worker(a) -> int:
    """Under the profiler: a warm-up call of everything, then per variant one separator launch and `--calls` calls."""
    import torch
    variants, separator, _ = build_variants(a)
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    for fn in variants.values():
        separator()
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
    separator()
    torch.cuda.synchronize()
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fsm_step.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--draft-len", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--choices", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run (kernel_us is then missing)")
    ap.add_argument("--trace-dir", default=None, help="keep the profiler's output here (default: a temporary directory)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)

    # 1. the kernel trace, in a fresh child process and before this one opens the GPU
    trace, trace_error = None, None
    if not a.no_trace:
        directory = os.path.abspath(a.trace_dir) if a.trace_dir is not None else tempfile.mkdtemp(prefix="fsm_trace_")
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", directory, "--", sys.executable, os.path.abspath(__file__),
               "--worker", "--batch", str(a.batch), "--draft-len", str(a.draft_len), "--vocab", str(a.vocab), "--calls", str(a.calls),
               "--choices", str(a.choices)]
        try:
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        except OSError as e:                                 # the profiler is not installed: go on without a trace
            trace_error = f"{type(e).__name__}: {e}"
        except subprocess.SubprocessError as e:              # the worker failed, faulted or hung: nothing more starts on the card
            raise SystemExit(f"bench_fsm.py: the traced worker did not finish ({type(e).__name__}: {e}); no variant was timed")
    # 2. the per-call figures from Python, profiler off
    import torch
    variants, _, info = build_variants(a)
    if not a.no_trace and trace_error is None:
        try:
            trace = parse_trace(directory, list(variants), a.calls, SEPARATOR)
        except (RuntimeError, KeyError, ValueError) as e:
            trace_error = f"{type(e).__name__}: {e}"
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
    res = {"what": "asd_fsm_mask_rows next to asd_logit_mask_rows (the same write stream) on the same tensors, and asd_fsm_advance / "
                   "asd_fsm_commit at states of 1 and of V edges, one call each",
           **info, "rounds": a.rounds, "calls_per_round": a.calls}
    if trace_error is not None:
        res["trace_error"] = trace_error
    for name, t in times.items():
        res[name] = {"us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2)}
        if trace is not None:
            k = trace[name]
            res[name].update(kernel_us=round(statistics.median(k["us"]), 2), kernel_us_min=round(min(k["us"]), 2),
                             kernel_us_max=round(max(k["us"]), 2), kernels_per_call=k["kernels_per_call"], kernel=k["kernel"])
    key = "kernel_us" if trace is not None else "us_median"
    notes = []
    for tail in ("", "_draft"):
        own, ref = res[f"fsm_mask{tail}"], res[f"logit_mask{tail}"]
        own["ratio_to_logit_mask"] = round(own[key] / ref[key], 3)
        own["write_gb_per_s"] = round(info["bytes"]["draft" if tail else "target"] / own[key] / 1e3, 1)
        lo, hi = ("kernel_us_min", "kernel_us_max") if trace is not None else ("us_min", "us_max")
        spread = max((r[hi] - r[lo]) / r[key] for r in (own, ref))               # run-to-run, relative, the wider of the two
        own["spread_rel"] = round(spread, 3)
        own["gap_inside_spread"] = bool(abs(own["ratio_to_logit_mask"] - 1.0) <= spread)
        notes.append(f"fsm_mask{tail} / logit_mask{tail} = {own['ratio_to_logit_mask']} ({key}); run-to-run spread {own['spread_rel']}: "
                     f"the gap lies {'inside' if own['gap_inside_spread'] else 'OUTSIDE'} it")
    res["ratios_from"] = key
    res["notes"] = notes
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
