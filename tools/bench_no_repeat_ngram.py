#!/usr/bin/env python3
"""Time the no-repeat-n-gram kernel (asd_no_repeat_ngram_rows) at the verify loop's shape, B = 32, K = 8, V = 152064, bf16, n = 3,
at history lengths (prompt plus generated tokens) of 128, 2048 and 16384, next to the multi-token bad-words kernel
(asd_bad_words_rows, unchanged since it was added) with 16 words per row, in the same process and on the same tensors:

  ngram_L              one call on the target's [B, K+1, V] output, n_prev = 0, every row with a history of L tokens (24 of them
                       the prompt) whose ids follow a Zipf law, so that the last bigram of a row has earlier occurrences as the
                       last bigram of running text has
  ngram_L_draft        one call on one proposal's [B, V] draft logits, n_prev = K / 2 (a verifying step makes K of these)
  bad_words_L[_draft]  asd_bad_words_rows with 16 words per row (a quarter each: one token, a bigram and a trigram that match,
                       an 8-token word that does not) on the same tensors: the yardstick -- one workgroup per (b, j), at most
                       seven history loads per lane, whatever the history's length
  ngram_L_one_slice[_draft]   at the longest history only: the same kernel built once more with ASD_NGRAM_SLICE = 2^30, so that
                       ONE workgroup per (b, j) walks the whole history (n_slices = 1) -- what the slices are there to avoid

    python tools/bench_no_repeat_ngram.py [--out profiles/no_repeat_ngram_step.json] [--rounds 15] [--calls 20] [--no-trace]
                                          [--one-slice-lib PATH]

Two figures per variant.  `kernel_us`: the kernels' own time, from a `rocprofv3 --kernel-trace` run OF ITS OWN (no counters, no
other tracing): this script starts itself once more under the profiler as a fresh child process (`--worker`) before it touches
the GPU, the child runs every variant `--calls` times, and the dispatches are attributed by position: a one-row f32 launch of
the n-gram kernel (another template instance, so another kernel name) is the separator between variants.  `us_median`: the
per-call time from Python with the profiler off -- one device-event pair around `--calls` back-to-back calls, the variants in
alternation, `--rounds` rounds after a warm-up round.  Both operations only store -inf, so a repeated call stores the same bits
again and nothing has to be restored.  `ratio_to_bad_words` is the quotient of kernel_us (of us_median where the trace is
missing).  The one-slice library is compiled from csrc/no_repeat_ngram.hip alone into a temporary directory (or taken from
`--one-slice-lib` when that file exists) before the GPU is touched.  Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_token_mask import parse_trace  # noqa: E402  (the kernel-trace reader: dispatches cut at a separator kernel)

SEPARATOR = ("k_no_repeat_ngram_rows<0>", "k_no_repeat_ngram_rowsILi0E")   # the f32 instance, demangled or not: the timed launches are bf16 (<1>)
ONE_SLICE = 1 << 30
PROMPT = 24


def build_one_slice_lib(path: str) -> str:
    """csrc/no_repeat_ngram.hip alone, with ASD_NGRAM_SLICE = 2^30: a library whose launcher always forms one slice."""
    from asd_amd import build as Bd
    if os.path.exists(path):
        return path
    cmd = [Bd._hipcc(), *Bd.COMMON, f"-DASD_NGRAM_SLICE={ONE_SLICE}", "-shared", os.path.join(Bd.CSRC, "no_repeat_ngram.hip"), "-o", path]
    subprocess.run(cmd, check=True)
    return path


def build_variants(a):
    """-> (variants: name -> callable, separator: callable, info).  Everything the timed calls touch is made here."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_no_repeat_ngram.py needs a GPU (no fallback)")
    from asd_amd import _binding
    from asd_amd import kernels as K

    B, Kd, V, n = a.batch, a.draft_len, a.vocab, a.n
    g = torch.Generator(device="cuda").manual_seed(1)
    y = (torch.randn((B, Kd + 1, V), generator=g, device="cuda") * 4.0).to(torch.bfloat16)
    yd = y[:, 0].clone()
    rng = np.random.default_rng(1)
    step_h = (rng.zipf(1.2, (B, Kd)) % V).astype(np.int32)
    step_tok = torch.from_numpy(step_h).cuda()
    one = ctypes.CDLL(a.one_slice_lib)
    one.asd_no_repeat_ngram_rows.restype, one.asd_no_repeat_ngram_rows.argtypes = _binding.SIGNATURES["asd_no_repeat_ngram_rows"]
    variants, slices, banned = {}, {}, {}
    for L in a.lengths:
        cap = L + 64
        tokens_h = (rng.zipf(1.2, (B, cap)) % V).astype(np.int32)
        seq_h = np.full((B,), L, dtype=np.int32)
        tokens, seq_len = torch.from_numpy(tokens_h).cuda(), torch.from_numpy(seq_h).cuda()
        ngram = K.pack_no_repeat_ngram([n] * B, [PROMPT] * B, PROMPT, "cuda")
        rows = []
        for b in range(B):
            last = [int(t) for t in rng.choice(V, 16, replace=False)]
            end, prop = int(tokens_h[b, L - 1]), int(step_h[b, 0])
            rows.append([((t,), (end, t), (end, prop, t), tuple(int(v) for v in rng.integers(0, V, 7)) + (t,))[i % 4]
                         for i, t in enumerate(last)])
        words = K.pack_bad_words(rows, "cuda")
        variants[f"ngram_{L}"] = lambda p=ngram, t=tokens, s=seq_len, c=cap: K.no_repeat_ngram_rows(y, p, t, s, c, step_tok, 0)
        variants[f"ngram_{L}_draft"] = lambda p=ngram, t=tokens, s=seq_len, c=cap: K.no_repeat_ngram_rows(yd, p, t, s, c, step_tok, Kd // 2)
        variants[f"bad_words_{L}"] = lambda w=words, t=tokens, s=seq_len, c=cap: K.bad_words_rows(y, w, t, s, PROMPT, c, step_tok, 0)
        variants[f"bad_words_{L}_draft"] = lambda w=words, t=tokens, s=seq_len, c=cap: K.bad_words_rows(yd, w, t, s, PROMPT, c, step_tok, Kd // 2)
        slices[L] = -(-(cap + Kd) // _binding.NGRAM_SLICE)
        # how much the rule bans at this length: distinct ids per row at position 0, from the host copy
        per_row = []
        for b in range(B):
            H = tokens_h[b, :L]
            hit = np.ones(L - n + 1, dtype=bool)
            for k in range(n - 1):
                hit &= H[k:L - n + 1 + k] == H[L - (n - 1) + k]
            per_row.append(len(set(H[n - 1:][hit].tolist())))
        banned[L] = round(float(np.mean(per_row)), 2)
        if L == max(a.lengths):
            def one_slice(x, K1, n_prev, p=ngram, t=tokens, s=seq_len, c=cap):
                rc = one.asd_no_repeat_ngram_rows(x.data_ptr(), K._DTYPE_CODE[x.dtype], x.stride(0), V, B, K1, V, None, n, p.row_start.data_ptr(),
                                                  t.data_ptr(), t.shape[1], s.data_ptr(), PROMPT, c, step_tok.data_ptr(), Kd, Kd,
                                                  n_prev, K._stream())
                assert rc == 0, rc
            variants[f"ngram_{L}_one_slice"] = lambda f=one_slice: f(y, Kd + 1, 0)
            variants[f"ngram_{L}_one_slice_draft"] = lambda f=one_slice: f(yd, 1, Kd // 2)
    tiny = torch.zeros((1, 1, 32), dtype=torch.float32, device="cuda")
    tiny_n = K.pack_no_repeat_ngram([1], [0], 0, "cuda")
    tiny_tokens, tiny_len = torch.zeros((1, 4), dtype=torch.int32, device="cuda"), torch.ones((1,), dtype=torch.int32, device="cuda")
    info = {"B": B, "K": Kd, "V": V, "n": n, "dtype": "bf16", "device": torch.cuda.get_device_name(0), "cus": K.device_cu_count(0),
            "prompt": PROMPT, "slice": _binding.NGRAM_SLICE, "n_slices": {str(k): v for k, v in slices.items()},
            "distinct_bans_per_row_at_position_0": {str(k): v for k, v in banned.items()}}
    return variants, (lambda: K.no_repeat_ngram_rows(tiny, tiny_n, tiny_tokens, tiny_len, 4)), info


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "no_repeat_ngram_step.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--draft-len", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--n", type=int, default=3, help="no_repeat_ngram_size of every row")
    ap.add_argument("--lengths", type=int, nargs="*", default=[128, 2048, 16384], help="history lengths (prompt plus generated)")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run (kernel_us is then missing)")
    ap.add_argument("--trace-dir", default=None, help="keep the profiler's output here (default: a temporary directory)")
    ap.add_argument("--one-slice-lib", default=None, help="the one-slice build of the kernel (built into a temporary directory when missing)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    a.one_slice_lib = build_one_slice_lib(os.path.abspath(a.one_slice_lib) if a.one_slice_lib else
                                          os.path.join(tempfile.mkdtemp(prefix="ngram_one_slice_"), "libngram_one_slice.so"))

    # 1. the kernel trace, in a fresh child process and before this one opens the GPU
    trace, trace_error = None, None
    if not a.no_trace:
        keep = a.trace_dir is not None
        directory = os.path.abspath(a.trace_dir) if keep else tempfile.mkdtemp(prefix="ngram_trace_")
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", directory, "--", sys.executable, os.path.abspath(__file__),
               "--worker", "--batch", str(a.batch), "--draft-len", str(a.draft_len), "--vocab", str(a.vocab), "--calls", str(a.calls),
               "--n", str(a.n), "--one-slice-lib", a.one_slice_lib, "--lengths", *map(str, a.lengths)]
        try:
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        except (OSError, subprocess.SubprocessError) as e:
            trace_error = f"{type(e).__name__}: {e}"
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
    res = {"what": "asd_no_repeat_ngram_rows at three history lengths next to asd_bad_words_rows with 16 words per row, on the same "
                   "tensors, one call each; at the longest history also the kernel built with one slice per (b, j)",
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
    for L in a.lengths:
        for tail in ("", "_draft"):
            for own in (f"ngram_{L}{tail}", f"ngram_{L}_one_slice{tail}"):
                if own in res:
                    res[own]["ratio_to_bad_words"] = round(res[own][key] / res[f"bad_words_{L}{tail}"][key], 4)
    res["ratios_from"] = key
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
