#!/usr/bin/env python3
"""Timing of the three top-k entry points (asd_draft_sample_top_k, asd_verify_accept_top_k, asd_residual_sample_top_k) beside
the top-p entry points they extend and the torch composition they replace: HF's TemperatureLogitsWarper + TopKLogitsWarper +
TopPLogitsWarper on the GPU, then log_softmax / multinomial / gather (the sampling of generate(do_sample=True, temperature=0.7,
top_p=0.9) with transformers' default top_k = 50, generate_training_data.py:110-119).  All on the same rows; the inputs rotate
over enough buffers that the working set exceeds the 256 MB Infinity Cache, so every call reads its rows from HBM.

    python tools/bench_top_k.py [--out profiles/top_k.json] [--batches 8,32,128]
"""
import argparse
import json
import os
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "top_k.json"))
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--batches", default="8,32,128")
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--scale", type=float, default=3.0)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    V, T, TOP_K, TOP_P, Kd = 152064, 0.7, 50, 0.9, a.K
    inv_t = float(torch.tensor(1.0 / T, dtype=torch.float32))
    try:
        from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
        warpers = (TemperatureLogitsWarper(T), TopKLogitsWarper(TOP_K), TopPLogitsWarper(TOP_P))
    except ImportError:
        warpers = None

    def warp(x):
        for w in warpers:
            x = w(None, x)
        return x

    def inverse_cdf(p, u):
        """The draw of every row of p [n, V] at the uniforms u [n] (inverse CDF in vocabulary order, the kernels' own rule;
        torch.multinomial is not used: its device-side validity assert ends the whole queue on one bad row)."""
        c = p.cumsum(-1)
        return torch.searchsorted(c, (u * c[:, -1])[:, None]).clamp_(max=p.shape[-1] - 1)

    res = dict(workload=dict(V=V, K=Kd, dtype="bf16", T=T, top_k=TOP_K, top_p=TOP_P, logits=f"{a.scale} * N(0,1)", reps=a.reps,
                             note="us per call, CUDA events over back-to-back calls; inputs rotate over >= 512 MB of logits; "
                                  "draft / residual at B rows / sequences, verify at B * K rows"),
               device=torch.cuda.get_device_name(0), batches={})
    for B in [int(x) for x in a.batches.split(",")]:
        g = torch.Generator(device=dev).manual_seed(B)
        row_bytes = B * Kd * V * 2
        nb = max(2, min(16, -(-(512 << 20) // row_bytes)))
        lgs = [(torch.randn((B, Kd, V), generator=g, device=dev) * a.scale).to(torch.bfloat16) for _ in range(nb)]
        dls = [(x.float() + torch.randn(x.shape, generator=g, device=dev) * 0.5).to(torch.bfloat16) for x in lgs[:2]]
        r = torch.rand((B * Kd,), generator=g, device=dev)
        rb = r[:B].contiguous()
        i = [0]
        rec = dict(buffers=nb)
        # ---- the proposal draw: B rows
        ds = K.DraftSampler(B, V, torch.bfloat16, dev)
        rows = [x[:, 0] for x in lgs]

        def draft_k():
            i[0] += 1
            return ds.top_k(rows[i[0] % nb], rb, inv_t, top_k=TOP_K, top_p=TOP_P)

        def draft_p():
            i[0] += 1
            return ds(rows[i[0] % nb], rb, inv_t, TOP_P)

        def draft_torch():
            i[0] += 1
            lq = torch.log_softmax(warp(rows[i[0] % nb].float()), dim=-1)
            t = inverse_cdf(lq.exp(), rb)
            return t, lq.gather(1, t)

        rec["draft_top_k_us"] = timed(draft_k, a.reps)
        rec["draft_top_p_us"] = timed(draft_p, a.reps)
        # ---- the verify: B * K rows
        tok = torch.randint(0, V, (B, Kd), generator=g, device=dev, dtype=torch.int32)
        tok[:, : Kd // 2] = lgs[0][:, : Kd // 2].float().argmax(-1).to(torch.int32)      # half the drafts inside the kept set
        lp_d = torch.full((B, Kd), -1.0, device=dev)
        u = torch.rand((B, Kd), generator=g, device=dev)
        out_k, out_p = [None], [None]

        def verify_k():
            i[0] += 1
            out_k[0] = K.verify_accept_top_k(lgs[i[0] % nb], tok, lp_d, u, None, inv_temperature=inv_t, top_k=TOP_K, top_p=TOP_P,
                                             out=out_k[0])

        def verify_p():
            i[0] += 1
            out_p[0] = K.verify_accept_top_p(lgs[i[0] % nb], tok, lp_d, u, None, inv_temperature=inv_t, top_p=TOP_P, out=out_p[0])

        def verify_torch():
            i[0] += 1
            x = warp(lgs[i[0] % nb].view(B * Kd, V).float())
            lp = torch.log_softmax(x, dim=-1).gather(1, tok.view(-1, 1).long()).view(B, Kd)
            acc = torch.log(u) <= lp - lp_d
            return acc.to(torch.int32).cumprod(1).sum(1)

        rec["verify_top_k_us"] = timed(verify_k, a.reps)
        rec["verify_top_p_us"] = timed(verify_p, a.reps)
        # ---- the commit draw: B sequences (rejected rows and bonus rows mixed)
        rs = K.ResidualSampler(B, V, torch.bfloat16, dev)
        n_acc = torch.randint(0, Kd + 1, (B,), generator=g, device=dev, dtype=torch.int32)
        vk = K.verify_accept_top_k(lgs[0], tok, lp_d, u, None, inv_temperature=inv_t, top_k=TOP_K, top_p=TOP_P)
        vp = K.verify_accept_top_p(lgs[0], tok, lp_d, u, None, inv_temperature=inv_t, top_p=TOP_P)
        dthr_k = torch.stack([K.DraftSampler(B, V, torch.bfloat16, dev).top_k(dls[0][:, k].contiguous(), rb, inv_t, top_k=TOP_K,
                                                                               top_p=TOP_P).thr for k in range(Kd)], 1).contiguous()
        dthr_p = torch.stack([K.DraftSampler(B, V, torch.bfloat16, dev)(dls[0][:, k].contiguous(), rb, inv_t, TOP_P).thr
                              for k in range(Kd)], 1).contiguous()
        bonus = [x[:, Kd - 1].contiguous() for x in lgs]

        def resid_k():
            i[0] += 1
            j = i[0] % nb
            return rs.top_k(lgs[j], dls[j % 2], n_acc, rb, bonus[j], inv_t, top_k=TOP_K, top_p=TOP_P,
                            t_threshold=vk.t_nucleus_logit, d_threshold=dthr_k)

        def resid_p():
            i[0] += 1
            j = i[0] % nb
            return rs.top_p(lgs[j], dls[j % 2], n_acc, rb, bonus[j], inv_t, top_p=TOP_P, t_threshold=vp.t_nucleus_logit,
                            d_threshold=dthr_p)

        def resid_torch():
            i[0] += 1
            j = i[0] % nb
            sel = n_acc.clamp(max=Kd - 1).long()
            b = torch.arange(B, device=dev)
            pt = torch.softmax(warp(lgs[j][b, sel].float()), -1)
            pd = torch.softmax(warp(dls[j % 2][b, sel].float()), -1)
            res_w = (pt - pd).clamp_min(0)
            # an empty residual (both rows truncated to the same single token: p_t = p_d = 1) draws from p_t, the kernels' rule
            res_w = torch.where((res_w.sum(-1) > 0)[:, None], res_w, pt)
            w = torch.where((n_acc < Kd)[:, None], res_w, torch.softmax(warp(bonus[j].float()), -1))
            return inverse_cdf(w, rb), w

        rec["residual_top_k_us"] = timed(resid_k, a.reps)
        rec["residual_top_p_us"] = timed(resid_p, a.reps)
        # the inputs are intact after the kernels ran, and every probability row the composition draws from is valid
        rec["inputs_finite"] = bool(all(torch.isfinite(x).all().item() for x in lgs + dls))
        if warpers:
            i[0] = -1
            _, w = resid_torch()
            lq = torch.log_softmax(warp(rows[0].float()), dim=-1)
            rec["composition_probabilities_valid"] = bool(torch.isfinite(w).all().item() and (w >= 0).all().item()
                                                          and (w.sum(-1) > 0).all().item() and (~torch.isnan(lq)).all().item())
            n_t = max(10, a.reps // 5)
            rec["draft_composition_us"] = timed(draft_torch, n_t)
            rec["verify_composition_us"] = timed(verify_torch, n_t)
            rec["residual_composition_us"] = timed(resid_torch, n_t)
            for step in ("draft", "verify", "residual"):
                rec[f"{step}_speedup_vs_composition"] = rec[f"{step}_composition_us"] / rec[f"{step}_top_k_us"]
            # agreement on the same rows (one buffer, outside the timing): the kept sets of the draft rows and n_acc of the verify
            i[0] = -1
            d = draft_k()
            keep_hf = torch.isfinite(warp(rows[0].float()))
            x0 = rows[0].float()
            keep_me = x0 >= d.thr[:, None]
            rec["draft_kept_set_agree_with_composition"] = float((keep_hf == keep_me).all(1).float().mean().item())
            # HF's top-p sort drops some scores EQUAL to the threshold (bf16 rows tie there often); this build keeps every tie
            only_ties = ~(keep_hf & ~keep_me).any(1) & ((keep_hf | ~keep_me) | (x0 == d.thr[:, None])).all(1)
            rec["draft_kept_set_agree_up_to_threshold_ties"] = float(only_ties.float().mean().item())
            i[0] = -1
            verify_k()
            i[0] = -1
            want = verify_torch()
            torch.cuda.synchronize()
            rec["verify_n_acc_agree_with_composition"] = float((out_k[0].n_acc.long() == want.long()).float().mean().item())
        res["batches"][str(B)] = rec
        print(f"B={B:4d}: draft top-k {rec['draft_top_k_us']:7.1f} us (top-p {rec['draft_top_p_us']:6.1f})   "
              f"verify top-k {rec['verify_top_k_us']:7.1f} us (top-p {rec['verify_top_p_us']:6.1f})   "
              f"residual top-k {rec['residual_top_k_us']:7.1f} us (top-p {rec['residual_top_p_us']:6.1f})   "
              f"torch {rec.get('draft_composition_us', float('nan')):7.1f} / {rec.get('verify_composition_us', float('nan')):7.1f} / "
              f"{rec.get('residual_composition_us', float('nan')):7.1f} us", flush=True)
        del lgs, dls, ds, rs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
