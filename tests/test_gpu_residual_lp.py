"""asd_residual_sample_lp: the commit draw that also reports log p_t^N(token).

The TOKEN must be the existing entry point's on the same inputs and workspace, bit for bit (that is the parent's behaviour, not
the new code's); lp is checked against the f64 log-probability of the token the kernel returned, over the target row the draw
used, restricted to that row's threshold and renormalised.  The bound, 2e-5, is the project's own for lp_t (DESIGN §0 item 5,
tests/test_gpu_full_size_loop.py).  Thresholds come from the project's own verify and draft calls.

V = 5000, K = 4: 625 (bf16 / f16) or 1250 (f32) 16-byte vectors -- 9 full 64-vector tiles and a ragged one; B = 3 and 33 take the
group form (many / an odd count of workgroups per sequence); B = 100 is the issue's case for the one-workgroup-per-sequence form,
but at these row lengths the launcher still picks the group form with G = 1 for it (its range is B <= 128), so B = 130 is added
to reach k_residual_row; the three-launch form is forced through asd_debug_residual_groups(-1)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import encode_logits, to_device_logits
from tests.stage_scenario import ref_logprob

pytestmark = pytest.mark.gpu

LP_ATOL = 2e-5
INV_T = float(np.float32(1 / 0.7))
TRUNCATIONS = ("none", "d_threshold", "target_top_p", "target_top_k_top_p")


def _case(B, K, V, dtype, seed):
    """The logit scale of tests/test_gpu_residual.py; n_acc covers 0, an inner position and K (the bonus row)."""
    rng = np.random.default_rng(seed)
    xt = (rng.standard_normal((B * K, V)) * 3).astype(np.float32)
    xd = (xt + rng.standard_normal((B * K, V))).astype(np.float32)
    bonus = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    n_acc = rng.integers(0, K + 1, B).astype(np.int32)
    n_acc[:3] = (0, K // 2, K)
    r = rng.uniform(0, 1, B).astype(np.float32)
    return encode_logits(xt, dtype), encode_logits(xd, dtype), encode_logits(bonus, dtype), n_acc, r, rng


def _run(Kn, B, K, V, dtype, trunc, seed, groups=0):
    import torch
    st, sd, sb, n_acc, r, rng = _case(B, K, V, dtype, seed)
    t = to_device_logits(st, dtype).view(B, K, V)
    d = to_device_logits(sd, dtype).view(B, K, V)
    bo = to_device_logits(sb, dtype).view(B, V)
    na, rr = torch.from_numpy(n_acc).cuda(), torch.from_numpy(r).cuda()
    top_k = 50 if trunc == "target_top_k_top_p" else 0
    top_p = 0.9 if trunc.startswith("target") else 1.0
    # thresholds from the project's own calls: the draft's nucleus from asd_draft_sample, the target's from the verify,
    # the bonus rows' (for the reference only) from the draft sampler's select on those rows
    d_thr = t_thr = b_thr = None
    if trunc != "none":
        rd = torch.from_numpy(rng.uniform(0, 1, B * K).astype(np.float32)).cuda()
        d_thr = Kn.DraftSampler(B * K, V, t.dtype)(d.view(B * K, V), rd, INV_T, 0.9).thr.view(B, K).contiguous()
    if trunc.startswith("target"):
        tok = torch.from_numpy(rng.integers(0, V, (B, K)).astype(np.int32)).cuda()
        lp_d = torch.from_numpy((-rng.uniform(0, 5, (B, K))).astype(np.float32)).cuda()
        u = torch.from_numpy(rng.uniform(0, 1, (B, K)).astype(np.float32)).cuda()
        rb = torch.from_numpy(rng.uniform(0, 1, B).astype(np.float32)).cuda()
        if top_k:
            t_thr = Kn.verify_accept_top_k(t, tok, lp_d, u, None, inv_temperature=INV_T, top_k=top_k, top_p=top_p).t_nucleus_logit
            b_thr = Kn.DraftSampler(B, V, t.dtype).top_k(bo, rb, INV_T, top_k=top_k, top_p=top_p).thr
        else:
            t_thr = Kn.verify_accept_top_p(t, tok, lp_d, u, None, inv_temperature=INV_T, top_p=top_p).t_nucleus_logit
            b_thr = Kn.DraftSampler(B, V, t.dtype)(bo, rb, INV_T, top_p).thr

    def existing(samp, bonus):
        if top_k:
            return samp.top_k(t, d, na, rr, bonus, INV_T, top_k=top_k, top_p=top_p, t_threshold=t_thr, d_threshold=d_thr)
        if top_p < 1.0:
            return samp.top_p(t, d, na, rr, bonus, INV_T, top_p=top_p, t_threshold=t_thr, d_threshold=d_thr)
        return samp(t, d, na, rr, bonus, INV_T, d_threshold=d_thr)

    def body(lib=None):
        if lib is not None:
            lib.asd_debug_residual_groups(int(groups))
        try:
            samp = Kn.ResidualSampler(B, V, t.dtype)
            out = {}
            for name, bonus in (("bonus", bo), ("no_bonus", None)):
                tok_ref = existing(samp, bonus).clone()
                torch.cuda.synchronize()
                ws_ref = samp.buf.clone()
                tok_lp, lp = samp.lp(t, d, na, rr, bonus, INV_T, top_k=top_k, top_p=top_p, t_threshold=t_thr, d_threshold=d_thr)
                torch.cuda.synchronize()
                ws_lp = samp.buf.clone()
                tok_again = existing(samp, bonus)
                torch.cuda.synchronize()
                out[name] = (tok_ref.cpu().numpy(), tok_lp.cpu().numpy(), lp.cpu().numpy(), tok_again.cpu().numpy(),
                             torch.equal(ws_ref, ws_lp))
            nvec = V * t.element_size() // 16
            mail0 = 256 + -(-B * 32 * 16 // 256) * 256 + -(-B * ((nvec + 63) // 64) * 8 // 256) * 256
            mail1 = int(Kn._lib().asd_residual_sample_workspace_bytes(B, V, Kn._DTYPE_CODE[t.dtype]))
            return out, samp.status(), int(samp.buf[mail0:mail1].count_nonzero()), int(samp.buf.count_nonzero())
        finally:
            if lib is not None:
                lib.asd_debug_residual_groups(0)

    if groups:
        with Kn.test_hooks() as lib:                # the TEST build of the library: the product one has no asd_debug_* switches
            out, status, mail_nonzero, ws_nonzero = body(lib)
    else:
        out, status, mail_nonzero, ws_nonzero = body()

    xt = O.logits_as_f32(st, dtype).reshape(B, K, V)
    xb = O.logits_as_f32(sb, dtype)
    t_thr_h = None if t_thr is None else t_thr.cpu().numpy()
    b_thr_h = None if b_thr is None else b_thr.cpu().numpy()
    worst = 0.0
    for name, (tok_ref, tok_lp, lp, tok_again, ws_same) in out.items():
        assert np.array_equal(tok_lp, tok_ref), (name, "the token is the existing entry point's, bit for bit")
        assert np.array_equal(tok_again, tok_ref), (name, "the existing entry point after the new one, same workspace")
        assert ws_same, (name, "the workspace is left exactly as the existing entry point leaves it")
        none = tok_lp == -1
        assert np.isnan(lp[none]).all() and np.isfinite(lp[~none]).all()
        if name == "no_bonus":
            assert none[n_acc == K].all() and none[2] and not none[n_acc < K].any()
        else:
            assert not none.any()
        for b in np.where(~none)[0]:
            j = int(n_acc[b])
            row, thr = (xt[b, j], -np.inf if t_thr_h is None else t_thr_h[b, j]) if j < K else \
                (xb[b], -np.inf if b_thr_h is None else b_thr_h[b])
            ref = ref_logprob(row, tok_lp[b], INV_T, thr)
            worst = max(worst, abs(float(lp[b]) - ref))
    print(f"residual_lp B={B} V={V} dtype={dtype} {trunc} groups={groups}: max |lp - f64| = {worst:.3g}")
    assert worst <= LP_ATOL, worst
    assert status == 0 and mail_nonzero == 0, "clean status word, mailboxes handed back empty"
    if groups >= 0 and not trunc.startswith("target"):
        assert ws_nonzero == 0, "the one-launch forms without a target nucleus leave the whole workspace all-zero"


@pytest.mark.parametrize("trunc", TRUNCATIONS)
@pytest.mark.parametrize("B", [3, 33, 100, 130])     # 130: past the group form's range (B <= 128), k_residual_row
@pytest.mark.parametrize("dtype", [O.DT_BF16, O.DT_F32, O.DT_F16])
def test_residual_sample_lp(dtype, B, trunc):
    from asd_amd import kernels as Kn
    _run(Kn, B, 4, 5000, dtype, trunc, seed=B * 7 + dtype)


@pytest.mark.parametrize("trunc", TRUNCATIONS)
@pytest.mark.parametrize("dtype", [O.DT_BF16, O.DT_F32])
def test_residual_sample_lp_three_launch_form(dtype, trunc):
    from asd_amd import kernels as Kn
    _run(Kn, 5, 4, 5000, dtype, trunc, seed=77 + dtype, groups=-1)


@pytest.mark.parametrize("trunc", TRUNCATIONS)
def test_residual_sample_lp_full_vocabulary(trunc):
    from asd_amd import kernels as Kn
    _run(Kn, 8, 4, 152064, O.DT_BF16, trunc, seed=5)


def test_lp_is_required():
    import torch
    from asd_amd import _binding
    lib = _binding.load_library()
    t = torch.zeros((2, 2, 1024), dtype=torch.bfloat16, device="cuda")
    z = torch.zeros(2, dtype=torch.int32, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    rc = lib.asd_residual_sample_lp(t.data_ptr(), 1024, t.data_ptr(), 1024, None, 1024, 1, z.data_ptr(), z.data_ptr(), 2, 2, 1024,
                                    1.0, 0, 1.0, None, None, z.data_ptr(), None, ws.data_ptr(), ws.numel(), None)
    assert rc == -1


def test_one_sequence_sliced_from_a_longer_output():
    """B = 1, as a verifying stage hands it over: score = t_out[:, :K].contiguous() of a [1, K + 1, V] output is the view itself
    (torch ignores the stride of a size-1 dimension), so stride(0) is (K + 1) V, not K V.  The launcher never uses that stride;
    it once refused such a tensor.  Same token and log-prob bits as the compact copy; two unevenly spaced sequences still raise."""
    import torch
    from asd_amd import kernels as Kn
    K, V = 4, 1024
    g = torch.Generator(device="cuda").manual_seed(3)
    out = torch.randn((1, K + 1, V), generator=g, device="cuda") * 3
    score, bonus = out[:, :K].contiguous(), out[:, K].contiguous()
    assert score.stride(0) == (K + 1) * V
    compact = torch.empty((1, K, V), device="cuda").copy_(score)
    d = compact + torch.randn((1, K, V), generator=g, device="cuda")
    samp = Kn.ResidualSampler(1, V, score.dtype)
    r = torch.full((1,), 0.37, device="cuda")
    for n in (0, 2, K):
        na = torch.full((1,), n, dtype=torch.int32, device="cuda")
        tok_a, lp_a = (x.clone() for x in samp.lp(score, d, na, r, bonus, INV_T))
        tok_b, lp_b = samp.lp(compact, d, na, r, bonus, INV_T)
        assert int(tok_a) == int(tok_b) >= 0 and lp_a.cpu().numpy().tobytes() == lp_b.cpu().numpy().tobytes()
        ref = ref_logprob((compact[0, n] if n < K else bonus[0]).cpu().numpy(), int(tok_a), INV_T)
        assert abs(float(lp_a) - ref) <= LP_ATOL
    two = torch.randn((2, K + 1, V), generator=g, device="cuda")
    with pytest.raises(ValueError, match="evenly spaced"):
        Kn.ResidualSampler(2, V, two.dtype).lp(two[:, :K], two[:, :K], torch.zeros(2, dtype=torch.int32, device="cuda"),
                                               torch.zeros(2, device="cuda"), None, INV_T)
    assert samp.status() == 0
