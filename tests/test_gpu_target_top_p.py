"""Target-side top-p: asd_verify_accept_top_p and asd_residual_sample_top_p (include/asd_hip.h).

The reference samples the target with HF generate(do_sample=True, temperature=0.7, top_p=0.9)
(generate_training_data.py:110-119, real_model_pipeline.py:60,326,378), and HF's assisted generation warps the target's
scores before `_speculative_sampling`: the target scores by its nucleus p^N, not by the full softmax(x / T).
Bars:
  - x* and lp_t are asd_draft_sample's nucleus_logit and log q(tok) on the same row, bit for bit (one select, shared code);
  - against the f64 oracle on rows stored with -inf below x* (the oracle's own x* where top_p is >= 1e-5 of mass away from a
    cumulative-mass step, the kernel's x* otherwise): lp_t within 1e-5, n_finite exactly, accept / n_acc away from the
    decision boundary, residual / bonus tokens away from CDF edges;
  - top_p = 1: the bits of asd_verify_accept_ex / asd_residual_sample_ex."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import encode_logits, make_verify_case, to_device_logits

pytestmark = pytest.mark.gpu

V_FULL = 152064
T = 0.7
INV_T = float(np.float32(1.0) / np.float32(T))
TOP_P = 0.9
NEG_INF_STORE = {O.DT_F32: np.float32(-np.inf), O.DT_BF16: np.uint16(0xFF80), O.DT_F16: np.uint16(0xFC00)}


@pytest.fixture(scope="module")
def K_():
    from asd_amd import kernels
    return kernels


def _masked(store, dtype, V, thr):
    """Storage rows [R, ld] with every score below the row's threshold replaced by -inf (the padding is left alone)."""
    out = store.copy()
    x = O.logits_as_f32(store[:, :V], dtype)
    below = x < np.asarray(thr, np.float32).reshape(-1, 1)
    out[:, :V][below] = NEG_INF_STORE[dtype]
    return out


def _gpu_verify(K_, case, top_p, inv_t=INV_T, ws=None):
    import torch
    B, K, V, dt = case["B"], case["K"], case["V"], case["dtype"]
    lg = to_device_logits(case["logits"], dt).view(B * K, case["ld"])[:, :V]
    res = K_.verify_accept_top_p(lg, torch.from_numpy(case["tok"]).cuda(), torch.from_numpy(case["lp_d"]).cuda(),
                                 torch.from_numpy(case["u"]).cuda(), ws, inv_temperature=inv_t, top_p=top_p)
    torch.cuda.synchronize()
    return {k: getattr(res, k).cpu().numpy() for k in ("lp_target", "accept", "n_acc", "accept_bits", "t_nucleus_logit", "n_finite")}


def _leading_finite(lp):
    fin = np.isfinite(lp)
    return np.where(fin.all(axis=1), lp.shape[1], np.argmin(fin, axis=1)).astype(np.int32)


def test_threshold_and_lp_equal_the_draft_samplers_on_the_fixture_rows(K_, golden):
    """tests/golden/top_p_nucleus.npz (HF TemperatureLogitsWarper + TopPLogitsWarper): the verify's x* is the draft sampler's
    nucleus_logit and lp_t of the token the sampler drew is its log q(tok) -- bit for bit -- and both match the warper."""
    import torch
    from tests.helpers import check_nucleus_against_warper, nucleus_cases
    g = golden.npz("top_p_nucleus.npz")
    n = 0
    for c in nucleus_cases(g):
        if not (0.0 < c["top_p"] < 1.0):
            continue
        inv_t = float(np.float32(1.0) / np.float32(c["T"]))
        lg = to_device_logits(c["store"], c["dtype"]).view(1, c["V"])
        d = K_.DraftSampler(1, c["V"], lg.dtype)(lg, torch.tensor([0.41], device="cuda"), inv_t, c["top_p"])
        res = K_.verify_accept_top_p(lg, d.tok.view(1, 1), torch.zeros((1, 1), device="cuda"), torch.full((1, 1), 0.5, device="cuda"),
                                     None, inv_temperature=inv_t, top_p=c["top_p"])
        torch.cuda.synchronize()
        thr, lp = res.t_nucleus_logit.cpu().numpy()[0, 0], res.lp_target.cpu().numpy()[0, 0]
        assert thr.tobytes() == d.thr.cpu().numpy()[0].tobytes(), (c["row"], thr, d.thr)
        assert lp.tobytes() == d.lp.cpu().numpy()[0].tobytes(), (c["row"], lp, d.lp)
        check_nucleus_against_warper(c, int(d.tok.cpu()[0]), float(lp), thr, 2e-5)
        n += 1
    assert n > 20


@pytest.mark.parametrize("dtype", [O.DT_BF16, O.DT_F16, O.DT_F32])
def test_threshold_and_lp_equal_the_draft_samplers_full_size(K_, dtype):
    """Full-size rows (V = 152064), 24 rows at once: every row's x* and the drawn token's lp_t equal asd_draft_sample's."""
    import torch
    R = 24
    rng = np.random.default_rng(7 + dtype)
    x = (rng.standard_normal((R, V_FULL)) * rng.uniform(1.0, 6.0, (R, 1))).astype(np.float32)
    lg = to_device_logits(encode_logits(x, dtype), dtype).view(R, V_FULL)
    d = K_.DraftSampler(R, V_FULL, lg.dtype)(lg, torch.from_numpy(rng.uniform(0, 1, R).astype(np.float32)).cuda(), INV_T, TOP_P)
    res = K_.verify_accept_top_p(lg, d.tok.view(R, 1), torch.zeros((R, 1), device="cuda"), torch.full((R, 1), 0.5, device="cuda"),
                                 None, inv_temperature=INV_T, top_p=TOP_P)
    torch.cuda.synchronize()
    assert res.t_nucleus_logit.cpu().numpy().reshape(-1).tobytes() == d.thr.cpu().numpy().tobytes()
    assert res.lp_target.cpu().numpy().reshape(-1).tobytes() == d.lp.cpu().numpy().tobytes()
    assert (res.n_finite.cpu().numpy() == 1).all()


# (B, K) x dtype: every batch size of the issue, K = 4 and 8, all three storage types (f32 rows are 600 KB: the largest
# batches run in the 16-bit types)
VERIFY_CASES = [(1, 8, O.DT_F32), (8, 4, O.DT_F32), (32, 8, O.DT_F32), (33, 4, O.DT_F32),
                (1, 4, O.DT_BF16), (8, 8, O.DT_BF16), (32, 8, O.DT_BF16), (33, 8, O.DT_BF16), (128, 8, O.DT_BF16),
                (1, 8, O.DT_F16), (8, 4, O.DT_F16), (32, 4, O.DT_F16), (33, 8, O.DT_F16), (128, 4, O.DT_F16)]


@pytest.mark.parametrize("B,K,dtype", VERIFY_CASES)
def test_verify_top_p_against_the_oracle_on_masked_rows(K_, B, K, dtype):
    case = make_verify_case(B, K, V_FULL, dtype, seed=300 + B * 10 + K + dtype, ld_row=V_FULL + 64)
    got = _gpu_verify(K_, case, TOP_P)
    R = B * K
    ds = O.draft_sample(case["logits"], dtype, np.full(R, 0.5, np.float32), R, V_FULL, INV_T, TOP_P, ld_row=case["ld"])
    thr = got["t_nucleus_logit"].reshape(-1)
    clear = ds["margin_p"] > 1e-5
    assert clear.mean() > 0.9
    assert thr[clear].tobytes() == ds["thr"][clear].tobytes()
    # the oracle scores the rows stored with -inf below x* (the kernel's own x* on the rows near a mass step)
    ref = O.verify_accept(_masked(case["logits"], dtype, V_FULL, thr), dtype, case["tok"], case["lp_d"], case["u"], B, K, V_FULL,
                          ld_row=case["ld"], n_threads=8, inv_temperature=INV_T)
    lp, want = got["lp_target"], ref["lp_t"]
    assert (np.isfinite(lp) == np.isfinite(want)).all()
    fin = np.isfinite(want)
    if R >= 16:
        assert fin.any() and (~fin).any()                # tokens inside and outside the nucleus
    np.testing.assert_allclose(lp[fin], want[fin], atol=1e-5, rtol=0)
    assert (got["n_finite"] == _leading_finite(want)).all()
    safe = ref["margin"] > 1e-5
    assert (got["accept"][safe] == ref["accept"][safe]).all()
    seq_safe = safe.all(axis=1)
    assert (got["n_acc"][seq_safe] == ref["n_acc"][seq_safe]).all()
    bits = (got["accept"].astype(np.uint64) << np.arange(K, dtype=np.uint64)).sum(axis=1)
    assert (got["accept_bits"].astype(np.uint64) == bits).all()
    inv = ~got["accept"].astype(bool)
    n = np.where(inv.any(axis=1), np.argmax(inv, axis=1), K)
    assert (got["n_acc"] == n).all()


def test_verify_top_p_edge_rows(K_):
    """Out-of-range tokens score -inf and reject; a NaN row gives NaN and rejects (as asd_verify_accept_ex); u = 0 never accepts
    a token outside the nucleus."""
    B, K = 2, 4
    case = make_verify_case(B, K, 32000, O.DT_BF16, seed=5)
    x = O.logits_as_f32(case["logits"], O.DT_BF16)
    case["tok"][0, 0], case["tok"][1, 0] = int(x[0].argmax()), int(x[K].argmax())      # inside the nucleus
    case["tok"][0, 1] = -3
    case["tok"][1, 2] = 32000
    case["logits"][5, 17] = np.uint16(0x7FC0)             # NaN in row (1, 1)
    case["u"][:] = 0.0
    got = _gpu_verify(K_, case, TOP_P)
    assert got["lp_target"][0, 1] == -np.inf and got["accept"][0, 1] == 0
    assert got["lp_target"][1, 2] == -np.inf and got["accept"][1, 2] == 0
    assert np.isnan(got["lp_target"][1, 1]) and got["accept"][1, 1] == 0
    assert got["n_finite"][0] == 1 and got["n_finite"][1] == 1
    assert got["n_acc"][0] == 1 and got["n_acc"][1] == 1          # u = 0 accepts every finite lp_t, nothing else


@pytest.mark.parametrize("dtype", [O.DT_BF16, O.DT_F32])
def test_top_p_one_is_bit_identical_to_the_existing_entry_points(K_, dtype):
    import torch
    B, K = 8, 4
    case = make_verify_case(B, K, V_FULL, dtype, seed=41)
    ws = K_.VerifyWorkspace(B, K, V_FULL, torch.float32 if dtype == O.DT_F32 else torch.bfloat16)
    for top_p in (1.0, 0.0, 1.5):
        got = _gpu_verify(K_, case, top_p, ws=ws)
        lg = to_device_logits(case["logits"], dtype).view(B, K, V_FULL)
        ref = K_.verify_accept(lg, torch.from_numpy(case["tok"]).cuda(), torch.from_numpy(case["lp_d"]).cuda(),
                               torch.from_numpy(case["u"]).cuda(), ws, inv_temperature=INV_T)
        torch.cuda.synchronize()
        for k in ("lp_target", "accept", "n_acc", "accept_bits"):
            assert got[k].tobytes() == getattr(ref, k).cpu().numpy().tobytes(), k
        assert (got["t_nucleus_logit"] == -np.inf).all()
        assert (got["n_finite"] == _leading_finite(got["lp_target"])).all()
    # the residual draw
    t = to_device_logits(case["logits"], dtype).view(B, K, V_FULL)
    d = to_device_logits(encode_logits(np.random.default_rng(3).standard_normal((B * K, V_FULL)).astype(np.float32) * 3, dtype), dtype).view(B, K, V_FULL)
    bonus = t[:, 0, :]
    n_acc = torch.tensor([0, 1, 2, 3, 4, 4, 0, 2], dtype=torch.int32, device="cuda")
    r = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, B).astype(np.float32)).cuda()
    rs = K_.ResidualSampler(B, V_FULL, t.dtype)
    a = rs(t, d, n_acc, r, bonus, INV_T).cpu().numpy()
    b = rs.top_p(t, d, n_acc, r, bonus, INV_T, top_p=1.0, t_threshold=None).cpu().numpy()
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("B,dtype", [(6, O.DT_BF16), (40, O.DT_F16), (100, O.DT_BF16), (12, O.DT_F32)])
def test_residual_draw_against_the_oracle_on_masked_rows(K_, B, dtype):
    """Rejection rows, bonus rows and empty residuals (draft row = target row, both truncated at the same x*): the token of
    the draw from max(0, p_t^N - p_d^N) / p_t^N / the bonus row's p^N equals the oracle's on masked rows, away from CDF edges;
    the bonus row's x* is asd_draft_sample's."""
    import torch
    K = 4
    rng = np.random.default_rng(900 + B + dtype)
    xt = (rng.standard_normal((B * K, V_FULL)) * 3.0).astype(np.float32)
    xd = (xt + rng.standard_normal((B * K, V_FULL)).astype(np.float32) * 0.7).astype(np.float32)
    xb = (rng.standard_normal((B, V_FULL)) * 3.0).astype(np.float32)
    n_acc = rng.integers(0, K + 1, B).astype(np.int32)
    n_acc[:3] = [0, K, 1]
    empty = rng.uniform(size=B) < 0.25
    for b in np.nonzero(empty)[0]:
        if n_acc[b] < K:
            xd[b * K + n_acc[b]] = xt[b * K + n_acc[b]]
    st, sd, sb = encode_logits(xt, dtype), encode_logits(xd, dtype), encode_logits(xb, dtype)
    t = to_device_logits(st, dtype).view(B, K, V_FULL)
    d = to_device_logits(sd, dtype).view(B, K, V_FULL)
    bon = to_device_logits(sb, dtype).view(B, V_FULL)
    R = B * K
    half = torch.full((R,), 0.5, device="cuda")
    dd = K_.DraftSampler(R, V_FULL, t.dtype)(d.view(R, V_FULL), half, INV_T, TOP_P)
    td = K_.DraftSampler(R, V_FULL, t.dtype)(t.view(R, V_FULL), half, INV_T, TOP_P)
    bd = K_.DraftSampler(B, V_FULL, t.dtype)(bon, torch.full((B,), 0.5, device="cuda"), INV_T, TOP_P)
    tthr = td.thr.view(B, K)
    r = rng.uniform(0, 1, B).astype(np.float32)
    rs = K_.ResidualSampler(B, V_FULL, t.dtype)
    got = rs.top_p(t, d, torch.from_numpy(n_acc).cuda(), torch.from_numpy(r).cuda(), bon, INV_T, top_p=TOP_P,
                   t_threshold=tthr, d_threshold=dd.thr.view(B, K)).cpu().numpy()
    torch.cuda.synchronize()
    tthr_h, dthr_h, bthr_h = tthr.cpu().numpy().reshape(-1), dd.thr.cpu().numpy(), bd.thr.cpu().numpy()
    # the oracle sees both rows stored with -inf below their thresholds (an empty residual is then exactly empty there too)
    want, margin = O.residual_sample(_masked(st, dtype, V_FULL, tthr_h), _masked(sd, dtype, V_FULL, dthr_h), dtype, n_acc, r, B, K,
                                     V_FULL, bonus=_masked(sb, dtype, V_FULL, bthr_h), inv_temperature=INV_T)
    safe = margin > 1e-5
    assert safe.mean() > 0.8
    bad = np.nonzero(safe & (got != want))[0]
    assert bad.size == 0, [(int(b), int(n_acc[b]), bool(empty[b]), float(margin[b]), int(got[b]), int(want[b])) for b in bad]
    # every committed token lies in its row's target nucleus
    for b in range(B):
        j = n_acc[b]
        row, thr = (xt[b * K + j], tthr_h[b * K + j]) if j < K else (xb[b], bthr_h[b])
        x = O.logits_as_f32(encode_logits(row[None, :], dtype), dtype)[0]
        assert x[got[b]] >= thr
    # the bonus token is the draft sampler's on the bonus row (the same x*, the same r)
    bon_rows = np.nonzero(n_acc == K)[0]
    bd2 = K_.DraftSampler(B, V_FULL, t.dtype)(bon, torch.from_numpy(r).cuda(), INV_T, TOP_P)
    tok2 = bd2.tok.cpu().numpy()
    assert bon_rows.size and (got[bon_rows][safe[bon_rows]] == tok2[bon_rows][safe[bon_rows]]).all()


def test_hf_fixture_target_top_p(K_, golden):
    """tests/golden/speculative_sampling_target_top_p.npz: transformers' _speculative_sampling, unmodified, on candidate AND
    target scores warped by TemperatureLogitsWarper(0.7) + TopPLogitsWarper(0.9).  n_acc equals HF's n_matches on every
    case; the committed token equals HF's (inverse CDF of its p') away from CDF edges, on the cases whose nuclei at the drawn
    position are HF's sets (the warper's sort drops some scores EQUAL to x*, which this build keeps by contract)."""
    import torch
    from tests.helpers import spec_full_cases
    g = golden.npz("speculative_sampling_target_top_p.npz")
    n = compared = 0
    for ci, c in enumerate(spec_full_cases(g)):
        K, V, dt = c["K"], c["V"], c["dtype"]
        new = to_device_logits(c["new"], dt).view(K + 1, V)
        cand = to_device_logits(c["cand"], dt).view(K, V)
        tok = torch.from_numpy(c["tok"]).cuda().view(1, K)
        res = K_.verify_accept_top_p(new[:K].view(1, K, V), tok, torch.from_numpy(c["lq"].astype(np.float32)).cuda().view(1, K),
                                     torch.from_numpy(c["u"]).cuda().view(1, K), None, inv_temperature=c["inv_t"], top_p=c["top_p"])
        torch.cuda.synchronize()
        n_acc = int(res.n_acc.cpu()[0])
        assert n_acc == c["n_matches"], (c["case"], n_acc, c["n_matches"])
        dthr = torch.from_numpy(c["thr"]).cuda().view(1, K)
        # the draw compares with HF's only where both nuclei of the drawn position are HF's: the target row's (the verify's x*,
        # the bonus row's from the draft sampler's select) and the draft row's (no equal scores dropped by the warper's sort)
        t0 = int(g["t_off"][ci])
        hf_t, hf_ties = g["t_thr"][t0 + n_acc], int(g["t_ties_removed"][t0 + n_acc])
        if n_acc < K:
            x_star = float(res.t_nucleus_logit.cpu()[0, n_acc])
            same = x_star == hf_t and c["ties_removed"][n_acc] == 0
        else:
            x_star = float(K_.DraftSampler(1, V, new.dtype)(new[K].view(1, V), torch.tensor([0.5], device="cuda"), c["inv_t"],
                                                            c["top_p"]).thr.cpu()[0])
            same = x_star == hf_t
        same = same and hf_ties == 0
        rs = K_.ResidualSampler(1, V, new.dtype)
        for i in range(c["r"].shape[0]):
            got = rs.top_p(new[:K].view(1, K, V), cand.view(1, K, V), res.n_acc, torch.tensor([float(c["r"][i])], device="cuda"),
                           new[K].view(1, V), c["inv_t"], top_p=c["top_p"], t_threshold=res.t_nucleus_logit, d_threshold=dthr)
            if same and c["margin"][i] > 1e-5:
                assert int(got.cpu()[0]) == int(c["want_tok"][i]), (c["case"], i)
                compared += 1
        n += 1
    assert n == 16 and compared >= 18


def _gpu_loop(dtype, keep=True, **cfg_kw):
    import torch
    from asd_amd.distributed import HipOps
    from asd_amd.serving import hierarchy as H
    from tests.test_hierarchy import NEW, P, V, _model, _predictor
    B, K = 6, 4
    cfg = H.HierarchyConfig(draft_len=K, temperature=0.7, top_p=0.9, lambda_value=25.0, seed=3, **cfg_kw)
    ops, pred = HipOps(), _predictor()
    prompt = torch.randint(0, V, (B, P), generator=torch.Generator().manual_seed(7)).cuda()
    d = H.DraftRole(_model(0, 0, dtype, "cuda"), cfg, ops, prompt, NEW, pred)
    ts = []
    for s, (noise, seed) in enumerate(zip((0.02, 0.04), (5, 6)), start=1):
        m = _model(noise, seed, dtype, "cuda")
        ts.append(H.VerifyRole(m, s, cfg, ops, prompt, NEW, pred, head=H.LogitsHead(m, ops), keep_inputs=keep))
    return H.generate_hierarchical(d, ts, keep_inputs=keep), ops, K


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_hierarchy_on_gpu_commits_from_the_target_nucleus(K_, dtype_name):
    """generate_hierarchical with small GPU tiers and target_top_p = 0.9: every token a verifying tier commits -- accepted
    drafts and drawn tokens alike -- lies in that tier's nucleus; the stop rule saw n_valid = n_finite.  With
    target_top_p = 1.0 the committed stream equals the default configuration's token for token."""
    import torch
    dtype = getattr(torch, dtype_name)
    tr, ops, K = _gpu_loop(dtype, target_top_p=TOP_P)
    torch.cuda.synchronize()
    checked = 0
    for rec in tr.records:
        for s, (v, drawn) in rec["tiers"].items():
            inp = v.inputs
            lg = inp["logits"]
            x = lg.float().cpu().numpy()
            thr = inp["t_nucleus_logit"].cpu().numpy()
            lp_t, n_acc, tok = inp["lp_t"].cpu().numpy(), inp["n_acc"].cpu().numpy(), inp["tok"].cpu().numpy()
            inside = np.take_along_axis(x, tok[..., None].astype(np.int64), 2)[..., 0] >= thr
            assert (np.isfinite(lp_t) == inside).all()
            assert (inp["n_finite"].cpu().numpy() == _leading_finite(lp_t)).all()
            assert (n_acc <= inp["n_finite"].cpu().numpy()).all()
            n, Kk, V = lg.shape
            d = K_.DraftSampler(n * Kk, V, lg.dtype)(lg.reshape(n * Kk, V).contiguous(), torch.full((n * Kk,), 0.5, device="cuda"),
                                                     INV_T, TOP_P)
            assert d.thr.cpu().numpy().tobytes() == thr.reshape(-1).tobytes()
            bon = inp["bonus_logits"].contiguous()
            bthr = K_.DraftSampler(n, V, bon.dtype)(bon, torch.full((n,), 0.5, device="cuda"), INV_T, TOP_P).thr.cpu().numpy()
            stop = v.stop.cpu().numpy()[v.idx.cpu().numpy()] == 1
            dr = drawn.cpu().numpy()
            for i in np.nonzero(stop)[0]:
                b, j = int(v.idx[i]), int(n_acc[i])
                row, x_star = (x[i, j], thr[i, j]) if j < K else (bon[i].float().cpu().numpy(), bthr[i])
                assert row[int(dr[b])] >= x_star, (s, b, j)
                checked += 1
    assert checked > 10
    a, _, _ = _gpu_loop(dtype, keep=False)
    b, _, _ = _gpu_loop(dtype, keep=False, target_top_p=1.0)
    assert torch.equal(a.tokens, b.tokens) and a.tier_counts == b.tier_counts
