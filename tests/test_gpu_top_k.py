"""Top-k before top-p: asd_draft_sample_top_k, asd_verify_accept_top_k and asd_residual_sample_top_k (include/asd_hip.h).

The reference calls HF generate(do_sample=True, temperature=0.7, top_p=0.9) and passes no top_k, so transformers applies its
default top_k = 50: the warper chain is Temperature -> TopK -> TopP on the draft's scores and on the target's.  Bars:
  - x_k (top_p off) equals numpy's k-th largest exactly, ties and short rows included;
  - the combined threshold max(x_k, x*_K) equals max(x_k, O.draft_sample(row masked below x_k).thr) wherever the oracle's
    top_p is >= 1e-5 of mass away from a cumulative-mass step, and HF's set on the fixture rows;
  - the draft sampler's threshold, the verify's t_nucleus_logit and the bonus row's threshold are one select: the same bits;
  - against the f64 oracle on rows stored with -inf below the threshold: lp within 1e-5, accept / n_acc away from the decision
    margin, tokens away from CDF edges;
  - top_k <= 0 or >= V: the bits of the top-p entry points; the outputs do not depend on the geometry."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import encode_logits, make_verify_case, to_device_logits

pytestmark = pytest.mark.gpu

V_FULL = 152064
T = 0.7
INV_T = float(np.float32(1.0) / np.float32(T))
TOP_K, TOP_P = 50, 0.9
NEG_INF_STORE = {O.DT_F32: np.float32(-np.inf), O.DT_BF16: np.uint16(0xFF80), O.DT_F16: np.uint16(0xFC00)}


@pytest.fixture(scope="module")
def K_():
    from asd_amd import kernels
    return kernels


def x_k_of(x, top_k):
    """The top_k-th largest value of every row of x [R, V] (f32) counting multiplicity; -inf with fewer than top_k values > -inf."""
    x = np.asarray(x, np.float32)
    Vr = x.shape[-1]
    kth = np.partition(x, Vr - top_k, axis=-1)[:, Vr - top_k]
    return np.where((x > -np.inf).sum(-1) >= top_k, kth, -np.inf).astype(np.float32)


def _masked(store, dtype, V, thr):
    """Storage rows [R, ld] with every score below the row's threshold replaced by -inf (the padding is left alone)."""
    out = store.copy()
    x = O.logits_as_f32(store[:, :V], dtype)
    below = x < np.asarray(thr, np.float32).reshape(-1, 1)
    out[:, :V][below] = NEG_INF_STORE[dtype]
    return out


def oracle_thr(store, dtype, V, top_k, top_p, inv_t=INV_T):
    """(thr, margin_p): max(x_k, x*_K) with x*_K the oracle's nucleus threshold of the row masked below x_k."""
    R = store.shape[0]
    x_k = x_k_of(O.logits_as_f32(store[:, :V], dtype), top_k)
    ds = O.draft_sample(_masked(store, dtype, V, x_k), dtype, np.full(R, 0.5, np.float32), R, V, inv_t, top_p,
                        ld_row=store.shape[1])
    return np.maximum(x_k, ds["thr"]).astype(np.float32), ds["margin_p"]


def _dev_rows(store, dtype, R, V):
    return to_device_logits(store, dtype).view(R, store.shape[1])[:, :V]


def _draft(K_, store, dtype, R, V, r, top_k, top_p, inv_t=INV_T):
    import torch
    lg = _dev_rows(store, dtype, R, V)
    d = K_.DraftSampler(R, V, lg.dtype).top_k(lg, torch.from_numpy(np.asarray(r, np.float32)).cuda(), inv_t, top_k=top_k,
                                              top_p=top_p)
    torch.cuda.synchronize()
    return d.tok.cpu().numpy(), d.lp.cpu().numpy(), d.thr.cpu().numpy()


def _verify(K_, case, top_k, top_p, inv_t=INV_T, ws=None):
    import torch
    B, K, V, dt = case["B"], case["K"], case["V"], case["dtype"]
    lg = to_device_logits(case["logits"], dt).view(B * K, case["ld"])[:, :V]
    res = K_.verify_accept_top_k(lg, torch.from_numpy(case["tok"]).cuda(), torch.from_numpy(case["lp_d"]).cuda(),
                                 torch.from_numpy(case["u"]).cuda(), ws, inv_temperature=inv_t, top_k=top_k, top_p=top_p)
    torch.cuda.synchronize()
    return {k: getattr(res, k).cpu().numpy() for k in ("lp_target", "accept", "n_acc", "accept_bits", "t_nucleus_logit", "n_finite")}


def _leading_finite(lp):
    fin = np.isfinite(lp)
    return np.where(fin.all(axis=1), lp.shape[1], np.argmin(fin, axis=1)).astype(np.int32)


def _x_k_rows(V, dtype, top_k, seed):
    """Rows of every kind the count select must get right: Gaussian, quantised to a coarse grid (many exact ties), all-equal,
    with -inf entries, and with fewer than top_k values > -inf."""
    rng = np.random.default_rng(seed)
    rows = [rng.standard_normal(V) * 3.0, rng.standard_normal(V) * 0.01 - 5.0,
            np.round(rng.standard_normal(V) * 2.0) / 2.0,                 # ~20 distinct values
            np.full(V, 1.25)]
    r = rng.standard_normal(V) * 2.0
    r[rng.uniform(size=V) < 0.3] = -np.inf
    rows.append(r)
    short = np.full(V, -np.inf)
    n_fin = max(top_k - 1, 0)
    short[rng.choice(V, n_fin, replace=False)] = rng.standard_normal(n_fin)
    rows.append(short)
    ties = rng.standard_normal(V) * 3.0                               # the boundary value repeated around x_k
    srt = np.sort(ties)[::-1]
    ties[np.argsort(-ties)[max(top_k - 3, 0):top_k + 3]] = srt[top_k - 1]
    rows.append(ties)
    x = np.stack(rows).astype(np.float32)
    store = encode_logits(x, dtype)
    return store, O.logits_as_f32(store, dtype)


@pytest.mark.parametrize("dtype", [O.DT_BF16, O.DT_F16, O.DT_F32])
@pytest.mark.parametrize("V", [V_FULL, 1000])
def test_x_k_is_exact(K_, dtype, V):
    """top_p off: the threshold is numpy's k-th largest value and { x >= thr } has the size numpy counts, ties included."""
    n_rows = 0
    for top_k in (1, 50, 1000, V - 1):
        if not 0 < top_k < V:
            continue
        store, x = _x_k_rows(V, dtype, top_k, seed=top_k + V + dtype)
        R = x.shape[0]
        r = np.random.default_rng(top_k).uniform(0, 1, R).astype(np.float32)
        tok, lp, thr = _draft(K_, store, dtype, R, V, r, top_k, 1.0)
        want = x_k_of(x, top_k)
        assert np.array_equal(thr, want), (top_k, thr, want)
        assert ((x >= thr[:, None]).sum(1) == (x >= want[:, None]).sum(1)).all()
        assert thr[-2] == -np.inf                                 # fewer than k values > -inf: the whole row is kept
        for i in range(R):
            if tok[i] >= 0:
                assert x[i, tok[i]] >= thr[i] and np.isfinite(lp[i]), (top_k, i)
        n_rows += R
    assert n_rows >= 3 * 7


def test_combined_threshold_matches_hf_on_the_fixture_rows(K_, golden):
    """tests/golden/speculative_sampling_top_k.npz: on every candidate row and target row, x_k is the fixture's (numpy) and
    the combined threshold is HF's (TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper): the same value and,
    where the warper's sort dropped no score equal to it, the same kept-set size."""
    from tests.helpers import spec_full_cases
    g = golden.npz("speculative_sampling_top_k.npz")
    compared = off = 0
    for ci, c in enumerate(spec_full_cases(g)):
        K, V, dt = c["K"], c["V"], c["dtype"]
        top_k, top_p = int(g["case_top_k"][ci]), float(g["case_top_p"][ci])
        a, b = int(g["off"][ci]), int(g["off"][ci + 1])
        t0, t1 = int(g["t_off"][ci]), int(g["t_off"][ci + 1])
        for store, R, hf_xk, hf_thr, hf_keep, hf_ties in (
                (c["cand"], K, g["x_k"][a:b], g["thr"][a:b], g["n_keep"][a:b], g["ties_removed"][a:b]),
                (c["new"], K + 1, g["t_x_k"][t0:t1], g["t_thr"][t0:t1], g["t_n_keep"][t0:t1], g["t_ties_removed"][t0:t1])):
            x = O.logits_as_f32(store, dt)
            _, _, xk = _draft(K_, store, dt, R, V, np.full(R, 0.5, np.float32), top_k, 1.0)
            assert np.array_equal(xk, hf_xk), (c["case"], xk, hf_xk)
            _, _, thr = _draft(K_, store, dt, R, V, np.full(R, 0.5, np.float32), top_k, top_p)
            # (top_p within float rounding of a cumulative-mass step may move HF's f32 cumsum and the fixed-point select apart)
            same = thr == hf_thr
            off += int((~same).sum())
            assert ((x >= thr[:, None]).sum(1)[same] == (hf_keep + hf_ties)[same]).all()
            compared += R
    assert compared >= 200 and off <= 2, off


@pytest.mark.parametrize("dtype", [O.DT_BF16, O.DT_F16, O.DT_F32])
def test_combined_threshold_matches_the_masked_oracle_and_hf_full_size(K_, dtype):
    """Full-size random rows: thr = max(x_k, O.draft_sample(row masked below x_k).thr) where the oracle's top_p is clear of a
    mass step, and the kept set is the one transformers' own warpers keep (16-bit rows: the same set)."""
    import torch
    R = 16
    rng = np.random.default_rng(70 + dtype)
    x = (rng.standard_normal((R, V_FULL)) * rng.uniform(0.5, 6.0, (R, 1))).astype(np.float32)
    store = encode_logits(x, dtype)
    xf = O.logits_as_f32(store, dtype)
    for top_k, top_p in ((TOP_K, TOP_P), (20, 0.8), (1000, 0.5), (5, 0.99)):
        _, _, thr = _draft(K_, store, dtype, R, V_FULL, rng.uniform(0, 1, R), top_k, top_p)
        want, margin = oracle_thr(store, dtype, V_FULL, top_k, top_p)
        clear = margin > 1e-5
        assert clear.mean() > 0.8
        assert np.array_equal(thr[clear], want[clear]), top_k
        assert (thr >= x_k_of(xf, top_k)).all()
        if dtype != O.DT_F32:
            from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
            s = TemperatureLogitsWarper(T)(None, torch.from_numpy(xf.copy()))
            s = TopPLogitsWarper(top_p)(None, TopKLogitsWarper(top_k)(None, s))
            hf_keep = torch.isfinite(s).numpy()
            mine = xf >= thr[:, None]
            # HF's sort may drop scores EQUAL to the threshold; this build keeps every tie by contract
            for i in np.nonzero(clear)[0]:
                assert not (hf_keep[i] & ~mine[i]).any(), (top_k, i)
                assert (xf[i][mine[i] & ~hf_keep[i]] == thr[i]).all(), (top_k, i)


@pytest.mark.parametrize("dtype", [O.DT_BF16, O.DT_F16, O.DT_F32])
def test_one_select_for_draft_verify_and_bonus(K_, dtype):
    """The draft sampler's threshold, the verify's t_nucleus_logit and lp_t (for the token the sampler drew) are the same
    bits; the bonus draw of the residual sampler (its own select on the bonus row) is the draft sampler's token."""
    import torch
    R = 24
    rng = np.random.default_rng(17 + dtype)
    x = (rng.standard_normal((R, V_FULL)) * rng.uniform(1.0, 6.0, (R, 1))).astype(np.float32)
    store = encode_logits(x, dtype)
    r = rng.uniform(0, 1, R).astype(np.float32)
    for top_k, top_p in ((TOP_K, TOP_P), (TOP_K, 1.0), (7, 0.95)):
        tok, lp, thr = _draft(K_, store, dtype, R, V_FULL, r, top_k, top_p)
        lg = _dev_rows(store, dtype, R, V_FULL)
        res = K_.verify_accept_top_k(lg, torch.from_numpy(tok).cuda().view(R, 1), torch.zeros((R, 1), device="cuda"),
                                     torch.full((R, 1), 0.5, device="cuda"), None, inv_temperature=INV_T, top_k=top_k, top_p=top_p)
        torch.cuda.synchronize()
        assert res.t_nucleus_logit.cpu().numpy().reshape(-1).tobytes() == thr.tobytes()
        assert res.lp_target.cpu().numpy().reshape(-1).tobytes() == lp.tobytes()
        assert (res.n_finite.cpu().numpy() == 1).all()
        # the bonus rows: n_acc = K = 1 draws from each row's own kept set with the same r
        rs = K_.ResidualSampler(R, V_FULL, lg.dtype)
        t3 = lg.contiguous().view(R, 1, V_FULL)
        got = rs.top_k(t3, t3, torch.ones(R, dtype=torch.int32, device="cuda"), torch.from_numpy(r).cuda(), lg.contiguous(), INV_T,
                       top_k=top_k, top_p=top_p, t_threshold=torch.from_numpy(thr).cuda().view(R, 1)).cpu().numpy()
        ref = O.draft_sample(_masked(store, dtype, V_FULL, thr), dtype, r, R, V_FULL, INV_T, 1.0)
        far = ref["margin_r"] > 1e-5
        assert far.mean() > 0.8
        assert np.array_equal(got[far], tok[far]), top_k


@pytest.mark.parametrize("B,dtype", [(1, O.DT_F32), (8, O.DT_BF16), (32, O.DT_BF16), (33, O.DT_F16), (128, O.DT_BF16)])
def test_draft_top_k_against_the_oracle_on_masked_rows(K_, B, dtype):
    rng = np.random.default_rng(500 + B + dtype)
    x = (rng.standard_normal((B, V_FULL)) * 3.0).astype(np.float32)
    store = encode_logits(x, dtype)
    r = rng.uniform(0, 1, B).astype(np.float32)
    tok, lp, thr = _draft(K_, store, dtype, B, V_FULL, r, TOP_K, TOP_P)
    want_thr, margin = oracle_thr(store, dtype, V_FULL, TOP_K, TOP_P)
    clear = margin > 1e-5
    assert np.array_equal(thr[clear], want_thr[clear])
    ref = O.draft_sample(_masked(store, dtype, V_FULL, thr), dtype, r, B, V_FULL, INV_T, 1.0)
    np.testing.assert_allclose(lp, ref["lp"], atol=1e-5, rtol=0)
    far = ref["margin_r"] > 1e-5
    assert np.array_equal(tok[far], ref["tok"][far])


VERIFY_CASES = [(1, 8, O.DT_F32), (8, 4, O.DT_F32), (32, 8, O.DT_BF16), (33, 8, O.DT_BF16), (8, 8, O.DT_F16),
                (32, 4, O.DT_F16), (128, 4, O.DT_BF16)]


@pytest.mark.parametrize("B,K,dtype", VERIFY_CASES)
def test_verify_top_k_against_the_oracle_on_masked_rows(K_, B, K, dtype):
    case = make_verify_case(B, K, V_FULL, dtype, seed=700 + B * 10 + K + dtype, ld_row=V_FULL + 64)
    got = _verify(K_, case, TOP_K, TOP_P)
    thr = got["t_nucleus_logit"].reshape(-1)
    want_thr, margin = oracle_thr(case["logits"], dtype, V_FULL, TOP_K, TOP_P)
    clear = margin > 1e-5
    assert clear.mean() > 0.8
    assert np.array_equal(thr[clear], want_thr[clear])
    ref = O.verify_accept(_masked(case["logits"], dtype, V_FULL, thr), dtype, case["tok"], case["lp_d"], case["u"], B, K, V_FULL,
                          ld_row=case["ld"], n_threads=8, inv_temperature=INV_T)
    lp, want = got["lp_target"], ref["lp_t"]
    assert (np.isfinite(lp) == np.isfinite(want)).all()
    fin = np.isfinite(want)
    if B * K >= 16:
        assert fin.any() and (~fin).any()
    np.testing.assert_allclose(lp[fin], want[fin], atol=1e-5, rtol=0)
    assert (got["n_finite"] == _leading_finite(want)).all()
    assert (got["n_acc"] <= got["n_finite"]).all()
    safe = ref["margin"] > 1e-5
    assert (got["accept"][safe] == ref["accept"][safe]).all()
    seq_safe = safe.all(axis=1)
    assert (got["n_acc"][seq_safe] == ref["n_acc"][seq_safe]).all()
    inv = ~got["accept"].astype(bool)
    assert (got["n_acc"] == np.where(inv.any(axis=1), np.argmax(inv, axis=1), K)).all()


@pytest.mark.parametrize("B,dtype", [(6, O.DT_BF16), (40, O.DT_F16), (100, O.DT_BF16), (12, O.DT_F32)])
def test_residual_top_k_against_the_oracle_on_masked_rows(K_, B, dtype):
    """Rejection rows, bonus rows and empty residuals: the committed token equals the oracle's on rows masked below the
    verify's / draft's / bonus row's thresholds, away from CDF edges, and lies in its row's kept set."""
    import torch
    K = 4
    rng = np.random.default_rng(1900 + B + dtype)
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
    R = B * K
    half = np.full(R, 0.5, np.float32)
    _, _, dthr = _draft(K_, sd, dtype, R, V_FULL, half, TOP_K, TOP_P)
    _, _, tthr = _draft(K_, st, dtype, R, V_FULL, half, TOP_K, TOP_P)
    _, _, bthr = _draft(K_, sb, dtype, B, V_FULL, half[:B], TOP_K, TOP_P)
    t = to_device_logits(st, dtype).view(B, K, V_FULL)
    d = to_device_logits(sd, dtype).view(B, K, V_FULL)
    bon = to_device_logits(sb, dtype).view(B, V_FULL)
    r = rng.uniform(0, 1, B).astype(np.float32)
    rs = K_.ResidualSampler(B, V_FULL, t.dtype)
    got = rs.top_k(t, d, torch.from_numpy(n_acc).cuda(), torch.from_numpy(r).cuda(), bon, INV_T, top_k=TOP_K, top_p=TOP_P,
                   t_threshold=torch.from_numpy(tthr).cuda().view(B, K),
                   d_threshold=torch.from_numpy(dthr).cuda().view(B, K)).cpu().numpy()
    torch.cuda.synchronize()
    assert rs.status() == 0
    want, margin = O.residual_sample(_masked(st, dtype, V_FULL, tthr), _masked(sd, dtype, V_FULL, dthr), dtype, n_acc, r, B, K,
                                     V_FULL, bonus=_masked(sb, dtype, V_FULL, bthr), inv_temperature=INV_T)
    safe = margin > 1e-5
    assert safe.mean() > 0.8
    bad = np.nonzero(safe & (got != want))[0]
    assert bad.size == 0, [(int(b), int(n_acc[b]), bool(empty[b]), float(margin[b]), int(got[b]), int(want[b])) for b in bad]
    xtf, xbf = O.logits_as_f32(st, dtype), O.logits_as_f32(sb, dtype)
    for b in range(B):
        j = n_acc[b]
        row, thr = (xtf[b * K + j], tthr[b * K + j]) if j < K else (xbf[b], bthr[b])
        assert row[got[b]] >= thr
        assert thr >= x_k_of(row[None, :], TOP_K)[0]                # the top-k set (ties included) bounds what is drawn


def test_hf_fixture_top_k(K_, golden):
    """tests/golden/speculative_sampling_top_k.npz: transformers' _speculative_sampling, unmodified, on candidate AND target
    scores warped by Temperature -> TopK -> TopP.  n_acc equals HF's n_matches on every case, the committed token equals HF's
    away from CDF edges where the kept sets are HF's; the top-p-only entry points disagree on the recorded cases."""
    import torch
    from tests.helpers import spec_full_cases
    g = golden.npz("speculative_sampling_top_k.npz")
    n = compared = differ_acc = 0
    for ci, c in enumerate(spec_full_cases(g)):
        K, V, dt = c["K"], c["V"], c["dtype"]
        top_k, top_p = int(g["case_top_k"][ci]), float(g["case_top_p"][ci])
        new = to_device_logits(c["new"], dt).view(K + 1, V)
        cand = to_device_logits(c["cand"], dt).view(K, V)
        tok = torch.from_numpy(c["tok"]).cuda().view(1, K)
        lq = torch.from_numpy(c["lq"].astype(np.float32)).cuda().view(1, K)
        u = torch.from_numpy(c["u"]).cuda().view(1, K)
        res = K_.verify_accept_top_k(new[:K].view(1, K, V), tok, lq, u, None, inv_temperature=c["inv_t"], top_k=top_k, top_p=top_p)
        only_p = K_.verify_accept_top_p(new[:K].view(1, K, V), tok, lq, u, None, inv_temperature=c["inv_t"], top_p=top_p)
        torch.cuda.synchronize()
        n_acc = int(res.n_acc.cpu()[0])
        assert n_acc == c["n_matches"], (c["case"], n_acc, c["n_matches"])
        # the top-p-only path: a larger kept set on every target row whose HF sets differ, and HF's other n_matches
        t0 = int(g["t_off"][ci])
        x = O.logits_as_f32(c["new"], dt)[:K]
        kp = (x >= only_p.t_nucleus_logit.cpu().numpy().reshape(K, 1)).sum(1)
        kk = (x >= res.t_nucleus_logit.cpu().numpy().reshape(K, 1)).sum(1)
        diff = g["t_n_keep_top_p"][t0:t0 + K] != g["t_n_keep"][t0:t0 + K]
        assert diff.any() and (kp[diff] > kk[diff]).all(), c["case"]
        if int(g["n_matches_top_p"][ci]) != c["n_matches"]:
            assert int(only_p.n_acc.cpu()[0]) != n_acc
            differ_acc += 1
        # the draw, where the kept sets of the drawn position are HF's (no tie at the threshold dropped by the warper's sort)
        hf_t, hf_ties = g["t_thr"][t0 + n_acc], int(g["t_ties_removed"][t0 + n_acc])
        if n_acc < K:
            same = float(res.t_nucleus_logit.cpu()[0, n_acc]) == hf_t and c["ties_removed"][n_acc] == 0
        else:
            same = True
        same = same and hf_ties == 0
        dthr = torch.from_numpy(c["thr"]).cuda().view(1, K)
        rs = K_.ResidualSampler(1, V, new.dtype)
        for i in range(c["r"].shape[0]):
            got = rs.top_k(new[:K].view(1, K, V), cand.view(1, K, V), res.n_acc, torch.tensor([float(c["r"][i])], device="cuda"),
                           new[K].view(1, V), c["inv_t"], top_k=top_k, top_p=top_p, t_threshold=res.t_nucleus_logit,
                           d_threshold=dthr)
            if same and c["margin"][i] > 1e-5:
                assert int(got.cpu()[0]) == int(c["want_tok"][i]), (c["case"], i)
                compared += 1
        n += 1
    assert n == 16 and compared >= 18 and differ_acc >= 1


@pytest.mark.parametrize("dtype", [O.DT_BF16, O.DT_F32])
def test_off_switch_is_bit_identical_to_the_top_p_entry_points(K_, dtype):
    import torch
    B, K = 8, 4
    V = V_FULL
    case = make_verify_case(B, K, V, dtype, seed=43)
    tdt = torch.float32 if dtype == O.DT_F32 else torch.bfloat16
    ws = K_.VerifyWorkspace(B, K, V, tdt)
    lg = to_device_logits(case["logits"], dtype).view(B * K, V)
    rr = torch.from_numpy(np.random.default_rng(1).uniform(0, 1, B * K).astype(np.float32)).cuda()
    ds = K_.DraftSampler(B * K, V, tdt)
    t = lg.view(B, K, V)
    d = to_device_logits(encode_logits(np.random.default_rng(3).standard_normal((B * K, V)).astype(np.float32) * 3, dtype),
                         dtype).view(B, K, V)
    n_acc = torch.tensor([0, 1, 2, 3, 4, 4, 0, 2], dtype=torch.int32, device="cuda")
    r = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, B).astype(np.float32)).cuda()
    rs = K_.ResidualSampler(B, V, tdt)
    for top_p in (TOP_P, 1.0):
        a = ds(lg, rr, INV_T, top_p)
        a = [x.cpu().numpy().tobytes() for x in (a.tok, a.lp, a.thr)]
        ref = _verify(K_, case, 0, top_p, ws=ws)                  # top_k = 0 is verify_accept_top_p ...
        ref_p = K_.verify_accept_top_p(lg.view(B, K, V), torch.from_numpy(case["tok"]).cuda(), torch.from_numpy(case["lp_d"]).cuda(),
                                       torch.from_numpy(case["u"]).cuda(), ws, inv_temperature=INV_T, top_p=top_p)
        torch.cuda.synchronize()
        for k in ref:
            assert ref[k].tobytes() == getattr(ref_p, k).cpu().numpy().tobytes(), k
        d_thr = torch.from_numpy(np.frombuffer(a[2], np.float32).copy()).cuda().view(B, K)
        want_rs = rs.top_p(t, d, n_acc, r, t[:, 0, :], INV_T, top_p=top_p, t_threshold=ref_p.t_nucleus_logit,
                           d_threshold=d_thr).cpu().numpy().tobytes()
        for top_k in (0, -1, V, V + 5):
            b = ds.top_k(lg, rr, INV_T, top_k=top_k, top_p=top_p)
            assert [x.cpu().numpy().tobytes() for x in (b.tok, b.lp, b.thr)] == a, top_k
            got = _verify(K_, case, top_k, top_p, ws=ws)
            for k in got:
                assert got[k].tobytes() == ref[k].tobytes(), (top_k, k)
            g = rs.top_k(t, d, n_acc, r, t[:, 0, :], INV_T, top_k=top_k, top_p=top_p, t_threshold=ref_p.t_nucleus_logit,
                         d_threshold=d_thr).cpu().numpy().tobytes()
            assert g == want_rs, top_k
        assert ds.status() == 0 and rs.status() == 0


@pytest.mark.parametrize("dtype", [O.DT_BF16, O.DT_F32])
@pytest.mark.parametrize("B", [8, 32])
def test_outputs_do_not_depend_on_the_geometry(K_, dtype, B):
    """Through the test library's geometry switches: every workgroups-per-row setting of the draft sampler gives the same
    threshold / lp / token bits and hands its workspace back all-zero; every residual geometry commits the same token away
    from CDF edges with a clean status word."""
    import torch
    V = V_FULL
    rng = np.random.default_rng(B + dtype)
    store = encode_logits((rng.standard_normal((B, V)) * 3.0).astype(np.float32), dtype)
    r = rng.uniform(0, 1, B).astype(np.float32)
    lg = _dev_rows(store, dtype, B, V)
    base = None
    with K_.test_hooks() as lib:
        try:
            for gph in (-1, 0, 2, 8, 32):
                lib.asd_debug_draft_groups(int(gph if gph <= 0 or B * gph <= 256 else 0))
                samp = K_.DraftSampler(B, V, lg.dtype)
                dd = samp.top_k(lg, torch.from_numpy(r).cuda(), INV_T, top_k=TOP_K, top_p=TOP_P)
                torch.cuda.synchronize()
                assert int(samp.buf.count_nonzero()) == 0
                out = [x.cpu().numpy().tobytes() for x in (dd.tok, dd.lp, dd.thr)]
                base = out if base is None else base
                assert out == base, gph
        finally:
            lib.asd_debug_draft_groups(0)
        thr = torch.from_numpy(np.frombuffer(base[2], np.float32).copy()).cuda()
        K = 2
        t = lg.contiguous().view(B, 1, V).expand(B, K, V).contiguous()
        dl = t.flip(2).contiguous()
        n_acc = torch.from_numpy(rng.integers(0, K + 1, B).astype(np.int32)).cuda()
        rr = torch.from_numpy(rng.uniform(0, 1, B).astype(np.float32)).cuda()
        tt = thr.view(B, 1).expand(B, K).contiguous()
        want = None
        try:
            for gph in (-1, 0, 2, 4, 8):
                lib.asd_debug_residual_groups(int(gph if gph <= 0 or B * gph <= 256 else 0))
                rs = K_.ResidualSampler(B, V, lg.dtype)
                got = rs.top_k(t, dl, n_acc, rr, lg.contiguous(), INV_T, top_k=TOP_K, top_p=TOP_P, t_threshold=tt,
                               d_threshold=tt.flip(1).contiguous()).cpu().numpy()
                torch.cuda.synchronize()
                assert rs.status() == 0
                want = got if want is None else want
                assert (got != want).sum() <= 1, gph          # (the group forms sum tile masses in their own order)
        finally:
            lib.asd_debug_residual_groups(0)


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_hierarchy_on_gpu_commits_from_the_top_k_set(K_, dtype_name):
    """generate_hierarchical with small GPU tiers, top_k = target_top_k = 50 and top_p = target_top_p = 0.9: every token a
    verifying tier commits by a draw lies in its row's kept set, lp_t is finite exactly there, n_acc <= n_finite, and the
    stream differs from the same run with top-k off."""
    import torch
    from tests.test_gpu_target_top_p import _gpu_loop
    dtype = getattr(torch, dtype_name)
    tr, ops, K = _gpu_loop(dtype, top_k=TOP_K, target_top_k=TOP_K, target_top_p=TOP_P)
    torch.cuda.synchronize()
    checked = 0
    for rec in tr.records:
        for s, (v, drawn) in rec["tiers"].items():
            inp = v.inputs
            lg = inp["logits"]
            x = lg.float().cpu().numpy()
            thr = inp["t_nucleus_logit"].cpu().numpy()
            lp_t, n_acc, tok = inp["lp_t"].cpu().numpy(), inp["n_acc"].cpu().numpy(), inp["tok"].cpu().numpy()
            assert (thr >= x_k_of(x.reshape(-1, x.shape[-1]), TOP_K).reshape(thr.shape)).all()
            inside = np.take_along_axis(x, tok[..., None].astype(np.int64), 2)[..., 0] >= thr
            assert (np.isfinite(lp_t) == inside).all()
            assert (inp["n_finite"].cpu().numpy() == _leading_finite(lp_t)).all()
            assert (n_acc <= inp["n_finite"].cpu().numpy()).all()
            n, Kk, V = lg.shape
            dthr = K_.DraftSampler(n * Kk, V, lg.dtype).top_k(lg.reshape(n * Kk, V).contiguous(),
                                                              torch.full((n * Kk,), 0.5, device="cuda"), INV_T, top_k=TOP_K,
                                                              top_p=TOP_P).thr
            assert dthr.cpu().numpy().tobytes() == thr.reshape(-1).tobytes()
            bon = inp["bonus_logits"].contiguous()
            bthr = K_.DraftSampler(n, V, bon.dtype).top_k(bon, torch.full((n,), 0.5, device="cuda"), INV_T, top_k=TOP_K,
                                                          top_p=TOP_P).thr.cpu().numpy()
            stop = v.stop.cpu().numpy()[v.idx.cpu().numpy()] == 1
            dr = drawn.cpu().numpy()
            for i in np.nonzero(stop)[0]:
                b, j = int(v.idx[i]), int(n_acc[i])
                row, bound = (x[i, j], thr[i, j]) if j < K else (bon[i].float().cpu().numpy(), bthr[i])
                assert row[int(dr[b])] >= bound, (s, b, j)
                checked += 1
    assert checked > 10
    a, _, _ = _gpu_loop(dtype, keep=False, target_top_p=TOP_P)
    b, _, _ = _gpu_loop(dtype, keep=False, top_k=TOP_K, target_top_k=TOP_K, target_top_p=TOP_P)
    assert not torch.equal(a.tokens, b.tokens)
