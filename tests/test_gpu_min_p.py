"""Min-p behind top-k and top-p: asd_draft_sample_min_p, asd_verify_accept_min_p and asd_residual_sample_lp_min_p
(include/asd_hip.h).  Bars:
  - top-k and top-p off: the threshold is np.float32(x_max) + np.float32(delta) exactly, min_p = 1 gives x_max; with top-k 50 /
    top-p 0.9 on it is max(asd_draft_sample_top_k's threshold, x_mp) exactly, and each side wins on some row;
  - the draft's threshold, the verify's t_nucleus_logit and the bonus row's threshold are one select: the same bits, and so are
    the draft's lp and the verify's lp_target for the token drawn;
  - against the f64 oracle on rows stored with -inf below the threshold (the bars of tests/test_gpu_top_k.py): lp within 1e-5,
    accept / n_acc away from the decision margin, tokens away from CDF edges, at most 2 % of the rows inside a margin;
  - min_p = 0 returns the bits of the top-k entry points; one lossless route through tests/lossless.py.
Shapes: V = 1000 (less than one sweep, ragged last tile), 1025 vectors (a second sweep trip with one live thread), and one pass
at the full vocabulary; 7 rows, K = 3."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import lossless as L
from tests.helpers import encode_logits, make_verify_case, to_device_logits
from tests.min_p_ref import combine, min_p_delta, x_mp_of
from tests.test_gpu_top_k import INV_T, TOP_K, TOP_P, V_FULL, _dev_rows, _draft, _leading_finite, _masked

pytestmark = pytest.mark.gpu

B, K = 7, 3
SMALL = [(O.DT_BF16, 1000), (O.DT_F16, 1000), (O.DT_F32, 1000), (O.DT_BF16, 8200), (O.DT_F16, 8200), (O.DT_F32, 4100)]
SHAPES = SMALL + [(O.DT_BF16, V_FULL)]
SETTINGS = ((0, 1.0, 0.1), (TOP_K, TOP_P, 0.3), (TOP_K, TOP_P, 1e-6))        # (top_k, top_p, min_p)


@pytest.fixture(scope="module")
def K_():
    from asd_amd import kernels
    return kernels


def rows_of_every_kind(V, dtype, seed):
    """7 rows: Gaussian, near-constant, a coarse grid (many ties), all-equal, with -inf entries, the maximum repeated, peaked."""
    rng = np.random.default_rng(seed)
    rows = [rng.standard_normal(V) * 3.0, rng.standard_normal(V) * 0.01 - 5.0, np.round(rng.standard_normal(V) * 2.0) / 2.0,
            np.full(V, 1.25)]
    r = rng.standard_normal(V) * 2.0
    r[rng.uniform(size=V) < 0.3] = -np.inf
    rows.append(r)
    r = rng.standard_normal(V) * 3.0
    r[rng.choice(V, 5, replace=False)] = r.max()
    rows.append(r)
    rows.append(rng.standard_normal(V) * 6.0)
    store = encode_logits(np.stack(rows).astype(np.float32), dtype)
    return store, O.logits_as_f32(store, dtype)


def _draft_mp(K_, store, dtype, R, V, r, top_k, top_p, min_p, inv_t=INV_T):
    import torch
    lg = _dev_rows(store, dtype, R, V)
    d = K_.DraftSampler(R, V, lg.dtype).min_p(lg, torch.from_numpy(np.asarray(r, np.float32)).cuda(), inv_t, min_p=min_p,
                                              top_k=top_k, top_p=top_p)
    torch.cuda.synchronize()
    return d.tok.cpu().numpy(), d.lp.cpu().numpy(), d.thr.cpu().numpy()


def _verify_mp(K_, lg3, tok, lp_d, u, top_k, top_p, min_p, ws=None):
    import torch
    res = K_.verify_accept_min_p(lg3, torch.from_numpy(tok).cuda(), torch.from_numpy(lp_d).cuda(), torch.from_numpy(u).cuda(), ws,
                                 inv_temperature=INV_T, top_k=top_k, top_p=top_p, min_p=min_p)
    torch.cuda.synchronize()
    return {k: getattr(res, k).cpu().numpy() for k in ("lp_target", "accept", "n_acc", "accept_bits", "t_nucleus_logit", "n_finite")}


@pytest.mark.parametrize("dtype,V", SHAPES)
def test_threshold_is_exact(K_, dtype, V):
    store, x = rows_of_every_kind(V, dtype, seed=V + dtype)
    R = x.shape[0]
    r = np.random.default_rng(V).uniform(0, 1, R).astype(np.float32)
    x_max = x.max(axis=1)
    for min_p in (1.0, 0.3, 0.05, 1e-4):
        tok, lp, thr = _draft_mp(K_, store, dtype, R, V, r, 0, 1.0, min_p)
        want = x_max + min_p_delta(min_p, INV_T)                              # one f32 addition
        assert want.dtype == np.float32 and thr.tobytes() == want.tobytes(), (min_p, thr, want)
        assert ((x >= thr[:, None]).sum(1) == (x >= want[:, None]).sum(1)).all()
        if min_p == 1.0:
            assert np.array_equal(thr, x_max)
        assert (tok >= 0).all() and (x[np.arange(R), tok] >= thr).all() and np.isfinite(lp).all()
    _, _, thr_kp = _draft(K_, store, dtype, R, V, r, TOP_K, TOP_P)
    won = np.zeros(2, int)
    for min_p in (0.5, 1e-6):
        tok, lp, thr = _draft_mp(K_, store, dtype, R, V, r, TOP_K, TOP_P, min_p)
        want, mp_won = combine(thr_kp, x_mp_of(x, min_p, INV_T))
        assert thr.tobytes() == want.tobytes(), (min_p, thr, want)
        assert (x[np.arange(R), tok] >= thr).all() and np.isfinite(lp).all()
        won += [int(mp_won.sum()), int((~mp_won).sum())]
    assert (won > 0).all(), won                                               # each side of the max won on some row


@pytest.mark.parametrize("dtype,V", SHAPES)
def test_one_select_for_draft_verify_and_bonus(K_, dtype, V):
    import torch
    store, x = rows_of_every_kind(V, dtype, seed=3 * V + dtype)
    R = x.shape[0]
    r = np.random.default_rng(V + 1).uniform(0, 1, R).astype(np.float32)
    lg = _dev_rows(store, dtype, R, V).contiguous()
    from asd_amd import _binding
    base = int(_binding.load_library().asd_residual_sample_workspace_bytes(R, V, dtype))
    for top_k, top_p, min_p in SETTINGS:
        tok, lp, thr = _draft_mp(K_, store, dtype, R, V, r, top_k, top_p, min_p)
        got = _verify_mp(K_, lg.view(R, 1, V), tok.reshape(R, 1), np.zeros((R, 1), np.float32), np.full((R, 1), 0.5, np.float32),
                         top_k, top_p, min_p)
        assert got["t_nucleus_logit"].reshape(-1).tobytes() == thr.tobytes()
        assert got["lp_target"].reshape(-1).tobytes() == lp.tobytes()
        assert (got["n_finite"] == 1).all()
        # the bonus rows: n_acc = K = 1 draws from each row's own kept set with the same r; their thresholds are the [R] floats
        # behind the part of the workspace asd_residual_sample_workspace_bytes sizes
        rs = K_.ResidualSampler(R, V, lg.dtype)
        t3 = lg.view(R, 1, V)
        btok, blp = rs.lp_min_p(t3, t3, torch.ones(R, dtype=torch.int32, device="cuda"), torch.from_numpy(r).cuda(), lg, INV_T,
                                top_k=top_k, top_p=top_p, min_p=min_p, t_threshold=torch.from_numpy(thr).cuda().view(R, 1))
        torch.cuda.synchronize()
        assert rs.status() == 0
        assert rs.buf[base:base + 4 * R].cpu().numpy().view(np.float32).tobytes() == thr.tobytes()
        btok, blp = btok.cpu().numpy(), blp.cpu().numpy()
        ref = O.draft_sample(_masked(store, dtype, V, thr), dtype, r, R, V, INV_T, 1.0)
        # (the threshold bits are compared above on every row.  The tokens of two different float summations can only be compared
        # away from CDF edges; on the near-constant and all-equal rows of the full vocabulary every token holds 6.6e-6 of the
        # mass, less than the 1e-5 margin, so those rows have no such draw: the 2 % cap belongs to the Gaussian rows of
        # test_against_the_oracle_on_masked_rows)
        far = ref["margin_r"] > 1e-5
        assert far.sum() >= 5
        assert np.array_equal(btok[far], tok[far]), (top_k, min_p)
        # the commit draw forms its normaliser with its own (slice) sums: the same value to f32 rounding, 1e-5 as against f64
        same = btok == tok
        np.testing.assert_allclose(blp[same], lp[same], atol=1e-5, rtol=0)


def _plan(dtype, V, top_k, top_p, min_p):
    """The verify case and the residual inputs of the oracle tests (numpy only)."""
    case = make_verify_case(B, K, V, dtype, seed=900 + V % 1000 + dtype, ld_row=V + 64)
    rng = np.random.default_rng(1700 + V % 1000 + dtype)
    xt = O.logits_as_f32(case["logits"][:, :V], dtype)
    xd = (xt + rng.standard_normal((B * K, V)).astype(np.float32) * 0.7).astype(np.float32)
    xb = (rng.standard_normal((B, V)) * 3.0).astype(np.float32)
    n_acc = rng.integers(0, K + 1, B).astype(np.int32)
    n_acc[:3] = [0, K, 1]
    xd[2 * K + 1] = xt[2 * K + 1]                                             # sequence 2 rejects at j = 1 with an empty residual
    return case, encode_logits(xd, dtype), encode_logits(xb, dtype), n_acc, rng.uniform(0, 1, B).astype(np.float32)


@pytest.mark.parametrize("top_k,top_p,min_p", SETTINGS)
@pytest.mark.parametrize("dtype,V", SHAPES)
def test_against_the_oracle_on_masked_rows(K_, dtype, V, top_k, top_p, min_p):
    import torch
    case, sd, sb, n_acc, r = _plan(dtype, V, top_k, top_p, min_p)
    st, ld = case["logits"], case["ld"]
    R = B * K
    # ---- the draft draw on the target rows
    rr = np.random.default_rng(V + 5).uniform(0, 1, R).astype(np.float32)
    lg = to_device_logits(st, dtype).view(R, ld)[:, :V]
    d = K_.DraftSampler(R, V, lg.dtype).min_p(lg, torch.from_numpy(rr).cuda(), INV_T, min_p=min_p, top_k=top_k, top_p=top_p)
    tok, lp, tthr = d.tok.cpu().numpy(), d.lp.cpu().numpy(), d.thr.cpu().numpy()
    ref = O.draft_sample(_masked(st, dtype, V, tthr), dtype, rr, R, V, INV_T, 1.0, ld_row=ld)
    np.testing.assert_allclose(lp, ref["lp"], atol=1e-5, rtol=0)
    far = ref["margin_r"] > 1e-5
    assert far.mean() >= 0.98 and np.array_equal(tok[far], ref["tok"][far])
    # ---- the verify
    got = _verify_mp(K_, lg.as_strided((B, K, V), (K * ld, ld, 1)), case["tok"], case["lp_d"], case["u"], top_k, top_p, min_p)
    assert got["t_nucleus_logit"].reshape(-1).tobytes() == tthr.tobytes()
    want = O.verify_accept(_masked(st, dtype, V, tthr), dtype, case["tok"], case["lp_d"], case["u"], B, K, V, ld_row=ld,
                           n_threads=8, inv_temperature=INV_T)
    lpt, wlp = got["lp_target"], want["lp_t"]
    fin = np.isfinite(wlp)
    assert (np.isfinite(lpt) == fin).all() and fin.any()
    np.testing.assert_allclose(lpt[fin], wlp[fin], atol=1e-5, rtol=0)
    assert (got["n_finite"] == _leading_finite(wlp)).all() and (got["n_acc"] <= got["n_finite"]).all()
    safe = want["margin"] > 1e-5
    assert safe.mean() >= 0.98
    assert (got["accept"][safe] == want["accept"][safe]).all()
    seq_safe = safe.all(axis=1)
    assert (got["n_acc"][seq_safe] == want["n_acc"][seq_safe]).all()
    inv = ~got["accept"].astype(bool)
    assert (got["n_acc"] == np.where(inv.any(axis=1), np.argmax(inv, axis=1), K)).all()
    # ---- the commit draw and its log-prob
    half = np.full(R, 0.5, np.float32)
    _, _, dthr = _draft_mp(K_, sd, dtype, R, V, half, top_k, top_p, min_p)
    _, _, bthr = _draft_mp(K_, sb, dtype, B, V, half[:B], top_k, top_p, min_p)
    t3 = lg.as_strided((B, K, V), (K * ld, ld, 1))
    d3 = to_device_logits(sd, dtype).view(B, K, V)
    bon = to_device_logits(sb, dtype).view(B, V)
    rs = K_.ResidualSampler(B, V, lg.dtype)
    ctok, clp = rs.lp_min_p(t3, d3, torch.from_numpy(n_acc).cuda(), torch.from_numpy(r).cuda(), bon, INV_T, top_k=top_k,
                            top_p=top_p, min_p=min_p, t_threshold=torch.from_numpy(tthr).cuda().view(B, K),
                            d_threshold=torch.from_numpy(dthr).cuda().view(B, K))
    torch.cuda.synchronize()
    assert rs.status() == 0
    ctok, clp = ctok.cpu().numpy(), clp.cpu().numpy()
    wtok, margin = O.residual_sample(_masked(st[:, :V].copy(), dtype, V, tthr), _masked(sd, dtype, V, dthr), dtype, n_acc, r, B, K, V,
                                     bonus=_masked(sb, dtype, V, bthr), inv_temperature=INV_T)
    safe = margin > 1e-5
    assert safe.mean() >= 0.98 and np.array_equal(ctok[safe], wtok[safe])
    from tests.stage_scenario import ref_logprob
    xtf, xbf = O.logits_as_f32(st[:, :V], dtype), O.logits_as_f32(sb, dtype)
    for b in range(B):
        j = n_acc[b]
        row, thr = (xtf[b * K + j], tthr[b * K + j]) if j < K else (xbf[b], bthr[b])
        assert row[ctok[b]] >= thr
        assert abs(float(clp[b]) - ref_logprob(row, ctok[b], INV_T, thr)) <= 1e-5


@pytest.mark.parametrize("dtype,V", [(O.DT_BF16, 1000), (O.DT_F32, 4100), (O.DT_BF16, V_FULL)])
def test_off_switch_is_bit_identical_to_the_top_k_entry_points(K_, dtype, V):
    import torch
    case, sd, sb, n_acc, r = _plan(dtype, V, 0, 1.0, 0.0)
    ld, R = case["ld"], B * K
    lg = to_device_logits(case["logits"], dtype).view(R, ld)[:, :V]
    t3 = lg.as_strided((B, K, V), (K * ld, ld, 1))
    d3, bon = to_device_logits(sd, dtype).view(B, K, V), to_device_logits(sb, dtype).view(B, V)
    rr = torch.from_numpy(np.random.default_rng(1).uniform(0, 1, R).astype(np.float32)).cuda()
    ds, rs = K_.DraftSampler(R, V, lg.dtype), K_.ResidualSampler(B, V, lg.dtype)
    ws = K_.VerifyWorkspace(B, K, V, lg.dtype)
    tk, lpd, u = (torch.from_numpy(case[k]).cuda() for k in ("tok", "lp_d", "u"))
    na, rc = torch.from_numpy(n_acc).cuda(), torch.from_numpy(r).cuda()
    bits = lambda *ts: [t.cpu().numpy().tobytes() for t in ts]
    for top_k, top_p in ((TOP_K, TOP_P), (0, TOP_P), (TOP_K, 1.0), (0, 1.0)):
        a = ds.top_k(lg, rr, INV_T, top_k=top_k, top_p=top_p)
        va = K_.verify_accept_top_k(t3, tk, lpd, u, ws, inv_temperature=INV_T, top_k=top_k, top_p=top_p)
        dthr = a.thr.view(B, K)
        ra = rs.lp(t3, d3, na, rc, bon, INV_T, top_k=top_k, top_p=top_p, t_threshold=va.t_nucleus_logit, d_threshold=dthr)
        want = bits(a.tok, a.lp, a.thr), bits(va.lp_target, va.accept, va.n_acc, va.accept_bits, va.t_nucleus_logit, va.n_finite), \
            bits(*ra)
        for off in (0.0, -1.0):
            b = ds.min_p(lg, rr, INV_T, min_p=off, top_k=top_k, top_p=top_p)
            vb = K_.verify_accept_min_p(t3, tk, lpd, u, ws, inv_temperature=INV_T, top_k=top_k, top_p=top_p, min_p=off)
            rb = rs.lp_min_p(t3, d3, na, rc, bon, INV_T, top_k=top_k, top_p=top_p, min_p=off, t_threshold=va.t_nucleus_logit,
                             d_threshold=dthr)
            got = bits(b.tok, b.lp, b.thr), bits(vb.lp_target, vb.accept, vb.n_acc, vb.accept_bits, vb.t_nucleus_logit, vb.n_finite), \
                bits(*rb)
            assert got == want, (top_k, top_p, off)
    torch.cuda.synchronize()
    assert ds.status() == 0 and rs.status() == 0 and ws.status() == 0


# ---------------------------------------------------------------------------------------------------------- losslessness
MIN_P_ROUTE = L.Route("m", 0, 0.9, 0, 1.0, "min_p")        # draft: top-p 0.9; target: min-p 0.1 alone
TARGET_MIN_P = 0.1
N_CALLS = 25                                               # 4096 x 25 sequences: ~1e5 (lossless.SMALL runs 50 calls)


def min_p_reference(xt, xd):
    """lossless.reference with the target rows cut by the new reference: softmax over { x >= x_max + delta } in f64."""
    ref = L.reference(xt, xd, MIN_P_ROUTE)
    p_t = np.empty_like(ref.p_t)
    R, K1, _ = xt.shape
    for c in range(R):
        thr = x_mp_of(xt[c], TARGET_MIN_P, L.INV_T)
        for j in range(K1):
            masked = np.where(xt[c, j] >= thr[j], xt[c, j], -np.inf).astype(np.float32)
            p_t[c, j] = L.target_distribution(masked, L.INV_T, 0, 1.0)[0]
    return L.Reference(p_t, ref.p_d, np.minimum(p_t[:, :-1], ref.p_d).sum(-1), ref.gap)


def test_lossless_with_target_min_p(K_):
    import torch
    from tests.test_gpu_lossless import DRAW_SEED, PAD, ROW_SEED, HipChain, TorchOps
    geom = L.SMALL
    xt, xd = L.make_rows(geom, "bf16", ROW_SEED)
    ref = min_p_reference(xt, xd)
    assert ((ref.p_t > 0).sum(-1) < geom.V).all()                            # min-p cuts every target row
    n_c = geom.B * N_CALLS // L.R_CLASSES
    reach = L.expected_reach(ref)
    # The expected counts clear MIN_BINS wherever the distribution has that many tokens to offer.  A min-p 0.1 set of these rows
    # holds 9 ... 39 tokens: like a draft cut to top-k 20 (lossless.draft_min_bins) such a histogram must keep EVERY token of
    # its support unpooled, the most the distribution allows.
    for c in range(L.R_CLASSES):
        for j in range(geom.K + 1):
            L._structure(ref.p_t[c, j], reach[c, j] * n_c * 0.97, L.draft_min_bins(ref.p_t[c, j]), ("target", c, j))
            assert L.draft_min_bins(ref.p_t[c, j]) >= 9
    chain = HipChain(K_, geom, L.ROUTES["b"], "bf16", xt, xd)                # the draft side of route b: top-p 0.9

    def verify(tok, lp_d, u):
        v = K_.verify_accept_min_p(chain.t3, tok.view(chain.B, chain.K), lp_d.view(chain.B, chain.K), torch.from_numpy(u).cuda(),
                                   None, inv_temperature=L.INV_T, min_p=TARGET_MIN_P)
        return v.n_acc, v.t_nucleus_logit

    def residual(n_acc, r, d_thr, t_thr):
        return chain.rs.lp_min_p(chain.t3, chain.d3, n_acc, torch.from_numpy(r).cuda(), chain.bonus, L.INV_T, min_p=TARGET_MIN_P,
                                 t_threshold=t_thr, d_threshold=d_thr)[0]
    chain.verify, chain.residual = verify, residual
    counts = L.run_chain(chain, geom, DRAW_SEED, geom.V + PAD + 1, xp=TorchOps, n_calls=N_CALLS)
    torch.cuda.synchronize()
    assert chain.ds.status() == 0 and chain.rs.status() == 0
    assert counts.n_seq == geom.B * N_CALLS
    got_reach = counts.commit.sum(-1)
    worst = 0.0
    for c in range(L.R_CLASSES):
        for j in range(geom.K + 1):
            chi2, crit, _ = L.check_histogram(counts.commit[c, j], ref.p_t[c, j], got_reach[c, j], L.draft_min_bins(ref.p_t[c, j]))
            worst = max(worst, chi2 / crit)
            if j < geom.K:
                L.check_histogram(counts.draft[c, j], ref.p_d[c, j], n_c, L.draft_min_bins(ref.p_d[c, j]))
                L.check_accept_count(int(got_reach[c, j + 1]), int(got_reach[c, j]), float(ref.rate[c, j]))
    print(f"[lossless] target min-p 0.1: worst commit chi2 / critical {worst:.3f}")
