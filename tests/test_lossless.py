"""Statistical losslessness of the oracle's draft / verify / commit chain (CPU), and the case tables of the GPU test.

The chain of tests/lossless.py runs through oracle.oracle -- draft_sample, verify_accept, residual_sample, with the masked-row
recipe of tests/test_top_k.py for truncated targets -- on about 2e5 sequences per route, and every committed-token histogram
is held to tests/lossless.target_distribution, which shares no code with the oracle.  This is the first check of the
SPECIFICATION both the oracle and the kernels were written from: six negative controls, each one
defect in the Python glue around the same oracle calls, must fail at the same number of sequences."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from tests import lossless as L  # noqa: E402
from tests.helpers import encode_logits  # noqa: E402

DT = {"f32": O.DT_F32, "bf16": O.DT_BF16, "f16": O.DT_F16}
NEG_INF_STORE = {O.DT_F32: np.float32(-np.inf), O.DT_BF16: np.uint16(0xFF80), O.DT_F16: np.uint16(0xFC00)}
ROW_SEED, DRAW_SEED = 1, 2024
CASES = [("a", "bf16"), ("b", "bf16"), ("c", "bf16"), ("d", "bf16"), ("e", "bf16"), ("a", "f32"), ("d", "f32"), ("a", "f16"),
         ("d", "f16")]
_POOL = ThreadPoolExecutor(8)


def _masked(store, dt, thr):
    """Storage rows with every score below the row's threshold replaced by -inf."""
    out = store.copy()
    out[O.logits_as_f32(store, dt) < np.asarray(thr, np.float32).reshape(-1, 1)] = NEG_INF_STORE[dt]
    return out


def _x_k(rows_f32, top_k):
    """tests/test_top_k.py::x_k_of: the top_k-th largest value counting multiplicity; -inf for a short row or top-k off."""
    Vr = rows_f32.shape[-1]
    if top_k <= 0 or top_k >= Vr:
        return np.full(rows_f32.shape[0], -np.inf, np.float32)
    kth = np.partition(rows_f32, Vr - top_k, axis=-1)[:, Vr - top_k]
    return np.where((rows_f32 > -np.inf).sum(-1) >= top_k, kth, -np.inf).astype(np.float32)


def oracle_thresholds(store, dt, top_k, top_p):
    """max(x_k, x*_K) of every storage row: x*_K is the oracle's nucleus threshold of the row masked below x_k."""
    R, V = store.shape
    x_k = _x_k(O.logits_as_f32(store, dt), top_k)
    if not 0.0 < top_p < 1.0:
        return x_k
    thr = O.draft_sample(_masked(store, dt, x_k), dt, np.full(R, 0.5, np.float32), R, V, L.INV_T, top_p)["thr"]
    return np.maximum(x_k, thr).astype(np.float32)


def _chunks(n, parts=8):
    edges = np.linspace(0, n, parts + 1).astype(int)
    return [(a, b) for a, b in zip(edges[:-1], edges[1:]) if b > a]


class OracleChain:
    """The backend of lossless.run_chain over oracle.oracle.  `defect` injects one error into the glue (the controls)."""

    def __init__(self, geom, route, dtype, xt, xd, defect=None):
        self.g, self.route, self.dt, self.defect = geom, route, DT[dtype], defect
        R, K, V, B = L.R_CLASSES, geom.K, geom.V, geom.B
        self.B, self.K, self.V = B, K, V
        cls = np.arange(B) % R
        st = encode_logits(xt.reshape(R * (K + 1), V), self.dt).reshape(R, K + 1, V)
        sd = encode_logits(xd.reshape(R * K, V), self.dt).reshape(R, K, V)
        self.st = np.ascontiguousarray(st[cls, :K]).reshape(B * K, V)        # row b * K + j: class b % R, position j
        self.sd = np.ascontiguousarray(sd[cls]).reshape(B * K, V)
        self.sb = np.ascontiguousarray(st[cls, K])
        t_thr = oracle_thresholds(st.reshape(-1, V), self.dt, route.t_top_k, route.t_top_p).reshape(R, K + 1)
        self.t_thr = np.ascontiguousarray(t_thr[cls, :K])                      # [B, K]
        self.st_masked = _masked(self.st, self.dt, self.t_thr.reshape(-1))
        self.sb_masked = _masked(self.sb, self.dt, t_thr[cls, K])
        d_xk = _x_k(O.logits_as_f32(sd.reshape(-1, V), self.dt), route.d_top_k).reshape(R, K)
        self.sd_masked = _masked(self.sd, self.dt, d_xk[cls].reshape(-1))      # top-k off: the rows themselves
        self.d_xk = np.ascontiguousarray(d_xk[cls]).reshape(-1)

    def draft(self, r):
        """The oracle's draw: top-p by O.draft_sample itself, top-k by masking the row below x_k first."""
        def part(ab):
            a, b = ab
            return O.draft_sample(self.sd_masked[a:b], self.dt, r[a:b], b - a, self.V, L.INV_T, self.route.d_top_p)
        out = list(_POOL.map(part, _chunks(self.B * self.K)))
        tok = np.concatenate([o["tok"] for o in out])
        lp = np.concatenate([o["lp"] for o in out]).astype(np.float32)
        thr = np.maximum(np.concatenate([o["thr"] for o in out]), self.d_xk)
        if self.defect == "lp_of_untruncated_draft":
            def full(ab):
                a, b = ab
                x = O.logits_as_f32(self.sd[a:b], self.dt).astype(np.float64) * L.INV_T
                lse = np.log(np.exp(x - x.max(1, keepdims=True)).sum(1)) + x.max(1)
                return x[np.arange(b - a), tok[a:b]] - lse
            lp = np.concatenate(list(_POOL.map(full, _chunks(self.B * self.K)))).astype(np.float32)
        truncated = self.route.d_top_k > 0 or self.route.d_top_p < 1.0
        return tok, lp, (thr.reshape(self.B, self.K) if truncated else None)

    def verify(self, tok, lp_d, u):
        v = O.verify_accept(self.st_masked, self.dt, tok, lp_d, u, self.B, self.K, self.V, n_threads=8, inv_temperature=L.INV_T)
        truncated = self.route.t_top_k > 0 or self.route.t_top_p < 1.0
        return v["n_acc"], (self.t_thr if truncated else None)

    def residual(self, n_acc, r, d_thr, t_thr):
        B, K = self.B, self.K
        st, sb = self.st_masked, self.sb_masked
        if self.defect == "no_d_threshold":
            d_thr = None
        if self.defect == "no_t_threshold":
            st, sb = self.st, self.sb
        if self.defect == "t_threshold_of_row_j_minus_1":
            shifted = np.concatenate([t_thr[:, :1], t_thr[:, :-1]], axis=1)
            st = _masked(self.st, self.dt, shifted.reshape(-1))
        if self.defect == "commit_reads_n_acc_plus_1":
            n_acc = np.minimum(n_acc + 1, K).astype(np.int32)
        sd = self.sd
        if self.defect == "redraw_from_p_t":           # the rejected position is drawn from the target row itself
            sb = np.where((n_acc < K)[:, None], st.reshape(B, K, -1)[np.arange(B), np.minimum(n_acc, K - 1)], sb)
            n_acc = np.full(B, K, np.int32)

        def part(ab):
            a, b = ab
            return O.residual_sample(st[a * K:b * K], sd[a * K:b * K], self.dt, n_acc[a:b], r[a:b], b - a, K, self.V, bonus=sb[a:b],
                                     inv_temperature=L.INV_T, d_threshold=None if d_thr is None else d_thr[a:b])[0]
        return np.concatenate(list(_POOL.map(part, _chunks(B))))


def _run(route_name, dtype, defect=None):
    route = L.ROUTES[route_name]
    xt, xd = L.make_rows(L.SMALL, dtype, ROW_SEED)
    ref = L.reference(xt, xd, route)
    counts = L.run_chain(OracleChain(L.SMALL, route, dtype, xt, xd, defect), L.SMALL, DRAW_SEED, L.SMALL.V + 1)
    return L.evaluate(counts, ref), counts


# ------------------------------------------------------------------------------------------------ the shared pieces
def test_chi2_critical_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    for df in list(range(5, 60)) + list(range(60, 501, 10)):
        want = float(stats.chi2.isf(1e-6, df))
        assert abs(L.chi2_critical(df, 1e-6) - want) / want < 0.02, df
    assert abs(L.normal_isf(1e-6) - float(stats.norm.isf(1e-6))) < 1e-9


def test_target_distribution_top_k_ties_and_short_rows():
    x = np.array([3.0, 1.0, 3.0, 2.0, 2.0, -np.inf, 0.5], np.float32)
    p, thr, gap = L.target_distribution(x, 1.0, 3, 1.0)
    assert thr == 2.0 and (p > 0).tolist() == [True, False, True, True, True, False, False]      # both ties at x_k kept
    e = np.exp(np.array([3.0, 3.0, 2.0, 2.0]))
    np.testing.assert_allclose(p[[0, 2, 3, 4]], e / e.sum(), rtol=1e-14)
    assert gap == np.inf and abs(p.sum() - 1.0) < 1e-14
    short = np.array([1.0, -np.inf, 0.0, -np.inf, -np.inf], np.float32)
    p, thr, _ = L.target_distribution(short, 1.0, 3, 1.0)                   # fewer than k values > -inf: kept whole
    assert thr == -np.inf and (p > 0).tolist() == [True, False, True, False, False]


def test_target_distribution_top_p_cut_and_ties():
    # masses 0.4, 0.2, 0.2, 0.1, 0.1: top_p 0.5 cuts inside the tie at 0.2 -> both kept; the gaps are to 0.8 and to 0.4
    x = np.log(np.array([0.4, 0.2, 0.1, 0.2, 0.1])).astype(np.float32)
    p, thr, gap = L.target_distribution(x, 1.0, 0, 0.5)
    assert thr == x[1] and (p > 0).tolist() == [True, True, False, True, False]
    np.testing.assert_allclose(p[[0, 1, 3]], [0.5, 0.25, 0.25], rtol=1e-6)
    assert abs(gap - 0.1) < 1e-6
    p, thr, gap = L.target_distribution(x, 1.0, 0, 0.85)                    # the whole row: the last upper set
    assert thr == x[2] and (p > 0).all() and abs(gap - 0.05) < 1e-6
    # the temperature is applied before the cut: at T = 0.5 the same row is 16 : 4 : 1 : 4 : 1
    p, thr, _ = L.target_distribution(x, 2.0, 0, 0.7)
    assert (p > 0).tolist() == [True, True, False, True, False]
    # top-k first, top-p over the kept set renormalised: top-2 (with the tie: 3 tokens, 0.5 / 0.25 / 0.25), then 0.5 -> one
    p, thr, _ = L.target_distribution(x, 1.0, 2, 0.5)
    assert (p > 0).tolist() == [True, False, False, False, False] and thr == x[0]


def test_target_distribution_no_ops():
    x = (np.random.default_rng(0).standard_normal(40) * 2).astype(np.float32)
    base, thr, gap = L.target_distribution(x, L.INV_T, 0, 1.0)
    assert thr == -np.inf and gap == np.inf
    z = x.astype(np.float64) * L.INV_T
    np.testing.assert_allclose(base, np.exp(z - z.max()) / np.exp(z - z.max()).sum(), rtol=1e-14)
    for top_k, top_p in ((0, 1.0), (-3, 1.0), (40, 1.5), (41, 1.0), (0, 0.0), (0, -1.0)):
        p, thr, _ = L.target_distribution(x, L.INV_T, top_k, top_p)
        assert thr == -np.inf and np.array_equal(p, base), (top_k, top_p)


def test_target_distribution_keeps_hf_top_p_sets(golden):
    """tests/golden/top_p_nucleus.npz (transformers' TemperatureLogitsWarper + TopPLogitsWarper): the same threshold and the
    same number of kept tokens (plus the ties the warper's sort dropped) wherever the warper's f32 cut is unambiguous."""
    from tests.helpers import nucleus_cases
    n = 0
    for c in nucleus_cases(golden.npz("top_p_nucleus.npz")):
        if c["margin"] <= 1e-5:
            continue
        p, thr, gap = L.target_distribution(c["x"], float(np.float32(1.0) / np.float32(c["T"])), 0, c["top_p"])
        assert thr == c["thr"], (c["row"], thr, c["thr"])
        assert int((p > 0).sum()) == c["n_keep"] + c["ties_removed"] == int((c["x"] >= thr).sum())
        n += 1
    assert n >= 20


def test_target_distribution_keeps_hf_top_k_sets(golden):
    """tests/golden/speculative_sampling_top_k.npz (Temperature -> TopK -> TopP by transformers' warpers, V = 152064): x_k, the
    combined threshold and the kept-set size of every candidate and target row, up to two rows whose f32 cumulative sum in
    the warper sits on a mass step (the allowance tests/test_gpu_top_k.py gives the kernels on the same rows)."""
    from tests.helpers import spec_full_cases
    g = golden.npz("speculative_sampling_top_k.npz")
    compared = off = 0
    for ci, c in enumerate(spec_full_cases(g)):
        top_k, top_p = int(g["case_top_k"][ci]), float(g["case_top_p"][ci])
        a, b = int(g["off"][ci]), int(g["off"][ci + 1])
        t0, t1 = int(g["t_off"][ci]), int(g["t_off"][ci + 1])
        for store, hf_xk, hf_thr, hf_keep, hf_ties in (
                (c["cand"], g["x_k"][a:b], g["thr"][a:b], g["n_keep"][a:b], g["ties_removed"][a:b]),
                (c["new"], g["t_x_k"][t0:t1], g["t_thr"][t0:t1], g["t_n_keep"][t0:t1], g["t_ties_removed"][t0:t1])):
            x = O.logits_as_f32(store, c["dtype"])
            for i in range(x.shape[0]):
                _, xk, _ = L.target_distribution(x[i], c["inv_t"], top_k, 1.0)
                assert xk == hf_xk[i]
                p, thr, gap = L.target_distribution(x[i], c["inv_t"], top_k, top_p)
                compared += 1
                if thr != hf_thr[i]:
                    off += 1
                    assert gap < 1e-5, (c["case"], i, gap)
                else:
                    assert int((p > 0).sum()) == int(hf_keep[i] + hf_ties[i])
    assert compared >= 200 and off <= 2, off


def test_check_histogram_conditions():
    p = np.full(40, 1.0 / 40)
    rng = np.random.default_rng(5)
    counts = np.bincount(rng.choice(40, 4000, p=p), minlength=44)          # (slots past the vocabulary stay empty)
    chi2, crit, df = L.check_histogram(counts, p, 4000)
    assert df == 39 and chi2 < crit
    bad = counts.copy()
    bad[41] += 1
    with pytest.raises(L.HistogramError, match="support"):
        L.check_histogram(bad, p, 4001)
    with pytest.raises(L.HistogramError, match="structure"):               # expected 10 per bin: every bin pooled
        L.check_histogram(np.bincount(rng.choice(40, 400, p=p), minlength=40), p, 400)
    q = np.r_[np.full(30, 0.8 / 30), np.full(2000, 0.2 / 2000)]            # 20 % of the mass in bins too small to test
    with pytest.raises(L.HistogramError, match="pooled"):
        L.check_histogram(np.bincount(rng.choice(2030, 4000, p=q), minlength=2030), q, 4000)
    skew = p.copy()
    skew[:20] *= 1.2
    skew[20:] *= 0.8
    with pytest.raises(L.HistogramError, match="chi2"):
        L.check_histogram(np.bincount(rng.choice(40, 4000, p=skew), minlength=40), p, 4000)
    with pytest.raises(L.HistogramError, match="accept"):
        L.check_accept_count(5300, 10000, 0.5)
    assert L.check_accept_count(5100, 10000, 0.5)[0] == pytest.approx(2.0)


# ------------------------------------------------------------------------------------------------ the cases, reference alone
@pytest.mark.parametrize("geom,cases", [(L.SMALL, CASES), (L.FULL, [("c", "bf16"), ("d", "bf16"), ("e", "bf16")])],
                         ids=["V512", "V152064"])
def test_case_tables_meet_the_input_conditions(geom, cases):
    """Accept rates in [0.3, 0.9], the bonus position reached by >= 15 %, >= 30 unpooled bins and <= 10 % pooled mass in every
    histogram, and every top-p cut >= 1e-4 of mass away from a step -- for both geometries the GPU test runs."""
    rows = {}
    for route_name, dtype in cases:
        if dtype not in rows:
            rows[dtype] = L.make_rows(geom, dtype, ROW_SEED)
        xt, xd = rows[dtype]
        route = L.ROUTES[route_name]
        ref = L.reference(xt, xd, route)
        L.check_inputs(ref, route, geom.B * geom.n_calls // L.R_CLASSES)
        # the draft's support is not the target's, and where both are cut by top-p it is not inside it in every row either
        # (a top-20 draft set does lie inside the target's top-50 set at this draft noise)
        st, sd = ref.p_t[:, :-1] > 0, ref.p_d > 0
        if route_name in "bcde":
            assert (st & ~sd).any(-1).all()
        if route_name in "cd":
            assert (sd & ~st).any(-1).sum() >= 4
    assert geom.B * geom.n_calls >= (2e5 if geom is L.SMALL else 9e4)


# ------------------------------------------------------------------------------------------------ the oracle chain
@pytest.mark.parametrize("route_name,dtype", CASES)
def test_oracle_chain_is_lossless(route_name, dtype):
    findings, counts = _run(route_name, dtype)
    assert counts.n_seq >= 200000
    L.assert_lossless(findings, f"oracle chain, route {route_name} {dtype}")


CONTROLS = [("no_d_threshold", "b"), ("no_t_threshold", "c"), ("commit_reads_n_acc_plus_1", "a"), ("redraw_from_p_t", "a"),
            ("lp_of_untruncated_draft", "c"), ("t_threshold_of_row_j_minus_1", "d")]


@pytest.mark.parametrize("defect,route_name", CONTROLS)
def test_negative_controls_fail(defect, route_name):
    """One defect in the glue, the same cases and the same number of sequences: the statistical checks must notice (a failure
    of the test's own structural conditions does not count)."""
    findings, _ = _run(route_name, "bf16", defect)
    bad = L.failures(findings, statistical_only=True)
    print(f"[lossless] control {defect} on route {route_name}: {len(bad)} checks failed; "
          + " | ".join(f"{f.what} class {f.cls} j {f.j}: {f.error}" for f in bad[:3]))
    assert bad, defect
    assert all(f.what != "draft" for f in bad)              # no defect touches the proposal itself
