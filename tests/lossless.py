"""Statistical losslessness of the draft / verify / commit chain: shared code of tests/test_lossless.py (CPU, the oracle) and
tests/test_gpu_lossless.py (the HIP kernels).  numpy only: it imports neither torch nor the oracle, and it knows the target
distribution and nothing of this project's algorithm.

The claim: whatever the draft proposes, the token committed at position j of a sequence that reached j
(n_acc >= j) is distributed as softmax(x_t[j] / T) after the target's top-k / top-p truncation.  The chain is run many times
with fresh uniforms and the histogram of committed tokens is held to that distribution by a chi-square test at 1e-6.

  target_distribution   the HF chain Temperature -> TopK -> TopP in f64, from the definition, ties at the cut kept
  chi2_critical         Wilson-Hilferty upper quantile of chi-square (scipy may be absent where the GPU tests run)
  check_histogram       support + pooled chi-square, with the two conditions that keep a test from hiding behind pooling
  make_rows / reference the case tables: R logit classes of K + 1 target rows and K draft rows, their f64 distributions
  run_chain             the driver over a backend with draft / verify / residual callables
  evaluate              every histogram and accept count of a run against the reference"""
import math
from typing import NamedTuple

import numpy as np

T = 0.7
INV_T = float(np.float32(1.0) / np.float32(T))      # the f32 the kernels and the oracle are handed
ALPHA = 1e-6
R_CLASSES = 4
MIN_EXPECTED, MIN_BINS, MAX_POOLED = 20.0, 30, 0.10


class Route(NamedTuple):
    name: str
    d_top_k: int
    d_top_p: float
    t_top_k: int
    t_top_p: float
    family: str          # the entry points it takes: "plain" (verify + residual_sample[_ex]), "top_p", "top_k"


ROUTES = {r.name: r for r in (
    Route("a", 0, 1.0, 0, 1.0, "plain"),
    Route("b", 0, 0.9, 0, 1.0, "plain"),
    Route("c", 0, 0.9, 0, 0.95, "top_p"),
    Route("d", 50, 0.9, 50, 0.95, "top_k"),
    Route("e", 20, 1.0, 50, 1.0, "top_k"),
)}


# ------------------------------------------------------------------------------------------------ reference distribution
def target_distribution(x_f32_row, inv_temperature, top_k, top_p):
    """(p f64[V], thr, gap): softmax(x * inv_temperature) after TopK (every tie at the k-th largest value kept; a row with
    fewer than k values > -inf kept whole) and then TopP over that set (the smallest upper set { x >= v } whose mass reaches
    top_p: every tie at the cut kept), renormalised.  The kept set is { x >= thr }; thr = -inf where nothing is cut.
    gap: how far top_p lies from the mass of the kept set and from the mass of the next smaller upper set, whichever is
    nearer (inf with top-p off).  top_k <= 0 or >= V and top_p outside (0, 1) are no-ops."""
    x = np.asarray(x_f32_row, np.float32).astype(np.float64)
    V = x.shape[0]
    thr = -np.inf
    keep = x > -np.inf
    if 0 < top_k < V and int(keep.sum()) >= top_k:
        thr = np.sort(x)[V - top_k]
        keep = x >= thr
    z = np.where(keep, x * float(inv_temperature), -np.inf)
    e = np.exp(z - z.max())
    p = e / e.sum()
    gap = np.inf
    if 0.0 < top_p < 1.0:
        vals = np.unique(x[keep])[::-1]                                   # distinct kept values, largest first
        upper = np.array([p[x >= v].sum() for v in vals]) if vals.size <= 64 else _upper_masses(x, p, keep, vals)
        i = int(np.argmax(upper >= top_p)) if (upper >= top_p).any() else vals.size - 1
        thr = vals[i]
        gap = min(abs(upper[i] - top_p), abs(top_p - (upper[i - 1] if i else 0.0)))
        p = np.where(x >= thr, p, 0.0)
        p = p / p.sum()
    return p, np.float32(thr), float(gap)


def _upper_masses(x, p, keep, vals):
    """Mass of { x >= v } for every distinct value v (largest first), in one pass over the sorted row."""
    order = np.argsort(-x[keep], kind="stable")
    xs, cs = x[keep][order], np.cumsum(p[keep][order])
    last = np.searchsorted(-xs, -vals, side="right") - 1                  # the last position holding each value
    return cs[last]


# ------------------------------------------------------------------------------------------------ statistics
def normal_isf(alpha):
    """z with P(N(0,1) > z) = alpha, by bisection on erfc."""
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if 0.5 * math.erfc(mid / math.sqrt(2.0)) > alpha:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def _chi2_sf(x, df):
    """P(chi-square_df > x) for x > df: the upper incomplete gamma function by its continued fraction (modified Lentz)."""
    a, x = 0.5 * df, 0.5 * x
    tiny = 1e-300
    b = x + 1.0 - a
    c, d = 1.0 / tiny, 1.0 / b
    h = d
    for i in range(1, 2000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-15:
            break
    return math.exp(-x + a * math.log(x) - math.lgamma(a)) * h


def chi2_critical(df, alpha):
    """Upper-alpha quantile of chi-square with df degrees of freedom: the Wilson-Hilferty approximation, which at 1e-6 is 4.5 %
    high at df = 5 (and so would pass too much), brought onto the exact tail by bisection around it."""
    a = 2.0 / (9.0 * df)
    wh = df * (1.0 - a + normal_isf(alpha) * math.sqrt(a)) ** 3
    lo, hi = max(0.8 * wh, df + 2.0), 1.2 * wh
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if _chi2_sf(mid, df) > alpha:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


class HistogramError(AssertionError):
    """kind: "structure" (the test's own conditions), "support" (mass where p = 0) or "chi2"."""

    def __init__(self, kind, msg):
        super().__init__(f"{kind}: {msg}")
        self.kind = kind


def check_histogram(counts, p, n, min_bins=MIN_BINS):
    """counts[v] of n draws against the distribution p.  counts may be longer than p (ids past the vocabulary): every bin
    where p = 0 must be empty.  Bins with an expected count < 20 are pooled into one tail bin; at least min_bins bins stay
    unpooled and the pooled bin holds at most 10 % of the mass, or the check fails whatever the counts are.
    Returns (chi2, critical value at 1e-6, df)."""
    counts = np.asarray(counts, np.int64)
    p = np.asarray(p, np.float64)
    pp = np.zeros(counts.shape[0])
    pp[:p.shape[0]] = p
    if int(counts.sum()) != int(n):
        raise HistogramError("structure", f"{int(counts.sum())} draws counted, {int(n)} expected")
    outside = int(counts[pp == 0.0].sum())
    if outside != 0:
        raise HistogramError("support", f"{outside} of {n} draws outside the support, ids {np.nonzero((pp == 0) & (counts > 0))[0][:8]}")
    expected = pp * n
    big = expected >= MIN_EXPECTED
    pooled_mass = float(pp[~big].sum())
    if int(big.sum()) < min_bins:
        raise HistogramError("structure", f"{int(big.sum())} unpooled bins < {min_bins} (n = {n})")
    if pooled_mass > MAX_POOLED:
        raise HistogramError("structure", f"pooled bin holds {pooled_mass:.3f} of the mass (n = {n})")
    chi2 = float(((counts[big] - expected[big]) ** 2 / expected[big]).sum())
    bins = int(big.sum())
    if pooled_mass > 0.0:
        ep = pooled_mass * n
        chi2 += float((counts[~big].sum() - ep) ** 2 / ep)
        bins += 1
    df = bins - 1
    crit = chi2_critical(df, ALPHA)
    if not chi2 <= crit:
        raise HistogramError("chi2", f"chi2 {chi2:.1f} > {crit:.1f} (df {df}, n {n})")
    return chi2, crit, df


def check_accept_count(accepted, n, rate):
    """Two-sided normal-approximation test at 1e-6 of accepted ~ Binomial(n, rate).  Returns (|z|, critical z)."""
    var = n * rate * (1.0 - rate)
    if not var >= 100.0:
        raise HistogramError("structure", f"n rate (1 - rate) = {var:.1f} < 100")
    z = abs(accepted - n * rate) / math.sqrt(var)
    zc = normal_isf(ALPHA / 2.0)
    if not z <= zc:
        raise HistogramError("accept", f"{accepted} of {n} accepted, rate {rate:.5f} expected: |z| {z:.1f} > {zc:.2f}")
    return z, zc


# ------------------------------------------------------------------------------------------------ cases
def decode_storage(x, dtype):
    """f32 values as a bf16 / f16 / f32 store returns them (round to nearest even)."""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == "f32":
        return x
    if dtype == "f16":
        return x.astype(np.float16).astype(np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32).reshape(x.shape)


class Geometry(NamedTuple):
    """Logit rows of one geometry: scale * N(0, 1) everywhere, and on `head` random ids of each target row
    boost + head_scale * N(0, 1) instead (head = 0: none); the draft row is the target row + noise * N(0, 1)."""
    V: int
    K: int
    B: int
    n_calls: int
    scale: float
    noise: float
    head: int = 0
    boost: float = 0.0
    head_scale: float = 0.0


# V = 512: scale / noise put every accept rate in [0.3, 0.9] and leave >= 30 bins with an expected count >= 20 at the bonus
# position; V = 152064: a head of a few dozen tokens carries the mass, so the truncated support is testable over the whole
# vocabulary (tests/test_lossless.py asserts all of it on the reference alone).
SMALL = Geometry(V=512, K=4, B=4096, n_calls=50, scale=1.0, noise=0.35, head=96, boost=6.0, head_scale=1.1)
FULL = Geometry(V=152064, K=2, B=32, n_calls=3072, scale=1.0, noise=0.4, head=96, boost=14.0, head_scale=0.6)


def make_rows(geom, dtype, seed):
    """(xt [R, K + 1, V], xd [R, K, V]): the stored values (f32 after the dtype's rounding) of every class's rows."""
    rng = np.random.default_rng([seed, geom.V, geom.K])
    R, K, V = R_CLASSES, geom.K, geom.V
    xt = (rng.standard_normal((R, K + 1, V)) * geom.scale).astype(np.float32)
    if geom.head:
        for c in range(R):
            for j in range(K + 1):
                ids = rng.choice(V, geom.head, replace=False)
                xt[c, j, ids] = (geom.boost + geom.head_scale * rng.standard_normal(geom.head)).astype(np.float32)
    xd = (xt[:, :K] + rng.standard_normal((R, K, V)) * geom.noise).astype(np.float32)
    return decode_storage(xt, dtype), decode_storage(xd, dtype)


class Reference(NamedTuple):
    p_t: np.ndarray     # [R, K + 1, V] f64
    p_d: np.ndarray     # [R, K, V] f64
    rate: np.ndarray    # [R, K]  sum_v min(p_t, p_d)
    gap: float          # the smallest mass gap at any top-p cut


def reference(xt, xd, route):
    R, K1, V = xt.shape
    p_t, p_d = np.empty((R, K1, V)), np.empty((R, K1 - 1, V))
    gap = np.inf
    for c in range(R):
        for j in range(K1):
            p_t[c, j], _, g = target_distribution(xt[c, j], INV_T, route.t_top_k, route.t_top_p)
            gap = min(gap, g)
            if j < K1 - 1:
                p_d[c, j], _, g = target_distribution(xd[c, j], INV_T, route.d_top_k, route.d_top_p)
                gap = min(gap, g)
    return Reference(p_t, p_d, np.minimum(p_t[:, :-1], p_d).sum(-1), float(gap))


def expected_reach(ref):
    """[R, K + 1]: the probability that a sequence of class c reaches position j."""
    R, K = ref.rate.shape
    return np.concatenate([np.ones((R, 1)), np.cumprod(ref.rate, axis=1)], axis=1)


def check_inputs(ref, route, n_per_class):
    """The conditions the case tables are built to meet, on the reference alone."""
    R, K = ref.rate.shape
    assert ((ref.rate >= 0.3) & (ref.rate <= 0.9)).all(), ref.rate
    reach = expected_reach(ref)
    assert (reach[:, K] >= 0.15).all(), reach[:, K]
    assert ref.gap >= 1e-4, ref.gap
    for c in range(R):
        for j in range(K + 1):
            n = reach[c, j] * n_per_class * 0.97                 # (the reach count itself fluctuates by < 3 % here)
            _structure(ref.p_t[c, j], n, MIN_BINS, ("target", c, j))
            if j < K:
                _structure(ref.p_d[c, j], n_per_class, draft_min_bins(ref.p_d[c, j]), ("draft", c, j))
                assert n_per_class * reach[c, j] * 0.97 * ref.rate[c, j] * (1 - ref.rate[c, j]) >= 100.0


def _structure(p, n, min_bins, what):
    big = p * n >= MIN_EXPECTED
    assert int(big.sum()) >= min_bins, (what, int(big.sum()), n)
    assert p[~big].sum() <= MAX_POOLED, (what, float(p[~big].sum()), n)


def draft_min_bins(p_d):
    """The committed-token histograms keep >= 30 unpooled bins.  A draft cut to top-k 20 has no 30 tokens to offer: its
    histogram must then keep EVERY token of its support unpooled, the most that distribution allows."""
    return min(MIN_BINS, int((p_d > 0).sum()))


# ------------------------------------------------------------------------------------------------ driver
class NumpyOps:
    """The few array operations the bookkeeping needs; the GPU test supplies the same five over torch tensors on the device."""
    arange = staticmethod(lambda n: np.arange(n, dtype=np.int64))
    i64 = staticmethod(lambda a: np.asarray(a).astype(np.int64))
    where = staticmethod(np.where)
    bincount = staticmethod(lambda keys, n: np.bincount(keys, minlength=n))
    to_numpy = staticmethod(lambda a: np.asarray(a))


class Counts(NamedTuple):
    commit: np.ndarray    # [R, K + 1, W] committed tokens at j over the sequences with n_acc >= j (W - 1: not a token id)
    draft: np.ndarray     # [R, K, W]     drafted tokens at j over all sequences
    n_seq: int            # sequences run (n_seq / R of every class)


def run_chain(backend, geom, seed, width, xp=NumpyOps, n_calls=None):
    """n_calls rounds of B sequences (sequence b is of class b % R) through backend.draft / .verify / .residual, each round on
    fresh uniforms from default_rng([seed, call]):
        tok, lp_d, d_thr = backend.draft(r [B * K])             one proposal per (b, j): row b * K + j
        n_acc, t_thr     = backend.verify(tok, lp_d, u [B, K])
        drawn            = backend.residual(n_acc, r [B], d_thr, t_thr)
    The uniforms are numpy f32 arrays; what the backend returns stays in its own array type (xp's).  `width` is the length
    of a histogram row: ids in [V, width - 1) are counted as they come (a read across a padded row's stride lands there), any
    other value in the last slot."""
    R, K, B = R_CLASSES, geom.K, geom.B
    assert B % R == 0
    n_calls = geom.n_calls if n_calls is None else n_calls
    cls = xp.arange(B) % R
    jj = xp.arange(K)
    commit = draft = None
    for call in range(n_calls):
        rng = np.random.default_rng([seed, call])
        r_d = rng.random(B * K, dtype=np.float32)
        u = rng.random((B, K), dtype=np.float32)
        r_c = rng.random(B, dtype=np.float32)
        tok, lp_d, d_thr = backend.draft(r_d)
        n_acc, t_thr = backend.verify(tok, lp_d, u)
        drawn = backend.residual(n_acc, r_c, d_thr, t_thr)
        tok, n_acc, drawn = xp.i64(tok).reshape(B, K), xp.i64(n_acc), xp.i64(drawn)

        def slot(t):
            return xp.where((t >= 0) & (t < width - 1), t, width - 1)
        # position j < K: the drafted token where it was accepted, the drawn one at j = n_acc; position K: the bonus draw
        at_j = slot(xp.where(jj[None, :] < n_acc[:, None], tok, drawn[:, None]))
        key = (cls[:, None] * (K + 1) + jj[None, :]) * width + at_j
        key_k = (cls * (K + 1) + K) * width + slot(drawn)
        c = xp.bincount(key[jj[None, :] <= n_acc[:, None]], R * (K + 1) * width) \
            + xp.bincount(key_k[n_acc == K], R * (K + 1) * width)
        d = xp.bincount(((cls[:, None] * K + jj[None, :]) * width + slot(tok)).reshape(-1), R * K * width)
        commit = c if commit is None else commit + c
        draft = d if draft is None else draft + d
    return Counts(xp.to_numpy(commit).reshape(R, K + 1, width), xp.to_numpy(draft).reshape(R, K, width), n_calls * B)


# ------------------------------------------------------------------------------------------------ evaluation
class Finding(NamedTuple):
    what: str        # "commit", "draft" or "accept"
    cls: int
    j: int
    stat: float      # chi2, or |z| of the accept count (nan where the check stopped before computing it)
    crit: float
    n: int
    error: object    # None, or the HistogramError


def evaluate(counts, ref):
    """Every check of one run, failed ones included (nothing is raised here): per class and position the committed-token
    histogram over the sequences that reached it, and for j < K the drafted-token histogram and the accept count."""
    R, K = ref.rate.shape
    n_c = counts.n_seq // R
    reach = counts.commit.sum(-1)                                  # [R, K + 1]: sequences with n_acc >= j
    out = []

    def run(what, c, j, n, fn):
        try:
            stat, crit = fn()[:2]
            out.append(Finding(what, c, j, stat, crit, int(n), None))
        except HistogramError as e:
            out.append(Finding(what, c, j, float("nan"), float("nan"), int(n), e))

    for c in range(R):
        for j in range(K + 1):
            run("commit", c, j, reach[c, j], lambda: check_histogram(counts.commit[c, j], ref.p_t[c, j], reach[c, j]))
            if j < K:
                run("draft", c, j, n_c, lambda: check_histogram(counts.draft[c, j], ref.p_d[c, j], n_c,
                                                                draft_min_bins(ref.p_d[c, j])))
                run("accept", c, j, reach[c, j], lambda: check_accept_count(int(reach[c, j + 1]), int(reach[c, j]),
                                                                            float(ref.rate[c, j])))
    return out


def failures(findings, statistical_only=False):
    bad = [f for f in findings if f.error is not None]
    return [f for f in bad if f.error.kind != "structure"] if statistical_only else bad


def summary(findings):
    """One line per kind: the largest chi2 / critical ratio (the smallest margin) among the passed checks."""
    lines = []
    for what in ("commit", "draft", "accept"):
        ok = [f for f in findings if f.what == what and f.error is None]
        if ok:
            w = max(ok, key=lambda f: f.stat / f.crit)
            lines.append(f"{what}: {len(ok)} checks, worst {w.stat:.1f} / {w.crit:.1f} at class {w.cls} j {w.j} (n {w.n})")
    return "; ".join(lines)


def assert_lossless(findings, label):
    bad = failures(findings)
    print(f"[lossless] {label}: {summary(findings)}")
    assert not bad, f"{label}: " + " | ".join(f"{f.what} class {f.cls} j {f.j}: {f.error}" for f in bad[:6])
