"""References, bounds and input builders for the decoder-stack tests (plain torch: no kernels, no package; every function works on
the device of the tensors it is given, and the module itself needs none).

tests/test_decoder_refs.py shows on the CPU that the assertions below pass a faithful restatement of k_attn_ragged's algorithm
and fail six single defects of it; tests/test_gpu_decoder_edges.py holds the kernel itself to the same assertions on the same
cases (the builders are pure functions of the case, so both see the same bits).  The f64 references of the single ops at the end
(rmsnorm_ref, linear_ref, rope_ref, attn_ref, silu_mul_ref) are chained over a model by tests/test_decoder_refs.py, which holds the
chain to SyntheticLM's own f64 forward; tests/test_gpu_decoder_widths.py holds every kernel of the stack to them."""
import math
from collections import namedtuple
from functools import lru_cache

import torch

BF = torch.bfloat16
HD = 128
TILE = 32
NEG_BIG = -1.0e30                       # the kernel's finite running-max sentinel
SCALE_LOG2 = 1.4426950408889634074 / math.sqrt(float(HD))

DEFECTS = ("mask_lt", "mask_plus_one", "drop_key", "swap_v", "no_rescale", "merge_unscaled")


def _row_of(M, n_cache_rows, row_of):
    if row_of is not None:
        return [int(r) for r in row_of]
    assert M % n_cache_rows == 0
    return [m // (M // n_cache_rows) for m in range(M)]


def attn_ref(q, k, v, pos, row_of=None):
    """f64 softmax attention with grouped queries.  q [M, H, 128], k and v [cache rows, KVH, t_max, 128] (v NOT transposed),
    pos [M]; query position m reads cache row row_of[m] (default: M / rows consecutive positions per row), head `head` reads kv
    head `head // (H / KVH)`, keys j <= pos[m], scores q.k / sqrt(128).  Returns (ref, A), both [M, H, 128] f64:
    ref = sum_j p_j v_j and A = sum_j p_j |v_j| with p the softmax weights."""
    M, H, _ = q.shape
    KVH, t_max = k.shape[1], k.shape[2]
    rep = H // KVH
    rows = _row_of(M, k.shape[0], row_of)
    pos = torch.as_tensor(pos).tolist()
    q64 = q.double().view(M, KVH, rep, HD)
    ref = torch.empty(M, H, HD, dtype=torch.float64, device=q.device)
    A = torch.empty_like(ref)
    j = torch.arange(t_max, device=q.device)
    for m in range(M):
        kk, vv = k[rows[m]].double(), v[rows[m]].double()                       # [KVH, t_max, 128]
        sc = torch.matmul(q64[m], kk.transpose(1, 2)) / math.sqrt(float(HD))     # [KVH, rep, t_max]
        sc = sc.masked_fill(j > int(pos[m]), -math.inf)
        p = torch.softmax(sc, dim=-1)
        ref[m] = torch.matmul(p, vv).view(H, HD)
        A[m] = torch.matmul(p, vv.abs()).view(H, HD)
    return ref, A


def attn_bound(ref, A):
    """1.05 * 2^-8 * (A + |ref|) + 1e-6, element by element.

    k_attn_ragged computes out = (sum_j bf16(p_j) v_j) / (sum_j p_j) with p_j = exp2(s_j - max) in f32 and rounds out to bf16.
    * Each weight is rounded to bf16 (8 significant bits, round to nearest: relative error <= 2^-8) before the second MFMA, so the
      numerator is off by at most 2^-8 * sum_j p_j |v_j| = 2^-8 * A after the division.
    * The denominator is summed in f32 from the UNROUNDED weights: it carries no 2^-8 term.
    * The quotient is rounded once to bf16: <= 2^-8 |out|.
    * The factor 1.05 covers the second-order terms and the errors of v_exp_f32 and of the f32 accumulations (about 2^-22
      relative each; a score of magnitude up to 2^7 carries an f32 rounding of 2^-17, i.e. 2^-17 ln 2 relative in its weight).
    * 1e-6 covers values flushed near zero.
    One key dropped, duplicated or leaked at L keys moves an element by about |v| / L; at L = 300 that is 3e-3 against a bound of
    about 2^-8 * 0.8 = 3e-3 for unit Gaussian V, and the flat 6e-3 of tests/test_gpu_decoder.py is twice that -- hence the
    uniform and needle cases below, whose bounds have no such slack."""
    return 1.05 * 2.0 ** -8 * (A + ref.abs()) + 1.0e-6


def _bf16_round(x):
    return x.to(BF).float()


def attn_emulated(q, k, v, pos, row_of=None, defect=None):
    """k_attn_ragged's algorithm restated in plain f32 torch: 32-key tiles dealt round-robin to four streams (the kernel's four
    waves), each with a running max / running sum / accumulator that is rescaled by alpha = exp2(m_old - m_new) per tile, scores
    in log2 units, masked scores -inf over a finite sentinel, P rounded to bf16 for the second product while the sum takes the
    unrounded values, the four streams merged in order with exp2(m_w - m_all), one division, one rounding to bf16.  Every query
    row walks every tile up to the largest position (tiles past its own position contribute exact zeros, as in a kernel row tile
    that mixes positions).  Returns [M, H, 128] f32 holding bf16 values.

    defect: None or one of DEFECTS --
      mask_lt         keys j < pos instead of j <= pos
      mask_plus_one   keys j <= pos + 1
      drop_key        key 32 n + 5 of the middle tile n is skipped
      swap_v          the V rows of keys 33 and 44 (tile 1) are exchanged
      no_rescale      the accumulator is not multiplied by alpha (the running sum still is)
      merge_unscaled  the four streams are merged without exp2(m_w - m_all)"""
    assert defect is None or defect in DEFECTS
    M, H, _ = q.shape
    KVH, t_max = k.shape[1], k.shape[2]
    rep = H // KVH
    rows = torch.tensor(_row_of(M, k.shape[0], row_of))
    pos = torch.as_tensor(pos).to(torch.int64)
    limit = pos.clone()                                       # last live key per query position
    if defect == "mask_lt":
        limit = pos - 1
    if defect == "mask_plus_one":
        limit = (pos + 1).clamp(max=t_max - 1)
    n_tiles = int(limit.max()) // TILE + 1
    qf = q.float().view(M, KVH, rep, HD)
    kf, vf = k.float(), v.float()                             # [cache rows, KVH, t_max, 128]
    if defect == "swap_v" and t_max > 44:
        vf = vf.clone()
        vf[:, :, [33, 44]] = vf[:, :, [44, 33]]
    dropped = TILE * (n_tiles // 2) + 5 if defect == "drop_key" else -1
    scale = torch.tensor(SCALE_LOG2, dtype=torch.float32)
    m_run = torch.full((4, M, KVH, rep), NEG_BIG, dtype=torch.float32)
    l_run = torch.zeros(4, M, KVH, rep, dtype=torch.float32)
    acc = torch.zeros(4, M, KVH, rep, HD, dtype=torch.float32)
    for tile in range(n_tiles):
        w = tile % 4
        key = torch.arange(TILE * tile, TILE * tile + TILE)
        kt, vt = kf[rows, :, TILE * tile: TILE * tile + TILE], vf[rows, :, TILE * tile: TILE * tile + TILE]   # [M, KVH, 32, 128]
        s = torch.matmul(qf, kt.transpose(2, 3)) * scale                                 # [M, KVH, rep, 32]
        ok = (key[None, :] <= limit[:, None]) & (key[None, :] != dropped)                # [M, 32]
        s = torch.where(ok[:, None, None, :], s, torch.tensor(-math.inf))
        m_new = torch.maximum(m_run[w], s.max(dim=-1).values)
        alpha = torch.exp2(m_run[w] - m_new)
        p = torch.exp2(s - m_new[..., None])
        l_run[w] = l_run[w] * alpha + p.sum(dim=-1)
        m_run[w] = m_new
        if defect != "no_rescale":
            acc[w] = acc[w] * alpha[..., None]
        acc[w] = acc[w] + torch.matmul(_bf16_round(p), vt)
    m_all = m_run.max(dim=0).values
    f = torch.exp2(m_run - m_all[None])
    if defect == "merge_unscaled":
        f = torch.ones_like(f)
    l_all = torch.zeros_like(m_all)
    o_all = torch.zeros_like(acc[0])
    for w in range(4):
        l_all = l_all + l_run[w] * f[w]
        o_all = o_all + acc[w] * f[w][..., None]
    inv_l = torch.where(l_all > 0, 1.0 / l_all, torch.zeros_like(l_all))
    return _bf16_round(o_all * inv_l[..., None]).view(M, H, HD)


# ---- the attention cases: pure functions of (kind, geometry, pos0, subset)

T_MAX = 4096
NEEDLES = (0, 1, 31, 32, 33, 127, 128, 129, 2047, 2048, 4000, None)          # None: the case's largest position

AttnCase = namedtuple("AttnCase", "kind Bn T H KVH t_max pos0 cache_rows rows")

_GEOMS = ((2, 5, 8, 2), (2, 9, 28, 4))                # rep * T = 20: one row tile; 63: two row tiles mixing positions and heads
KINDS = ("uniform", "needle", "rising", "gaussian")


def attn_cases():
    out = []
    for kind in KINDS:
        for Bn, T, H, KVH in _GEOMS:
            out.append(AttnCase(kind, Bn, T, H, KVH, T_MAX, (0, T_MAX - T), Bn, None))       # first token | a full cache
            out.append(AttnCase(kind, Bn, T, H, KVH, T_MAX, (95, 1029), Bn, None))           # ragged last tile, n_tiles % 4 != 0
        Bn, T, H, KVH = _GEOMS[0]
        out.append(AttnCase(kind, Bn, T, H, KVH, T_MAX, (0, T_MAX - T), 4, (3, 1)))         # rows: a subset of a larger cache
    return out


def case_id(c):
    return f"{c.kind}-B{c.Bn}T{c.T}H{c.H}KV{c.KVH}-pos{c.pos0[0]}_{c.pos0[1]}" + ("-subset" if c.rows else "")


def _seed(c):
    return 1000 * KINDS.index(c.kind) + 100 * c.H + 10 * c.T + (c.pos0[0] % 7) + (50 if c.rows else 0)


def _needle_rows(c, pos, needles):
    """needle index per query row (m, head): among the needles at or before pos[m] the one chosen least often so far, the LATER
    one on a tie (few rows can reach the late needles); a row at position 0 can only take needle 0."""
    count = [0] * len(needles)
    pick = torch.empty(len(pos), c.H, dtype=torch.int64)
    for m in range(len(pos)):
        live = [i for i, j in enumerate(needles) if j <= int(pos[m])]
        for head in range(c.H):
            i = min(reversed(live), key=lambda n: count[n])
            count[i] += 1
            pick[m, head] = i
    return pick, count


@lru_cache(maxsize=None)
def build_attn_case(c):
    """The inputs of case c as CPU tensors holding bf16-exact values, its f64 reference and the bound each element is held to:
    dict(q [M, H, 128] bf16, k / v [cache rows, KVH, t_max, 128] bf16, pos [M] int32, row_of [M], ref, bound [M, H, 128] f64,
    exact_zero: mask of elements that must be exactly 0).  Callers must not modify what they get (the result is shared)."""
    g = torch.Generator().manual_seed(_seed(c))
    M = c.Bn * c.T
    pos = (torch.tensor(c.pos0)[:, None] + torch.arange(c.T)).reshape(M)
    assert int(pos.max()) < c.t_max
    rows = list(c.rows) if c.rows else list(range(c.Bn))
    row_of = [rows[m // c.T] for m in range(M)]
    kv_shape = (c.cache_rows, c.KVH, c.t_max, HD)
    extra = {}
    if c.kind == "uniform":
        # every score 0, every weight exactly 1; V in multiples of 2^-3 within [-4, 4]: every partial sum is a multiple of 2^-3 below
        # 2^21, exact in f32 in any order, and l = L exactly.  out = fl_bf16(fl(fl(1 / L) * sum)): 2^-8 + 2 * 2^-24 relative.
        q = torch.randn(M, c.H, HD, generator=g)
        k = torch.zeros(kv_shape)
        v = torch.randint(-32, 33, kv_shape, generator=g).float() / 8.0
    elif c.kind == "needle":
        # k = 32 e_c at needle c, zero elsewhere; q = 32 e_c: the needle's score leads by 1024 / sqrt(128) * log2(e) = 130.6 binades,
        # every other weight is below 2^-130, their sum over 4096 keys of |v| <= 8 below 2^-115: out = v[needle] to the last bit.
        needles = sorted({int(pos.max()) if j is None else j for j in NEEDLES})
        assert len(needles) == len(NEEDLES)
        pick, count = _needle_rows(c, pos, needles)
        reachable = [j <= int(pos.max()) for j in needles]
        # every needle a row can see is chosen (pos0 = [95, 1029] cannot see 2047, 2048, 4000: they stay in the cache as live masked
        # keys; the [0, t_max - T] cases choose all twelve -- tests/test_decoder_refs.py::test_case_table)
        assert all(n > 0 for n, r in zip(count, reachable) if r), (needles, count)
        k = torch.zeros(kv_shape)
        for i, j in enumerate(needles):
            k[:, :, j, i] = 32.0
        q = torch.zeros(M, c.H, HD)
        q.scatter_(2, pick[..., None], 32.0)
        v = torch.randn(kv_shape, generator=g).clamp_(-8, 8)
        extra = dict(needles=needles, pick=pick, count=count)
    elif c.kind == "rising":
        # k_j = (j // 32) / 2 * w with w = +-1 (exact in bf16: 7 bits); q.w = 16 +- 3: every tile lifts the score by about one binade,
        # so every tile of every stream rescales (alpha about 2^-4) and the streams meet with different maxima
        w = (torch.randint(0, 2, (HD,), generator=g) * 2 - 1).float()
        q = 0.25 * torch.randn(M, c.H, HD, generator=g) + 0.125 * w
        k = ((torch.arange(c.t_max) // TILE).float() * 0.5)[None, None, :, None] * w.expand(kv_shape)
        v = torch.randn(kv_shape, generator=g)
        assert bool(((q.to(BF).float() * w).sum(-1) > 4.0).all())
    else:
        q = torch.randn(M, c.H, HD, generator=g)
        k = torch.randn(kv_shape, generator=g)
        v = torch.randn(kv_shape, generator=g)
    q, k, v = q.to(BF), k.to(BF), v.to(BF)
    ref, A = attn_ref(q, k, v, pos, row_of)
    exact_zero = torch.zeros_like(ref, dtype=torch.bool)
    if c.kind == "uniform":
        # ref = (sum_{j <= pos} v_j) / L with the sum exact in f64 (the softmax of attn_ref holds 1 / L to 2^-53 only)
        kvh_of = (torch.arange(c.H) // (c.H // c.KVH))[None, :]
        total = v.double().cumsum(dim=2)[torch.tensor(row_of)[:, None], kvh_of, pos[:, None]]            # [M, H, 128]
        want = total / (pos + 1).double()[:, None, None]
        assert float((want - ref).abs().max()) <= 2.0 ** -48
        ref = want
        bound = (2.0 ** -8 + 2.0 ** -20) * ref.abs()          # no absolute term: one key too many at L = 4096 is 4 x the bound
        exact_zero = ref == 0
    elif c.kind == "needle":
        hit = torch.tensor(extra["needles"])[extra["pick"]]                              # [M, H] key index
        want = v[torch.tensor(row_of)[:, None], (torch.arange(c.H) // (c.H // c.KVH))[None, :], hit].double()   # [M, H, 128]
        assert float((want - ref).abs().max()) <= 2.0 ** -100                             # the two references agree
        ref = want
        bound = torch.full_like(ref, 2.0 ** -40)
    else:
        bound = attn_bound(ref, A)
    return dict(q=q, k=k, v=v, pos=pos.to(torch.int32), row_of=row_of, ref=ref, bound=bound, exact_zero=exact_zero, **extra)


def attn_violations(out, case):
    """(number of elements of `out` [M, H, 128] outside the case's assertion, worst |err| / bound)."""
    err = (out.double() - case["ref"]).abs()
    bad = (err > case["bound"]) | (case["exact_zero"] & (out != 0)) | ~torch.isfinite(out)
    ratio = err / case["bound"]
    ratio = ratio[case["bound"] > 0]
    return int(bad.sum()), float(ratio.max()) if ratio.numel() else 0.0


# ---- rotary embedding

def rope_ref(x, pos, inv_freq):
    """x [M, heads, 128] (any float type), pos [M] integer, inv_freq [64] f32 -> f64.  The angle is the f32 product
    f32(pos) * inv_freq of the kernel, its cosine and sine are f64: pairs (i, i + 64)."""
    ang = (pos.float()[:, None] * inv_freq.float()[None, :]).double()[:, None, :]
    x = x.double()
    x1, x2 = x[..., : HD // 2], x[..., HD // 2:]
    return torch.cat([x1 * ang.cos() - x2 * ang.sin(), x2 * ang.cos() + x1 * ang.sin()], dim=-1)


def rope_bound(ref):
    """2^-8 |ref| + 1e-5 (tests/test_gpu_decoder.py::test_rope_kv_store): one bf16 rounding plus the cosf / sinf error."""
    return 2.0 ** -8 * ref.abs() + 1.0e-5


# ---- the other ops of a decoder layer, and inputs that are not the special case bias = 0, norm weight = 1

def rmsnorm_ref(x, w, eps):
    """x [M, D], w [D] (any float type) -> f64 x * rsqrt(mean(x^2) + eps) * w."""
    v = x.double()
    return v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps) * w.double()


def silu_mul_ref(gu):
    """gu [M, 2 I] = gate | up (any float type) -> f64 [M, I] silu(gate) * up."""
    I = gu.shape[-1] // 2
    g, u = gu[..., :I].double(), gu[..., I:].double()
    return g / (1.0 + torch.exp(-g)) * u


def linear_ref(x, w, bias=None, residual=None):
    """x [M, D], w [N, D] (nn.Linear layout), bias [N] or None, residual [M, N] or None -> f64 x . w^T + bias + residual."""
    r = x.double() @ w.double().T
    if bias is not None:
        r = r + bias.double()
    if residual is not None:
        r = r + residual.double()
    return r


def elementwise_bound(ref):
    """2^-8 |ref| + 1e-6 (tests/test_gpu_decoder.py::test_rmsnorm, test_silu_mul): f32 arithmetic and one bf16 rounding."""
    return 2.0 ** -8 * ref.abs() + 1.0e-6


def linear_bound(ref):
    """2^-8 |ref| + 2e-4 (tests/test_gpu_linear.py::_check for bf16): f32 accumulation in MFMA order and one bf16 rounding."""
    return 2.0 ** -8 * ref.abs() + 2.0e-4


def randomize_affine(lm, seed):
    """Every `*.bias` of the model becomes N(0, 1) and every norm weight 1 + 0.25 N(0, 1), in place and in the model's dtype
    (SyntheticLM initialises them to 0 and 1, where a wrong bias or weight index changes nothing).  The values are drawn on the
    CPU in f32, in named_parameters order, and then copied to the parameter's device: one seed gives the same values to a CPU and a
    GPU model.  Call it before enable_hip_layers (which re-points q|k|v biases at a fused buffer)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in lm.named_parameters():
            if p.dim() != 1:
                continue
            z = torch.randn(p.shape, generator=g, dtype=torch.float32)
            if not name.endswith(".bias"):
                z = 1.0 + 0.25 * z
            p.copy_(z.to(p.dtype))
