"""Per-sequence sampling parameters on the GPU: asd_draft_sample_rows, asd_verify_accept_rows, asd_residual_sample_lp_rows and
asd_top_logprobs_rows (include/asd_hip.h, "Per-sequence sampling parameters").  Bars:
  1. sequence b of a *_rows call has the BITS of the scalar min-p entry point called with b's four values on the whole batch
     (the draft's token: of the one-workgroup form, asd_debug_draft_groups(-1); the commit draw at the same geometry, the
     heuristic's and the multi-launch / one-workgroup forms through asd_debug_residual_groups(-1); the top-N table at the same
     splits) -- the verify on all six outputs for every sequence that truncates something;
  2. one select: the draft's threshold and lp are the verify's t_nucleus_logit and lp_target for the drawn token, and the bonus
     row's threshold, untruncated sequences included;
  3. untruncated sequences of the verify: lp_target within 1e-5 of the f64 oracle run per sequence at its own temperature,
     accept / n_acc equal to the oracle's -- on ALL 24 rows: the case is chosen so that every oracle margin exceeds 1e-5, and
     the test asserts that first, on the oracle's margins alone;
  4. a uniform table is the scalar min-p entry points, bit for bit;
  5. status codes (a NULL table, B = 0, ...).
Shapes: V = 1000 (ragged last tile), 8200 bf16 / f16 and 4100 f32 (a second sweep trip), one pass at V = 152064 bf16; B = 8
sequences carrying the 8 on/off combinations of (top-k 50, top-p 0.9, min-p), K = 3; rows of every kind plus a Gaussian one."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import encode_logits, to_device_logits
from tests.test_gpu_min_p import rows_of_every_kind
from tests.test_gpu_top_k import V_FULL

pytestmark = pytest.mark.gpu

B, K = 8, 3
SMALL = [(O.DT_BF16, 1000), (O.DT_F16, 1000), (O.DT_F32, 1000), (O.DT_BF16, 8200), (O.DT_F16, 8200), (O.DT_F32, 4100)]
SHAPES = SMALL + [(O.DT_BF16, V_FULL)]
# (top_k, top_p, min_p, temperature) per sequence: the 8 on/off combinations; sequence 0 truncates nothing
TABLE_A = [(0, 1.0, 0.0, 0.7), (50, 1.0, 0.0, 0.5), (0, 0.9, 0.0, 0.9), (50, 0.9, 0.0, 1.0),
           (0, 1.0, 0.1, 1.3), (50, 1.0, 0.3, 2.0), (0, 0.9, 1e-6, 0.7), (50, 0.9, 0.1, 0.5)]


def table_b(V):
    """The edges: top_k = 1, top_k >= V (off), min_p = 1, top_p = 1.0 (off); sequence 5 truncates nothing."""
    return [(1, 1.0, 0.0, 0.7), (V, 0.9, 0.0, 1.0), (V + 7, 1.0, 1.0, 0.9), (0, 1.0, 1.0, 1.3),
            (1, 0.9, 1.0, 0.5), (0, 1.0, 0.0, 2.0), (50, 1.0, 0.0, 1.0), (2 ** 31 - 1, 0.5, 0.3, 0.7)]


def inv_t_of(T):
    return float(np.float32(1.0) / np.float32(T))


def truncates(p, V):
    return 0 < p[0] < V or 0.0 < p[1] < 1.0 or p[2] > 0.0


@pytest.fixture(scope="module")
def K_():
    from asd_amd import kernels
    return kernels


def make_rows(V, dtype, seed, n):
    """n storage rows [n, V]: blocks of rows_of_every_kind's seven plus one Gaussian row, rolled so that a sequence meets
    another kind at every position."""
    out = []
    k = 0
    while len(out) < n:
        store, _ = rows_of_every_kind(V, dtype, seed + 31 * k)
        g = encode_logits((np.random.default_rng(seed + 31 * k + 7).standard_normal((1, V)) * 4.0).astype(np.float32), dtype)
        block = np.concatenate([store, g])
        out.extend(np.roll(block, k, axis=0))
        k += 1
    return np.stack(out[:n])


def table_of(K_, params, V, tdtype):
    return K_.SamplingRows([inv_t_of(p[3]) for p in params], [p[0] for p in params], [p[1] for p in params],
                           [p[2] for p in params], V=V, dtype=tdtype)


def bits(*ts):
    return [t.cpu().numpy().tobytes() for t in ts]


class Plan:
    """The inputs of one (dtype, V): bonus / draft-step rows [B, V], target and draft rows [B, K, V], uniforms."""

    def __init__(self, dtype, V, n_seq=B):
        import torch
        self.dtype, self.V, self.n = dtype, V, n_seq
        rng = np.random.default_rng(77 + V % 1000 + dtype)
        sb = make_rows(V, dtype, 1000 + V % 1000 + dtype, n_seq)
        # (K blocks of n_seq rows; row (b, k) = block k's row b)
        st = np.stack([make_rows(V, dtype, 2000 + V % 1000 + dtype + 100 * k, n_seq) for k in range(K)], 1).reshape(n_seq * K, V)
        xt = O.logits_as_f32(st, dtype)
        sd = encode_logits((xt + rng.standard_normal(xt.shape).astype(np.float32) * 0.7).astype(np.float32), dtype)
        self.bonus = to_device_logits(sb, dtype).view(n_seq, V)
        self.t3 = to_device_logits(st, dtype).view(n_seq, K, V)
        self.d3 = to_device_logits(sd, dtype).view(n_seq, K, V)
        self.st = st
        cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()         # noqa: E731
        self.r_draft = cu(rng.uniform(0, 1, n_seq).astype(np.float32))
        self.r_k = [cu(rng.uniform(0, 1, n_seq).astype(np.float32)) for _ in range(K)]
        self.u = cu(rng.uniform(0, 1, (n_seq, K)).astype(np.float32))
        self.r_commit = cu(rng.uniform(0, 1, n_seq).astype(np.float32))
        n_acc = np.array([0, K, 1, 2, K, 0, K, 1] * (n_seq // 8 + 1), np.int32)[:n_seq]
        self.n_acc = cu(n_acc)
        self.noise = cu((-rng.uniform(0, 1.5, (n_seq, K))).astype(np.float32))
        self.swap = rng.integers(0, V, n_seq).astype(np.int32)


def run_rows(K_, plan, params):
    """Every *_rows op once -> dict of device tensors (the chain of a verifying step: K proposals on the target rows, the
    verify on the drawn tokens, the commit draw)."""
    import torch
    V, n = plan.V, plan.n
    tbl = table_of(K_, params, V, plan.t3.dtype)
    ds, rs = K_.DraftSampler(n, V, plan.t3.dtype), K_.ResidualSampler(n, V, plan.t3.dtype)
    out = dict(table=tbl, ds=ds, rs=rs)
    d = ds.rows(plan.bonus, plan.r_draft, tbl)
    out["draft"] = (d.tok, d.lp, d.thr)
    steps = [ds.rows(plan.t3[:, k].contiguous(), plan.r_k[k], tbl) for k in range(K)]
    dsteps = [ds.rows(plan.d3[:, k].contiguous(), plan.r_k[k], tbl) for k in range(K)]
    tok = torch.stack([s.tok for s in steps], 1).contiguous()
    out["drawn_tok"] = tok.clone()
    # position 1 of every other sequence: another token (usually outside the kept set: lp_target = -inf, n_finite = 1)
    tok[::2, 1] = torch.from_numpy(plan.swap).cuda()[::2]
    out["tok"] = tok
    out["step_lp"] = torch.stack([s.lp for s in steps], 1).contiguous()
    out["step_thr"] = torch.stack([s.thr for s in steps], 1).contiguous()
    out["d_thr"] = torch.stack([s.thr for s in dsteps], 1).contiguous()
    out["lp_d"] = torch.minimum(out["step_lp"] + plan.noise, torch.zeros_like(plan.noise)).contiguous()
    v = K_.verify_accept_rows(plan.t3, tok, out["lp_d"], plan.u, tbl)
    out["verify"] = (v.lp_target, v.accept, v.n_acc, v.accept_bits, v.t_nucleus_logit, v.n_finite)
    out["commit"] = rs.lp_rows(plan.t3, plan.d3, plan.n_acc, plan.r_commit, plan.bonus, rows=tbl, t_threshold=v.t_nucleus_logit,
                               d_threshold=out["d_thr"])
    torch.cuda.synchronize()
    return out


def scalar_draft(ds, lg, r, p):
    d = ds.min_p(lg, r, inv_t_of(p[3]), min_p=p[2], top_k=p[0], top_p=p[1])
    return d.tok, d.lp, d.thr


def check_against_scalar_calls(K_, plan, params, got, forced_residual=False):
    """Bars 1 and 2 for one table."""
    import torch
    V, n = plan.V, plan.n
    tdt = plan.t3.dtype
    ws = K_.VerifyWorkspace(n, K, V, tdt)
    sets = sorted(set(params), key=params.index)
    for p in sets:
        seqs = [b for b in range(n) if params[b] == p]
        inv_t = inv_t_of(p[3])
        # ---- the draft: lp / threshold at the scalar call's own geometry, the token at the one-workgroup form
        free = scalar_draft(K_.DraftSampler(n, V, tdt), plan.bonus, plan.r_draft, p)
        with K_.test_hooks() as lib:
            lib.asd_debug_draft_groups(-1)
            try:
                one = scalar_draft(K_.DraftSampler(n, V, tdt), plan.bonus, plan.r_draft, p)
                torch.cuda.synchronize()
            finally:
                lib.asd_debug_draft_groups(0)
        for b in seqs:
            g = [t[b:b + 1] for t in got["draft"]]
            assert bits(*g) == bits(*[t[b:b + 1] for t in one]), ("draft", p, b)
            assert bits(*g[1:]) == bits(*[t[b:b + 1] for t in free[1:]]), ("draft lp / thr, free geometry", p, b)
        # ---- the verify: all six outputs of a sequence that truncates something
        sv = K_.verify_accept_min_p(plan.t3, got["tok"], got["lp_d"], plan.u, ws, inv_temperature=inv_t, top_k=p[0], top_p=p[1],
                                    min_p=p[2])
        sv = (sv.lp_target, sv.accept, sv.n_acc, sv.accept_bits, sv.t_nucleus_logit, sv.n_finite)
        if truncates(p, V):
            for b in seqs:
                assert bits(*[t[b:b + 1] for t in got["verify"]]) == bits(*[t[b:b + 1] for t in sv]), ("verify", p, b)
        # ---- the commit draw: token and lp at the same geometry (the scalar call is handed the rows call's thresholds)
        rs = K_.ResidualSampler(n, V, tdt)
        kw = dict(top_k=p[0], top_p=p[1], min_p=p[2], t_threshold=got["verify"][4], d_threshold=got["d_thr"])
        sc = rs.lp_min_p(plan.t3, plan.d3, plan.n_acc, plan.r_commit, plan.bonus, inv_t, **kw)
        torch.cuda.synchronize()
        assert rs.status() == 0
        for b in seqs:
            assert bits(*[t[b:b + 1] for t in got["commit"]]) == bits(*[t[b:b + 1] for t in sc]), ("commit", p, b)
        if forced_residual:
            with K_.test_hooks() as lib:
                lib.asd_debug_residual_groups(-1)
                try:
                    rs2 = K_.ResidualSampler(n, V, tdt)
                    fr = rs2.lp_rows(plan.t3, plan.d3, plan.n_acc, plan.r_commit, plan.bonus, rows=got["table"],
                                     t_threshold=got["verify"][4], d_threshold=got["d_thr"])
                    fs = rs2.lp_min_p(plan.t3, plan.d3, plan.n_acc, plan.r_commit, plan.bonus, inv_t, **kw)
                    torch.cuda.synchronize()
                finally:
                    lib.asd_debug_residual_groups(0)
            assert rs2.status() == 0
            for b in seqs:
                assert bits(*[t[b:b + 1] for t in fr]) == bits(*[t[b:b + 1] for t in fs]), ("commit, forced form", p, b)
    # ---- bar 2, every sequence: one select for the draw, the verify and the bonus row
    lp_t, _, _, _, t_thr, n_fin = got["verify"]
    assert bits(t_thr) == bits(got["step_thr"])
    kept = (got["tok"] == got["drawn_tok"]).cpu().numpy()
    assert kept.sum() >= n * K - (n + 1) // 2
    assert lp_t.cpu().numpy()[kept].tobytes() == got["step_lp"].cpu().numpy()[kept].tobytes()
    for b in range(n):
        if not truncates(params[b], V):
            assert np.isneginf(t_thr[b].cpu().numpy()).all()
    # the bonus rows' thresholds: the [n] floats behind the part of the workspace asd_residual_sample_workspace_bytes sizes
    from asd_amd import _binding
    base = int(_binding.load_library().asd_residual_sample_workspace_bytes(n, V, plan.dtype))
    b_thr = got["rs"].buf[base:base + 4 * n].cpu().numpy().view(np.float32)
    bonus_seq = (plan.n_acc.cpu().numpy() == K)
    assert bonus_seq.any() and b_thr[bonus_seq].tobytes() == got["draft"][2].cpu().numpy()[bonus_seq].tobytes()
    ctok, clp = (t.cpu().numpy() for t in got["commit"])
    # (a kept set of one token: lp may sit a rounding above 0 where min-p is off, and reads as 0 where it is on)
    assert (ctok >= 0).all() and np.isfinite(clp).all() and (clp <= 1e-6).all()
    assert all(clp[b] <= 0.0 for b in range(n) if params[b][2] > 0.0)
    assert got["ds"].status() == 0 and got["rs"].status() == 0 and ws.status() == 0


@pytest.mark.parametrize("dtype,V", SHAPES)
def test_rows_are_the_scalar_calls_bit_for_bit(K_, dtype, V):
    plan = Plan(dtype, V)
    for params in (TABLE_A, table_b(V)):
        got = run_rows(K_, plan, params)
        check_against_scalar_calls(K_, plan, params, got, forced_residual=V != V_FULL or params is TABLE_A)


def test_rows_in_the_one_workgroup_commit_form(K_):
    """B = 96 is where the commit draw keeps a sequence in one workgroup (k_residual_row) once the group form is switched off."""
    import torch
    dtype, V, n = O.DT_BF16, 1000, 96
    plan = Plan(dtype, V, n_seq=n)
    params = [TABLE_A[b % 8] for b in range(n)]
    got = run_rows(K_, plan, params)
    tdt = plan.t3.dtype
    with K_.test_hooks() as lib:
        lib.asd_debug_residual_groups(-1)
        try:
            rs = K_.ResidualSampler(n, V, tdt)
            fr = rs.lp_rows(plan.t3, plan.d3, plan.n_acc, plan.r_commit, plan.bonus, rows=got["table"],
                            t_threshold=got["verify"][4], d_threshold=got["d_thr"])
            for p in TABLE_A:
                fs = rs.lp_min_p(plan.t3, plan.d3, plan.n_acc, plan.r_commit, plan.bonus, inv_t_of(p[3]), top_k=p[0], top_p=p[1],
                                 min_p=p[2], t_threshold=got["verify"][4], d_threshold=got["d_thr"])
                torch.cuda.synchronize()
                for b in range(n):
                    if params[b] == p:
                        assert bits(*[t[b:b + 1] for t in fr]) == bits(*[t[b:b + 1] for t in fs]), (p, b)
        finally:
            lib.asd_debug_residual_groups(0)
    assert rs.status() == 0 and got["rs"].status() == 0


@pytest.mark.parametrize("dtype,V", [(O.DT_BF16, 1000), (O.DT_F32, 4100), (O.DT_BF16, V_FULL)])
def test_top_logprobs_rows_is_the_scalar_call_per_sequence(K_, dtype, V):
    import torch
    plan = Plan(dtype, V)
    temps = [0.5, 0.7, 0.9, 1.0, 1.3, 2.0, 0.7, 0.5]
    inv = torch.tensor([inv_t_of(t) for t in temps], dtype=torch.float32, device="cuda")
    top = K_.TopLogprobs(B, K, V, plan.t3.dtype, n=5)
    view = plan.t3[:, :, :V]
    for splits in (0, 1, 3):
        ids, lps = (t.clone() for t in top(view, inv, splits))
        for b, t in enumerate(temps):
            sid, slp = top(view, inv_t_of(t), splits)
            assert bits(ids[b], lps[b]) == bits(sid[b], slp[b]), (splits, b)
    # [B, V] logits (stage 0's call)
    top1 = K_.TopLogprobs(B, 1, V, plan.t3.dtype, n=3)
    ids, lps = (t.clone() for t in top1(plan.bonus, inv))
    for b, t in enumerate(temps):
        sid, slp = top1(plan.bonus, inv_t_of(t))
        assert bits(ids[b], lps[b]) == bits(sid[b], slp[b]), b
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------- bar 3
UNTRUNCATED_TEMPS = [0.5, 0.7, 0.9, 1.0, 1.3, 2.0, 0.7, 1.0]


def untruncated_case(dtype, V):
    """numpy only: 24 Gaussian rows, tokens (the row's arg-max w.p. 0.7), draft log-probs near the target's at the sequence's
    own temperature, uniforms; and the f64 oracle run per sequence with that temperature."""
    rng = np.random.default_rng(4100 + V % 1000 + dtype)
    x = (rng.standard_normal((B * K, V)) * 4.0).astype(np.float32)
    store = encode_logits(x, dtype)
    xf = O.logits_as_f32(store, dtype)
    tok = np.where(rng.uniform(size=B * K) < 0.7, xf.argmax(1), rng.integers(0, V, B * K)).astype(np.int32).reshape(B, K)
    u = rng.uniform(0, 1, (B, K)).astype(np.float32)
    lp_d = np.empty((B, K), np.float32)
    ref = []
    for b, T in enumerate(UNTRUNCATED_TEMPS):
        rows = store[b * K:(b + 1) * K]
        base = O.verify_accept(rows, dtype, tok[b:b + 1], np.zeros((1, K), np.float32), np.full((1, K), 0.5, np.float32), 1, K, V,
                               inv_temperature=inv_t_of(T))
        lp_d[b] = np.minimum(base["lp_t64"].reshape(-1) + rng.normal(0, 0.5, K), 0.0).astype(np.float32)
        ref.append(O.verify_accept(rows, dtype, tok[b:b + 1], lp_d[b:b + 1], u[b:b + 1], 1, K, V, inv_temperature=inv_t_of(T)))
    return store, tok, lp_d, u, ref


@pytest.mark.parametrize("dtype,V", SHAPES)
def test_untruncated_sequences_of_the_verify_against_the_f64_oracle(K_, dtype, V):
    import torch
    store, tok, lp_d, u, ref = untruncated_case(dtype, V)
    margin = np.concatenate([r["margin"].reshape(-1) for r in ref])
    assert margin.shape == (B * K,) and (margin > 1e-5).all(), margin.min()      # no row is left out: asserted on the oracle alone
    lg = to_device_logits(store, dtype).view(B, K, V)
    tbl = K_.SamplingRows([inv_t_of(t) for t in UNTRUNCATED_TEMPS], V=V, dtype=lg.dtype)
    v = K_.verify_accept_rows(lg, torch.from_numpy(tok).cuda(), torch.from_numpy(lp_d).cuda(), torch.from_numpy(u).cuda(), tbl)
    torch.cuda.synchronize()
    lp_t, acc, n_acc, abits, thr, n_fin = (t.cpu().numpy() for t in (v.lp_target, v.accept, v.n_acc, v.accept_bits,
                                                                      v.t_nucleus_logit, v.n_finite))
    want_lp = np.concatenate([r["lp_t64"].reshape(1, K) for r in ref])
    worst = float(np.abs(lp_t.astype(np.float64) - want_lp).max())
    print(f"[per-request] untruncated verify rows, dtype {dtype} V {V}: max |lp_target - f64| = {worst:.3e}")
    assert worst <= 1e-5
    assert np.array_equal(acc, np.concatenate([r["accept"].reshape(1, K) for r in ref]))
    assert np.array_equal(n_acc, np.concatenate([r["n_acc"].reshape(-1) for r in ref]))
    assert np.isneginf(thr).all() and (n_fin == K).all()
    assert np.array_equal(abits.view(np.uint64), np.concatenate([r["bits"].reshape(-1) for r in ref]))
    # and the select's sweep-1 normaliser is asd_draft_sample's: the lp it reports for the token it draws on these rows
    ds = K_.DraftSampler(B, V, lg.dtype)
    r = torch.full((B,), 0.37, dtype=torch.float32, device="cuda")
    for k in range(K):
        d = ds.rows(lg[:, k].contiguous(), r, tbl)
        t1 = torch.from_numpy(tok).cuda().clone()
        t1[:, k] = d.tok
        v1 = K_.verify_accept_rows(lg, t1, torch.from_numpy(lp_d).cuda(), torch.from_numpy(u).cuda(), tbl)
        assert bits(v1.lp_target[:, k]) == bits(d.lp)
        for b, T in enumerate(UNTRUNCATED_TEMPS):                                  # ... which is the scalar draft's lp
            s = ds(lg[:, k].contiguous(), r, inv_t_of(T), 1.0)
            assert bits(s.lp[b:b + 1], s.thr[b:b + 1]) == bits(d.lp[b:b + 1], d.thr[b:b + 1])
    torch.cuda.synchronize()
    assert ds.status() == 0


# ---------------------------------------------------------------------------------------------------------- bar 4
@pytest.mark.parametrize("dtype,V", [(O.DT_BF16, 1000), (O.DT_F32, 1000), (O.DT_BF16, V_FULL)])
@pytest.mark.parametrize("p", [(50, 0.9, 0.1, 0.7), (0, 1.0, 0.3, 1.3)])
def test_a_uniform_table_is_the_scalar_min_p_entry_points(K_, dtype, V, p):
    import torch
    plan = Plan(dtype, V)
    got = run_rows(K_, plan, [p] * B)
    tdt = plan.t3.dtype
    inv_t = inv_t_of(p[3])
    assert bits(*got["draft"]) == bits(*scalar_draft(K_.DraftSampler(B, V, tdt), plan.bonus, plan.r_draft, p))
    sv = K_.verify_accept_min_p(plan.t3, got["tok"], got["lp_d"], plan.u, None, inv_temperature=inv_t, top_k=p[0], top_p=p[1],
                                min_p=p[2])
    assert bits(*got["verify"]) == bits(sv.lp_target, sv.accept, sv.n_acc, sv.accept_bits, sv.t_nucleus_logit, sv.n_finite)
    rs = K_.ResidualSampler(B, V, tdt)
    sc = rs.lp_min_p(plan.t3, plan.d3, plan.n_acc, plan.r_commit, plan.bonus, inv_t, top_k=p[0], top_p=p[1], min_p=p[2],
                     t_threshold=sv.t_nucleus_logit, d_threshold=got["d_thr"])
    assert bits(*got["commit"]) == bits(*sc)
    torch.cuda.synchronize()
    assert rs.status() == 0 and got["rs"].status() == 0 and got["ds"].status() == 0


# ---------------------------------------------------------------------------------------------------------- bar 5
def test_status_codes(K_):
    import torch
    from asd_amd import _binding
    lib = _binding.load_library()
    OK, INVALID, UNSUPPORTED, WORKSPACE, ALIGNMENT = 0, -1, -2, -3, -5
    V, dt = 1000, _binding.DTYPE_BF16
    plan = Plan(O.DT_BF16, V)
    tbl = table_of(K_, TABLE_A, V, plan.t3.dtype)
    ds, rs = K_.DraftSampler(B, V, plan.t3.dtype), K_.ResidualSampler(B, V, plan.t3.dtype)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")              # noqa: E731
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")            # noqa: E731
    tok, lp, thr = i32(B), f32(B), f32(B)

    def draft(logits=plan.bonus.data_ptr(), ld=V, dtype=dt, r=plan.r_draft.data_ptr(), n=B, v=V, rows=tbl.buf.data_ptr()):
        return lib.asd_draft_sample_rows(logits, ld, dtype, r, n, v, rows, tok.data_ptr(), lp.data_ptr(), thr.data_ptr(),
                                         ds.buf.data_ptr(), ds.bytes, None)
    assert draft(rows=None) == INVALID and draft(n=0) == OK and draft(n=0, rows=None) == OK and draft(n=-1) == INVALID
    assert draft(dtype=7) == UNSUPPORTED and draft(logits=None) == INVALID and draft(ld=V - 8) == INVALID
    assert draft(v=1001, ld=1001) == ALIGNMENT and draft(v=0) == INVALID
    tk, lpd, u = i32(B, K), f32(B, K), f32(B, K)
    lpt, acc, nacc, ab, tthr, nf = f32(B, K), torch.zeros((B, K), dtype=torch.uint8, device="cuda"), i32(B), \
        torch.zeros((B,), dtype=torch.int64, device="cuda"), f32(B, K), i32(B)

    def verify(logits=plan.t3.data_ptr(), dtype=dt, ld=V, n=B, k=K, v=V, rows=tbl.buf.data_ptr(), out=lpt.data_ptr()):
        return lib.asd_verify_accept_rows(logits, dtype, ld, tk.data_ptr(), lpd.data_ptr(), u.data_ptr(), n, k, v, rows, out,
                                          acc.data_ptr(), nacc.data_ptr(), ab.data_ptr(), tthr.data_ptr(), nf.data_ptr(), None, 0, None)
    assert verify(rows=None) == INVALID and verify(n=0) == OK and verify(k=0) == OK and verify(n=0, rows=None) == OK
    assert verify(k=65) == UNSUPPORTED and verify(dtype=7) == UNSUPPORTED and verify(out=None) == INVALID
    assert verify(v=1001, ld=1001) == ALIGNMENT and verify(n=-1) == INVALID
    tkn, clp = i32(B), f32(B)

    def commit(rows=tbl.buf.data_ptr(), n=B, t_thr=tthr.data_ptr(), lp_out=clp.data_ptr(), ws_bytes=rs.bytes, dtype=dt):
        return lib.asd_residual_sample_lp_rows(plan.t3.data_ptr(), V, plan.d3.data_ptr(), V, plan.bonus.data_ptr(), V, dtype,
                                               plan.n_acc.data_ptr(), plan.r_commit.data_ptr(), n, K, V, rows, t_thr, None,
                                               tkn.data_ptr(), lp_out, rs.buf.data_ptr(), ws_bytes, None)
    plain = int(lib.asd_residual_sample_workspace_bytes(B, V, dt))
    assert commit(rows=None) == INVALID and commit(lp_out=None) == INVALID and commit(n=0) == OK and commit(n=0, rows=None) == OK
    assert commit(t_thr=None) == INVALID and commit(ws_bytes=plain) == WORKSPACE and commit(dtype=7) == UNSUPPORTED
    top = K_.TopLogprobs(B, K, V, plan.t3.dtype, n=3)
    ids, lps = top.out

    def top_rows(inv=tbl.inv_t.data_ptr(), n=B, splits=0, nn=3):
        return lib.asd_top_logprobs_rows(plan.t3.data_ptr(), dt, K * V, V, n, K, V, inv, nn, splits, ids.data_ptr(), lps.data_ptr(),
                                         top.buf.data_ptr(), top.bytes, None)
    assert top_rows(inv=None) == INVALID and top_rows(n=0) == OK and top_rows(n=0, inv=None) == OK
    assert top_rows(splits=65) == UNSUPPORTED and top_rows(nn=9) == UNSUPPORTED and top_rows(nn=0) == INVALID
    # the Python wrappers refuse a table packed for another shape
    with pytest.raises(ValueError, match="packed for"):
        ds.rows(plan.bonus[:4], plan.r_draft[:4], tbl)
    with pytest.raises(ValueError, match="packed for"):
        K_.verify_accept_rows(plan.t3, tk, lpd, u, table_of(K_, TABLE_A, V + 8, plan.t3.dtype))
    torch.cuda.synchronize()
    assert ds.status() == 0 and rs.status() == 0
