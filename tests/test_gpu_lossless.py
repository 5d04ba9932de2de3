"""Statistical losslessness of the HIP draft / verify / commit chain: DraftSampler, verify_accept[_top_p / _top_k] and
ResidualSampler run back to back on fresh uniforms, and the histogram of the tokens they commit is held to the f64 target
distribution of tests/lossless.py -- which knows softmax(x_t / T) after top-k / top-p and nothing of the algorithm, the oracle
or DESIGN.md's residual.  The case tables, seeds and bookkeeping are those of tests/test_lossless.py (which proves them sound
on the CPU oracle and shows six injected defects failing at the same number of sequences).

The kernels' f32 arithmetic differs from the f64 reference by ~1e-6 relative; at <= 1e6 draws the statistical resolution is two
orders coarser, so no tolerance is added to the chi-square bound at 1e-6.  Histograms are accumulated on the device."""
import numpy as np
import pytest

from tests import lossless as L

pytestmark = pytest.mark.gpu

ROW_SEED, DRAW_SEED = 1, 2024          # tests/test_lossless.py checks the tables of ROW_SEED against the input conditions
PAD = 8                                # a padded row: stride V + 8 elements (16-bit rows stay 16-byte aligned), filled with +30


@pytest.fixture(scope="module")
def K_():
    from asd_amd import kernels
    return kernels


class TorchOps:
    """lossless.NumpyOps over CUDA tensors."""

    @staticmethod
    def arange(n):
        import torch
        return torch.arange(n, device="cuda", dtype=torch.int64)

    @staticmethod
    def i64(a):
        import torch
        return a.to(torch.int64)

    @staticmethod
    def where(c, a, b):
        import torch
        return torch.where(c, a, b)

    @staticmethod
    def bincount(keys, n):
        import torch
        return torch.bincount(keys, minlength=n)

    @staticmethod
    def to_numpy(a):
        return a.cpu().numpy()


class HipChain:
    """The backend of lossless.run_chain over the package's sampling entry points.  The logits stay on the device for the whole
    case: sequence b holds the rows of class b % R; only the uniforms change from call to call."""

    def __init__(self, K_, geom, route, dtype, xt, xd, pad=0):
        import torch
        self.K_, self.route = K_, route
        R, K, V, B = L.R_CLASSES, geom.K, geom.V, geom.B
        self.B, self.K, self.V = B, K, V
        tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dtype]
        cls = np.arange(B) % R

        def rows(x):                                   # x [n, V] f32 stored values -> device [n, V] view of [n, V + pad]
            full = np.full((x.shape[0], V + pad), 30.0, np.float32)
            full[:, :V] = x
            dev = torch.from_numpy(full).cuda().to(tdt)            # exact: the values already went through the dtype
            assert torch.equal(dev[:, :V].float().cpu(), torch.from_numpy(np.ascontiguousarray(x)))
            return dev[:, :V]
        self.t = rows(xt[cls, :K].reshape(B * K, V))
        self.d = rows(xd[cls].reshape(B * K, V))
        self.bonus = rows(xt[cls, K])
        ld = V + pad
        self.t3 = self.t.as_strided((B, K, V), (K * ld, ld, 1))
        self.d3 = self.d.as_strided((B, K, V), (K * ld, ld, 1))
        self.ds = K_.DraftSampler(B * K, V, tdt)
        self.ws = K_.VerifyWorkspace(B, K, V, tdt)
        self.rs = K_.ResidualSampler(B, V, tdt)

    def draft(self, r):
        import torch
        r = torch.from_numpy(r).cuda()
        ro = self.route
        if ro.family == "top_k":
            d = self.ds.top_k(self.d, r, L.INV_T, top_k=ro.d_top_k, top_p=ro.d_top_p)
        else:
            d = self.ds(self.d, r, L.INV_T, ro.d_top_p)
        truncated = ro.d_top_k > 0 or ro.d_top_p < 1.0
        return d.tok, d.lp, (d.thr.view(self.B, self.K) if truncated else None)

    def verify(self, tok, lp_d, u):
        import torch
        K_, ro = self.K_, self.route
        tok, lp_d, u = tok.view(self.B, self.K), lp_d.view(self.B, self.K), torch.from_numpy(u).cuda()
        if ro.family == "plain":
            return K_.verify_accept(self.t3, tok, lp_d, u, self.ws, inv_temperature=L.INV_T).n_acc, None
        if ro.family == "top_p":
            v = K_.verify_accept_top_p(self.t3, tok, lp_d, u, self.ws, inv_temperature=L.INV_T, top_p=ro.t_top_p)
        else:
            v = K_.verify_accept_top_k(self.t3, tok, lp_d, u, self.ws, inv_temperature=L.INV_T, top_k=ro.t_top_k, top_p=ro.t_top_p)
        return v.n_acc, v.t_nucleus_logit

    def residual(self, n_acc, r, d_thr, t_thr):
        import torch
        r = torch.from_numpy(r).cuda()
        ro = self.route
        if ro.family == "plain":
            return self.rs(self.t3, self.d3, n_acc, r, self.bonus, L.INV_T, d_threshold=d_thr)
        if ro.family == "top_p":
            return self.rs.top_p(self.t3, self.d3, n_acc, r, self.bonus, L.INV_T, top_p=ro.t_top_p, t_threshold=t_thr,
                                 d_threshold=d_thr)
        return self.rs.top_k(self.t3, self.d3, n_acc, r, self.bonus, L.INV_T, top_k=ro.t_top_k, top_p=ro.t_top_p,
                             t_threshold=t_thr, d_threshold=d_thr)


_ROWS = {}


def _rows(geom, dtype):
    key = (geom.V, dtype)
    if key not in _ROWS:
        _ROWS.clear()                                  # (one table at a time: the V = 152064 rows are 15 MB of f32 each)
        _ROWS[key] = L.make_rows(geom, dtype, ROW_SEED)
    return _ROWS[key]


def _run_case(K_, geom, route_name, dtype, label, pad=0):
    import torch
    route = L.ROUTES[route_name]
    xt, xd = _rows(geom, dtype)
    ref = L.reference(xt, xd, route)
    chain = HipChain(K_, geom, route, dtype, xt, xd, pad)
    counts = L.run_chain(chain, geom, DRAW_SEED, geom.V + PAD + 1, xp=TorchOps)
    torch.cuda.synchronize()
    assert chain.ds.status() == 0 and chain.rs.status() == 0 and chain.ws.status() == 0
    assert counts.n_seq == geom.B * geom.n_calls
    L.assert_lossless(L.evaluate(counts, ref), label)


@pytest.mark.parametrize("route_name,dtype", [("a", "bf16"), ("b", "bf16"), ("c", "bf16"), ("d", "bf16"), ("e", "bf16"),
                                              ("a", "f32"), ("d", "f32"), ("a", "f16"), ("d", "f16")])
def test_small_vocabulary_many_sequences(K_, route_name, dtype):
    """V = 512, B = 4096 per call: one workgroup per sequence (k_residual_row, k_draft_row); >= 2e5 sequences per route."""
    assert L.SMALL.B * L.SMALL.n_calls >= 200000
    _run_case(K_, L.SMALL, route_name, dtype, f"V 512 B 4096, route {route_name} {dtype}")


def test_small_vocabulary_padded_rows(K_):
    """Route c with a row stride of V + 8 on the target, draft and bonus tensors and +30.0 in the padding: a kernel that read
    across the stride would put mass on ids >= V (counted, and outside the support) or shift the histogram."""
    _run_case(K_, L.SMALL, "c", "bf16", "V 512 B 4096 padded rows, route c bf16", pad=PAD)


@pytest.mark.parametrize("route_name", ["c", "d", "e"])
def test_production_shape(K_, route_name):
    """V = 152064 bf16, B = 32, K = 2: a row spread over several workgroups (the group forms).  The truncated support is a few
    dozen tokens, so the histogram runs over the whole vocabulary: one draw anywhere else fails the case."""
    _run_case(K_, L.FULL, route_name, "bf16", f"V 152064 B 32, route {route_name} bf16")


def test_production_shape_padded_rows(K_):
    _run_case(K_, L.FULL, "c", "bf16", "V 152064 B 32 padded rows, route c bf16", pad=PAD)


@pytest.mark.parametrize("groups", [-1, 4])
def test_production_shape_forced_forms(K_, groups):
    """Route d at B = 32 through the test library's geometry switches: the three-launch residual form (-1) and 4 workgroups
    per sequence, the draft sampler's switch set alike."""
    with K_.test_hooks() as lib:
        try:
            lib.asd_debug_residual_groups(int(groups))
            lib.asd_debug_draft_groups(int(groups))
            _run_case(K_, L.FULL, "d", "bf16", f"V 152064 B 32 forced groups {groups}, route d bf16")
        finally:
            lib.asd_debug_residual_groups(0)
            lib.asd_debug_draft_groups(0)
