"""asd_token_stats on the GPU against tests/token_stats_ref.py::ref_token_stats on the same stored values.  The reference orders and
counts the stored values upcast to f32, which is exact, and ties go by id in both, so ranks and ids are compared EXACTLY on every
row of every case, none skipped; log-probs within LP_ATOL (2e-5 absolute); the entropy within 1e-4 + 1e-5 |H| (the bar
tests/test_gpu_verify.py holds the verify kernel's entropy to at V = 152064) and inside [-1e-5, ln V + 1e-4]; NaN and -inf
positions exactly.  Shapes are the smallest at which each path of the kernel runs, as in tests/test_gpu_prompt_logprobs.py."""
import numpy as np
import pytest
import torch

from tests.test_gpu_prompt_logprobs import DTYPES, IDS, INF, NAN, SPLITS, boundary_ids, randn, view_at
from tests.token_stats_ref import check_kernel_outputs, ref_token_stats
from tests.top_logprobs_ref import LP_ATOL

pytestmark = pytest.mark.gpu


def run_kernel(view, tok, n_acc, drawn, n, splits=0, inv_t=1.0):
    from asd_amd import kernels
    out = kernels.token_stats(view, tok, n_acc, drawn, n, inv_t, splits)
    assert (out[2] is None) == (out[3] is None) == (n == 0)
    return [None if t is None else t.cpu().numpy() for t in out]


def i32(v):
    return torch.as_tensor(np.asarray(v, dtype=np.int64).astype(np.int32), dtype=torch.int32).cuda()


def check(x, tok, n_acc, drawn, ns=(0, 1, 8), splits=SPLITS, off=0, what="", table_check=False, inv_t=1.0):
    """x [B, K1, V] CPU tensor of the kernel's dtype; tok int [B, K1 - 1] or None; n_acc, drawn: B ints.  Every (n, split count)
    against the reference; with table_check the tables and the arg-max pair against asd_top_logprobs at the same split count,
    bit for bit on every live row.  -> (stat_id, stat_val, top_id, top_lp) of the last launch."""
    from asd_amd import kernels
    B, K1, V = x.shape
    want = ref_token_stats(x.float().numpy(), tok, n_acc, drawn, max(ns), inv_t)
    view = view_at(x, off)
    d_tok = None if tok is None else i32(tok).reshape(B, K1 - 1)
    d_acc, d_drawn = i32(n_acc), i32(drawn)
    a = np.clip(np.asarray(n_acc, dtype=np.int64), 0, K1 - 1)
    live = np.arange(K1)[None, :] <= a[:, None]
    got, ranks = None, None
    for n in ns:
        for s in splits:
            tag = (what, n, s)
            got = stat_id, stat_val, top_id, top_lp = run_kernel(view, d_tok, d_acc, d_drawn, n, s, inv_t)
            assert stat_id.shape == stat_val.shape == (B, K1, 2)
            check_kernel_outputs(got, want, V, tag)
            assert ranks is None or np.array_equal(ranks, stat_id[..., 0]), tag      # the rank does not depend on the geometry
            ranks = stat_id[..., 0]
            assert (stat_id[~live] == [0, -1]).all() and (stat_val[~live] == 0.0).all(), tag
            if n:
                assert top_id.shape == top_lp.shape == (B, K1, n)
                assert (top_id[~live] == -1).all() and np.isneginf(top_lp[~live]).all(), tag
                assert np.array_equal(top_id[..., 0][live], stat_id[..., 1][live]), tag
                assert top_lp[..., 0][live].tobytes() == stat_val[..., 1][live].tobytes(), tag
                g = np.where(np.arange(K1)[None, :] < a[:, None], np.pad(np.zeros((B, 0)) if tok is None else np.asarray(tok),
                                                                          ((0, 0), (0, 1))), np.asarray(drawn)[:, None])
                for b, j in np.argwhere(live):                                       # rank <= n: the slot holds the target
                    r = stat_id[b, j, 0]
                    if 1 <= r <= n and top_id[b, j, r - 1] >= 0:
                        assert top_id[b, j, r - 1] == g[b, j], tag
                    elif r > n:
                        assert int(g[b, j]) not in top_id[b, j].tolist(), tag
            if table_check:                                                          # asd_top_logprobs' bits at the same split count
                m = max(n, 1)
                t_id, t_lp = (t.cpu().numpy() for t in kernels.TopLogprobs(B, K1, V, x.dtype, m)(view, inv_t, s))
                assert np.array_equal(t_id[..., 0][live], stat_id[..., 1][live]), tag
                assert t_lp[..., 0][live].tobytes() == stat_val[..., 1][live].tobytes(), tag
                if n:
                    assert np.array_equal(t_id[live], top_id[live]) and t_lp[live].tobytes() == top_lp[live].tobytes(), tag
    return got


@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unaligned_rows_every_split_count(dtype, off):
    """B = 2, K1 = 3, V = 4099 (odd: every row has its own misalignment, a scalar head and a tail), n_acc = [2, 1]: one skipped
    row, whose values are NaN (nothing of it may reach an output).  The targets walk the head, the tail and the first and last
    vectors of the slices."""
    B, K1, V = 2, 3, 4099
    x = randn((B, K1, V), dtype, 21)
    x[1, 2] = NAN
    ids = boundary_ids(V, 4 if dtype == torch.float32 else 8)
    ids += ids[:(-len(ids)) % (B * K1)]
    sets = np.asarray(ids).reshape(-1, B, K1)
    for k, g in enumerate(sets):
        kw = dict(table_check=True) if k == 0 else dict(ns=(0, 8))
        check(x, g[:, :2], [2, 1], g[:, 2], off=off, what=f"set {k}", **kw)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ties_go_by_id(dtype):
    """Blocks of 700 equal values straddle lanes, waves (64 lanes x 8 elements) and slices; a flat row has entropy ln V, max
    log-prob -ln V, arg-max 0 and rank = id + 1."""
    V = 4099
    x = torch.empty((2, 3, V), dtype=dtype)
    x[:, 0] = 1.5
    x[:, 1] = -(torch.arange(V) // 700).to(dtype)
    x[:, 2] = ((torch.arange(V) * 37) % 11).to(dtype)
    stat_id, stat_val, _, _ = check(x, [[2049, 350], [4098, 4098 - 100]], [2, 2], [5, 4090], off=1, what="ties", table_check=True)
    assert stat_id[0, 0].tolist() == [2050, 0] and stat_id[1, 0].tolist() == [4099, 0]
    assert stat_id[0, 1].tolist() == [351, 0] and stat_id[1, 1, 0] == 4099 - 100
    for b in range(2):
        assert abs(float(stat_val[b, 0, 0]) - np.log(V)) <= 1e-4 + 1e-5 * np.log(V) and abs(float(stat_val[b, 0, 1]) + np.log(V)) <= LP_ATOL
    stat_id, _, _, _ = check(x, [[0, 0], [1, 699]], [2, 2], [10, 0], off=3, ns=(8,), what="ties at the ends")
    assert stat_id[0, 0, 0] == 1 and stat_id[0, 1, 0] == 1 and stat_id[1, 1, 0] == 700
    assert stat_id[1, 2, 0] == V - int((x[1, 2] == 0).sum()) + 1 and stat_id[1, 2, 1] == int(np.argmax(x[1, 2].float().numpy()))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_special_values(dtype):
    from asd_amd.distributed import HipOps
    V = 1030
    x = randn((2, 3, V), dtype, 22)
    x[0, 0, ::3] = -INF
    x[0, 0, 1::3] = -INF                                   # a masked row, -inf on 2/3 of it: the entropy is over the survivors
    x[0, 1] = -INF
    x[0, 1, 7] = 0.25                                      # one finite value: entropy 0, max log-prob 0
    x[0, 2] = -INF                                         # no finite value: entropy NaN, arg-max (-1, -inf)
    x[1, 0, 100:140] = NAN                                 # NaN elements: entropy NaN, never counted, never listed
    x[1, 1, 517] = NAN                                     # a NaN target: rank 0
    stat_id, stat_val, top_id, _ = check(x, [[2, 7], [50, 517]], [2, 2], [9, 5], off=1, what="special")
    assert 0 < stat_val[0, 0, 0] <= np.log(V // 3 + 1) + 1e-4 and stat_id[0, 0, 0] >= 1
    assert -1e-5 <= stat_val[0, 1, 0] <= 1e-4 and abs(float(stat_val[0, 1, 1])) <= LP_ATOL and stat_id[0, 1].tolist() == [1, 7]
    assert np.isnan(stat_val[0, 2, 0]) and stat_id[0, 2, 1] == -1 and np.isneginf(stat_val[0, 2, 1]) and stat_id[0, 2, 0] == 10
    assert np.isnan(stat_val[1, 0, 0]) and stat_id[1, 0, 0] >= 1 and not (set(range(100, 140)) & set(top_id[1, 0].tolist()))
    assert np.isnan(stat_val[1, 1, 0]) and stat_id[1, 1, 0] == 0
    # targets outside the vocabulary on rows inside a larger allocation (the neighbours hold +inf): rank 0, the status words clean
    x = randn((2, 3, V), dtype, 23)
    tok, drawn = [[-1, V], [V + 7, -(1 << 31)]], [5, (1 << 31) - 1]
    stat_id, _, _, _ = check(x, tok, [2, 2], drawn, off=3, ns=(0, 8), what="outside")
    assert stat_id[..., 0].ravel().tolist()[:2] == [0, 0] and stat_id[0, 2, 0] >= 1 and (stat_id[1, :, 0] == 0).all()
    ops = HipOps()
    out = ops.token_stats(view_at(x, 3), torch.tensor(tok, dtype=torch.int32, device="cuda"),
                          torch.tensor([2, 2], dtype=torch.int32, device="cuda"), torch.tensor(drawn, dtype=torch.int32, device="cuda"), n=8)
    torch.cuda.synchronize()
    ops.check_status()
    assert np.array_equal(out[0].cpu().numpy(), stat_id)
    # n_acc of -1 and K1 + 5 are clamped: one live row, all live rows
    stat_id, _, _, _ = check(x, [[3, 4], [5, 6]], [-1, 3 + 5], [7, 8], off=1, ns=(0, 8), splits=(1, 3), what="clamped")
    assert (stat_id[0, 1:, 0] == 0).all() and (stat_id[..., 0] >= 1).sum() == 4


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_tiny_vocabulary_and_one_row(dtype):
    """V = 3 with N = 8: slots that cannot be filled; K1 = 1 with tok = None: a stage without a draft, [B, V] logits."""
    from asd_amd import kernels
    _, _, top_id, top_lp = check(randn((2, 3, 3), dtype, 24), [[0, 1], [2, 2]], [2, 2], [2, 0], off=1, what="V = 3")
    assert (top_id[..., 3:] == -1).all() and np.isneginf(top_lp[..., 3:]).all() and (top_id[..., :3] >= 0).all()
    x = randn((3, 1, 1030), dtype, 25)
    stat_id, _, _, _ = check(x, None, [0, 0, 0], [4, 1029, 77], off=3, what="K1 = 1", table_check=True)
    assert (stat_id[..., 0] >= 1).all()
    d = x.cuda()
    flat = kernels.token_stats(d[:, 0], None, i32([0, 0, 0]), i32([4, 1029, 77]), 2)              # [B, V] is taken too
    assert np.array_equal(flat[0].cpu().numpy(), stat_id)
    with pytest.raises(ValueError):
        kernels.token_stats(d, i32([[1], [2], [3]]), i32([0, 0, 0]), i32([4, 1029, 77]), 2)       # tok with K1 == 1
    with pytest.raises(ValueError):
        kernels.token_stats(d, None, i32([0, 0, 0]).to(torch.int64), i32([4, 1029, 77]), 2)
    with pytest.raises(ValueError):
        kernels.token_stats(d, None, i32([0, 0, 0]), i32([4, 1029, 77]), 9)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_per_row_temperatures(dtype):
    """inv_t_rows: every sequence returns the bits of the scalar call with its own value; and the values are the reference's."""
    B, K1, V = 3, 3, 4099
    x = randn((B, K1, V), dtype, 26)
    inv = [float(np.float32(1.0 / t)) for t in (0.7, 1.0, 1.9)]
    tok, n_acc, drawn = [[1, 2], [3, 4000], [5, 6]], [2, 1, 0], [4098, 17, 8]
    view, d_inv = view_at(x, 1), torch.tensor(inv, dtype=torch.float32, device="cuda")
    want = ref_token_stats(x.float().numpy(), tok, n_acc, drawn, 8, inv)
    for s in (1, 3, 64):
        rows = run_kernel(view, i32(tok), i32(n_acc), i32(drawn), 8, s, d_inv)
        check_kernel_outputs(rows, want, V, ("rows", s))
        for b in range(B):
            one = run_kernel(view, i32(tok), i32(n_acc), i32(drawn), 8, s, inv[b])
            for r, o in zip(rows, one):
                assert r[b].tobytes() == o[b].tobytes(), (s, b)


def test_full_vocabulary():
    """V = 152064, B = 2, K1 = 4, bf16, randn scale 4: whole rows, 4 and 64 slices."""
    B, K1, V = 2, 4, 152064
    x = randn((B, K1, V), torch.bfloat16, 27, scale=4.0)
    top = x[0, 0].float().argsort(descending=True, stable=True)
    tok, drawn = [[int(top[0]), int(top[3]), V - 1], [int(top[100]), 76032, int(top[-1])]], [0, 4097]
    stat_id, _, _, _ = check(x, tok, [3, 2], drawn, ns=(0, 5), splits=(1, 4, 64), off=1, what="V = 152064", table_check=True)
    assert stat_id[0, 0, 0] == 1 and stat_id[..., 0].max() > 1000 and stat_id[1, 3].tolist() == [0, -1]


def test_workspace():
    from asd_amd import _binding, kernels
    lib = _binding.load_library()
    q = lib.asd_token_stats_workspace_bytes
    assert q(32, 9, 152064, 1, 0) % 256 == 0 and q(0, 9, 152064, 1, 0) == 256 and q(2, 3, 4099, 1, 1) == 256
    B, K1, V = 2, 3, 4099
    x = view_at(randn((B, K1, V), torch.bfloat16, 28))
    tok, n_acc, drawn = i32(np.zeros((B, K1 - 1))), i32([2, 2]), i32([1, 2])
    stat_id = torch.empty((B, K1, 2), dtype=torch.int32, device="cuda")
    stat_val = torch.empty((B, K1, 2), dtype=torch.float32, device="cuda")
    for s in (0, 1, 2, 64):
        need = q(B, K1, V, 1, s)
        assert need % 256 == 0 and need == lib.asd_prompt_logprobs_workspace_bytes(B, K1, V, 1, s)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        args = lambda nbytes: (x.data_ptr(), 1, K1 * V, V, B, K1, V, tok.data_ptr(), K1 - 1, n_acc.data_ptr(), drawn.data_ptr(),   # noqa: E731
                               1.0, None, 0, s, stat_id.data_ptr(), stat_val.data_ptr(), None, None, ws.data_ptr(), nbytes,
                               torch.cuda.current_stream().cuda_stream)
        assert lib.asd_token_stats(*args(need - 1)) == -3                           # one byte less is refused
        assert lib.asd_token_stats(*args(need)) == 0
    torch.cuda.synchronize()
    assert kernels.TokenStats(B, K1, V, torch.bfloat16, 0, 64).bytes == q(B, K1, V, 1, 64)
