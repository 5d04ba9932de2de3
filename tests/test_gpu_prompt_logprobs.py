"""asd_prompt_logprobs on the GPU against tests/prompt_logprobs_ref.py::ref_prompt_logprobs on the same stored values.  The
reference orders and counts the stored values upcast to f32, which is exact, and ties go by id in both, so `rank` and `top_id`
are compared EXACTLY on every row of every case, none skipped; `lp` and `top_lp` within LP_ATOL (2e-5 absolute, the project's
tolerance for kernel log-probs against f64 up to V = 152064; NaN and -inf exactly).  Shapes are the smallest at which each path
of the kernel runs: the scalar head and tail, more than one batch per lane, slices without elements, every merge stage."""
import numpy as np
import pytest
import torch

from tests.prompt_logprobs_ref import ref_prompt_logprobs
from tests.top_logprobs_ref import LP_ATOL

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
SPLITS = (1, 2, 3, 7, 64)
NAN, INF = float("nan"), float("inf")


def view_at(x, off=0):
    """x [B, T, V] on the CPU -> the same values on the GPU as a contiguous view that starts `off` elements into a larger
    allocation; what surrounds it holds +inf, which no result may show."""
    buf = torch.full((x.numel() + 16,), INF, dtype=x.dtype, device="cuda")
    buf[off:off + x.numel()] = x.reshape(-1).cuda()
    return buf[off:off + x.numel()].view(x.shape)


def run_kernel(view, target, first, n, splits=0, inv_t=1.0):
    from asd_amd import kernels
    out = kernels.prompt_logprobs(view, target, first, n, inv_t, splits)
    assert (out[2] is None) == (out[3] is None) == (n == 0)
    return [None if t is None else t.cpu().numpy() for t in out]


def same_lp(got, want, what):
    got = got.astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    fin = np.isfinite(want)
    err = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    assert err <= LP_ATOL, (what, err)
    rest = ~fin & ~np.isnan(want)
    assert np.array_equal(got[rest], want[rest]), what                              # -inf (and the skipped rows' 0) exactly
    return err


def check(x, target, first=None, ns=(0, 1, 8), splits=SPLITS, off=0, what="", table_check=False):
    """x [B, T, V] CPU tensor of the kernel's dtype, target int [B, T], first: B ints or None.  Every (n, split count) against
    the reference; -> (lp, rank, top_id, top_lp) of the last launch, with rank equal across all of them."""
    from asd_amd import kernels
    B, T, V = x.shape
    target = torch.as_tensor(np.asarray(target), dtype=torch.int32).reshape(B, T)
    want = ref_prompt_logprobs(x.float().numpy(), target.numpy(), first, max(ns))
    view, d_target = view_at(x, off), target.cuda()
    d_first = None if first is None else torch.tensor(first, dtype=torch.int32, device="cuda")
    got = None
    for n in ns:
        for s in splits:
            tag = (what, n, s)
            got = lp, rank, top_id, top_lp = run_kernel(view, d_target, d_first, n, s)
            assert lp.dtype == np.float32 and rank.dtype == np.int32 and lp.shape == rank.shape == (B, T)
            assert np.array_equal(rank, want[1]), (tag, np.argwhere(rank != want[1])[:5], rank[rank != want[1]][:5],
                                                   want[1][rank != want[1]][:5])
            same_lp(lp, want[0], tag)
            if n:
                assert top_id.dtype == np.int32 and top_lp.dtype == np.float32 and top_id.shape == top_lp.shape == (B, T, n)
                assert np.array_equal(top_id, want[2][..., :n]), tag
                same_lp(top_lp, want[3][..., :n], tag)
                listed = (rank >= 1) & (rank <= n) & (lp > -INF)                    # a listed target carries its slot's bits
                for b, t in np.argwhere(listed):
                    assert top_id[b, t, rank[b, t] - 1] == target[b, t] and top_lp[b, t, rank[b, t] - 1].tobytes() == lp[b, t].tobytes(), tag
                for b, t in np.argwhere(~listed):
                    assert int(target[b, t]) not in top_id[b, t].tolist() or not lp[b, t] > -INF, tag
                if table_check and first is None and T <= 65:                       # asd_top_logprobs' bits at the same split count
                    t_id, t_lp = kernels.TopLogprobs(B, T, V, x.dtype, n)(view, 1.0, s)
                    assert np.array_equal(t_id.cpu().numpy(), top_id) and t_lp.cpu().numpy().tobytes() == top_lp.tobytes(), tag
    return got


def randn(shape, dtype, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=g) * scale).to(dtype)
    if dtype == torch.float32:                             # f32 draws do not tie by themselves: plant equal values
        x[..., 5::7] = x[..., 4::7][..., :x[..., 5::7].shape[-1]]
    return x


def boundary_ids(V, per):
    """Ids at which a row of V elements changes hands: the scalar head and tail, and the first and last 16-byte vectors of the
    first, second and last slice at every split count of SPLITS, whatever the row's misalignment (head < per)."""
    ids = set(range(0, 2 * per + 2)) | set(range(V - 2 * per - 2, V))
    nvec = V // per
    for s in SPLITS[1:]:
        for k in (1, s - 1):
            c = (nvec * k // s) * per
            ids |= set(range(c - per - 1, c + 2 * per + 1))
    return sorted(i for i in ids if 0 <= i < V)


@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unaligned_rows_every_split_count(dtype, off):
    """B = 2, T = 3, V = 4099 (odd: every row has its own misalignment, a scalar head and a tail); the target walks the head, the
    tail and the first and last vectors of the slices.  The tables have asd_top_logprobs' bits at every split count."""
    B, T, V = 2, 3, 4099
    x = randn((B, T, V), dtype, 11)
    ids = boundary_ids(V, 4 if dtype == torch.float32 else 8)
    ids += ids[:(-len(ids)) % (B * T)]
    sets = np.asarray(ids).reshape(-1, B, T)
    check(x, sets[0], off=off, what="first set", table_check=True)
    for k, target in enumerate(sets[1:]):                 # the other target sets: every split count, the widest table and none
        check(x, target, ns=(0, 8), off=off, what=f"set {k + 1}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ties_go_by_id(dtype):
    """One repeated value with the target in its middle: rank = target + 1.  Blocks of 700 equal values straddle lanes, waves
    (64 lanes x 8 elements) and slices; the target holds the row's maximum (first block) and its minimum (last block)."""
    V = 4099
    x = torch.empty((2, 3, V), dtype=dtype)
    x[:, 0] = 1.5
    x[:, 1] = -(torch.arange(V) // 700).to(dtype)
    x[:, 2] = ((torch.arange(V) * 37) % 11).to(dtype)      # eleven values, interleaved
    target = [[2049, 350, 5], [4098, 4098 - 100, 4090]]
    _, rank, _, _ = check(x, target, off=1, what="ties")
    assert rank[0, 0] == 2050 and rank[1, 0] == 4099 and rank[0, 1] == 351 and rank[1, 1] == 4099 - 100
    target = [[0, 0, 10], [1, 699, 0]]                     # the maximum's first holder, the minimum's (x[:, 2, 0] == 0)
    _, rank, _, _ = check(x, target, off=3, ns=(8,), what="ties at the ends")
    assert rank[0, 0] == 1 and rank[0, 1] == 1 and rank[1, 1] == 700 and rank[1, 2] == V - int((x[1, 2] == 0).sum()) + 1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_special_values(dtype):
    V = 1030
    x = randn((2, 3, V), dtype, 12)
    x[0, 0, ::3] = -INF                                    # a -inf target: lp -inf, rank by the order (ties among -inf by id)
    x[0, 1, 100:140] = NAN                                 # NaN elsewhere: never counted, never listed; the row's lp is NaN
    x[0, 2, 517] = NAN                                     # a NaN target: lp NaN, rank 0
    x[1, 0] = -INF
    x[1, 0, 7] = 0.25                                      # one finite value: its lp is 0 (within LP_ATOL) ...
    x[1, 1] = -INF
    x[1, 1, 7] = 0.25                                      # ... and -inf, rank 2 + (ids below), for a -inf target beside it
    target = [[9, 50, 517], [7, 600, V - 1]]
    lp, rank, top_id, _ = check(x, target, off=1, what="special")
    assert np.isneginf(lp[0, 0]) and rank[0, 0] == 1 + int((x[0, 0] > -INF).sum()) + 3
    assert np.isnan(lp[0, 1]) and rank[0, 1] >= 1 and not (set(range(100, 140)) & set(top_id[0, 1].tolist()))
    assert np.isnan(lp[0, 2]) and rank[0, 2] == 0
    assert abs(float(lp[1, 0])) <= LP_ATOL and rank[1, 0] == 1 and np.isneginf(lp[1, 1]) and rank[1, 1] == 2 + 599
    assert top_id[1, 0].tolist() == [7] + [-1] * 7
    # V = 3 with N = 8: slots that cannot be filled
    lp, rank, top_id, top_lp = check(randn((2, 3, 3), dtype, 13), [[0, 1, 2], [2, 2, 0]], off=1, what="V = 3")
    assert (top_id[..., 3:] == -1).all() and np.isneginf(top_lp[..., 3:]).all() and (top_id[..., :3] >= 0).all()
    assert ((rank >= 1) & (rank <= 3)).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_skipped_rows_are_neutral_and_never_read(dtype):
    T, V = 3, 1030
    x = randn((3, T, V), dtype, 14)
    first = [0, 2, T]
    for b, f in enumerate(first):
        x[b, :f] = NAN                                     # nothing of a skipped row reaches an output
    target = torch.randint(0, V, (3, T), generator=torch.Generator().manual_seed(1))
    lp, rank, top_id, top_lp = check(x, target, first, off=3, what="first")
    for b, f in enumerate(first):
        assert (lp[b, :f] == 0).all() and (rank[b, :f] == 0).all() and (top_id[b, :f] == -1).all() and np.isneginf(top_lp[b, :f]).all()
        assert (rank[b, f:] >= 1).all() and np.isfinite(lp[b, f:]).all()
    x = randn((3, T, V), dtype, 14)
    _, rank, _, _ = check(x, target, None, ns=(8,), splits=(1, 3), what="first = NULL")          # scores every row
    assert (rank >= 1).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_target_ids_outside_the_vocabulary(dtype):
    """Ids -1 and V on rows that lie inside a larger allocation (the neighbours hold +inf): never dereferenced -- lp NaN, rank 0,
    the table still right -- and the status words stay clean."""
    from asd_amd.distributed import HipOps
    V = 1030
    x = randn((2, 3, V), dtype, 15)
    target = [[-1, V, 5], [V + 7, -(1 << 31), (1 << 31) - 1]]
    lp, rank, top_id, _ = check(x, target, off=3, what="outside")
    assert np.isnan(lp).sum() == 5 and (rank.ravel()[[0, 1, 3, 4, 5]] == 0).all() and rank[0, 2] >= 1 and (top_id >= 0).all()
    ops = HipOps()
    out = ops.prompt_logprobs(view_at(x, 3), torch.tensor(target, dtype=torch.int32, device="cuda"), None, 8)
    torch.cuda.synchronize()
    ops.check_status()
    assert np.array_equal(out[1].cpu().numpy(), rank) and np.array_equal(out[2].cpu().numpy(), top_id)


def test_no_65_row_limit():
    g = torch.Generator().manual_seed(16)
    for (B, T, V), splits in (((1, 300, 64), (0, 1, 2)), ((3, 70, 257), (2,))):
        x = randn((B, T, V), torch.bfloat16, 17)
        check(x, torch.randint(0, V, (B, T), generator=g), ns=(0, 5), splits=splits, off=1, what=f"T = {T}")
        first = [T // 2] * B
        check(x, torch.randint(0, V, (B, T), generator=g), first, ns=(5,), splits=splits[-1:], what=f"T = {T}, first")


def test_strided_views_are_read_in_place():
    """What the stages hand over: rows [:, :P-1] of a [B, P, V] tensor and the view ids32[:, 1:]."""
    from asd_amd import kernels
    B, P, V = 3, 6, 1000
    full = randn((B, P, V), torch.bfloat16, 18)
    ids = torch.randint(0, V, (B, P), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    first = [0, 3, 1]
    want = ref_prompt_logprobs(full[:, :P - 1].float().numpy(), ids[:, 1:].numpy(), first, 4)
    d_full, d_ids = full.cuda(), ids.cuda()
    lp, rank, top_id, top_lp = (t.cpu().numpy() for t in kernels.prompt_logprobs(d_full[:, :P - 1], d_ids[:, 1:],
                                                                                 torch.tensor(first, dtype=torch.int32, device="cuda"), 4))
    assert np.array_equal(rank, want[1]) and np.array_equal(top_id, want[2])
    same_lp(lp, want[0], "view")
    same_lp(top_lp, want[3], "view")
    with pytest.raises(ValueError):
        kernels.prompt_logprobs(d_full[:, :P - 1], d_ids[:, 1:].to(torch.int64), None, 4)
    with pytest.raises(ValueError):
        kernels.prompt_logprobs(d_full[:, :P - 1], d_ids, None, 4)
    with pytest.raises(ValueError):
        kernels.prompt_logprobs(d_full[:, :P - 1].transpose(1, 2), d_ids[:, 1:], None, 4)
    with pytest.raises(ValueError):
        kernels.prompt_logprobs(d_full[:, :P - 1], d_ids[:, 1:], None, 9)


def test_full_vocabulary():
    """V = 152064, B = 2, T = 4, bf16: whole rows, 4 and 64 slices; ids and ranks are equal in every geometry."""
    B, T, V = 2, 4, 152064
    x = randn((B, T, V), torch.bfloat16, 19, scale=4.0)
    top = x[0, 0].float().argsort(descending=True, stable=True)
    target = [[int(top[0]), int(top[3]), V - 1, 0], [int(top[100]), 76032, int(top[-1]), 4097]]
    lp, rank, _, _ = check(x, target, ns=(0, 5), splits=(1, 4, 64), off=1, what="V = 152064", table_check=True)
    assert rank[0, 0] == 1 and rank.max() > 1000


def test_workspace():
    from asd_amd import _binding, kernels
    lib = _binding.load_library()
    q = lib.asd_prompt_logprobs_workspace_bytes
    assert q(32, 2047, 152064, 1, 0) < (1 << 20) and q(32, 2047, 152064, 1, 0) % 256 == 0
    B, T, V = 2, 3, 4099
    x = view_at(randn((B, T, V), torch.bfloat16, 20))
    target = torch.zeros((B, T), dtype=torch.int32, device="cuda")
    lp = torch.empty((B, T), dtype=torch.float32, device="cuda")
    rank = torch.empty((B, T), dtype=torch.int32, device="cuda")
    for s in (0, 1, 2, 64):
        need = q(B, T, V, 1, s)
        assert need % 256 == 0
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        args = lambda nbytes: (x.data_ptr(), 1, T * V, V, B, T, V, target.data_ptr(), T, None, 1.0, 0, s, lp.data_ptr(),   # noqa: E731
                               rank.data_ptr(), None, None, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        assert lib.asd_prompt_logprobs(*args(need - 1)) == -3                       # one byte less is refused
        assert lib.asd_prompt_logprobs(*args(need)) == 0
    torch.cuda.synchronize()
    assert kernels.PromptLogprobs(B, T, V, torch.bfloat16, 0, 64).bytes == q(B, T, V, 1, 64)
