"""asd_top_logprobs and asd_commit_top_logprobs on the GPU against the numpy references of tests/top_logprobs_ref.py.  The
reference orders the stored values upcast to f32, which is exact, so the ids are compared EXACTLY in every row of every case;
the log-probs within 2e-5 (absolute) of f64, the project's tolerance for kernel log-probs at V = 152064.  Shapes are the
smallest at which each path of the kernel runs: the scalar head and tail (rows that start off a 16-byte boundary), more than
one batch per lane, slices without elements, every merge stage."""
import numpy as np
import pytest
import torch

from tests.top_logprobs_ref import LP_ATOL, ref_commit_top, ref_top_logprobs

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]


def strided(x, ld_row=None, extra_rows=0):
    """x [B, K1, V] on the CPU -> the same values on the GPU as a view with row stride ld_row and sequence stride
    (K1 + extra_rows) * ld_row; the padding holds +inf, which no result may show."""
    B, K1, V = x.shape
    ld_row = V if ld_row is None else ld_row
    buf = torch.full((B, K1 + extra_rows, ld_row), float("inf"), dtype=x.dtype, device="cuda")
    buf[:, :K1, :V] = x.cuda()
    return buf[:, :K1, :V]


def run_kernel(view, n, inv_t=1.0, splits=0):
    from asd_amd import kernels
    B, K1, V = view.shape
    top = kernels.TopLogprobs(B, K1, V, view.dtype, n)
    ids, lps = top(view, inv_t, splits)
    return ids.cpu().numpy(), lps.cpu().numpy()


def check(x, n, inv_t=1.0, splits=(0,), ld_row=None, extra_rows=0, what=""):
    """x [B, K1, V] CPU tensor of the kernel's dtype -> the ids of the first split count (all split counts give the same)."""
    want_id, want_lp = ref_top_logprobs(x.float().numpy(), n, inv_t)
    view = strided(x, ld_row, extra_rows)
    first = None
    for s in splits:
        got_id, got_lp = run_kernel(view, n, inv_t, s)
        assert got_id.dtype == np.int32 and got_lp.dtype == np.float32 and got_id.shape == want_id.shape == got_lp.shape
        assert np.array_equal(got_id, want_id), (what, s, np.argwhere(got_id != want_id)[:5], got_id[got_id != want_id][:5],
                                                 want_id[got_id != want_id][:5])
        got = got_lp.astype(np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want_lp)), (what, s)
        fin = np.isfinite(want_lp)
        err = np.abs(got[fin] - want_lp[fin]).max() if fin.any() else 0.0
        assert err <= LP_ATOL, (what, s, err)
        assert np.array_equal(got[~fin & ~np.isnan(want_lp)], want_lp[~fin & ~np.isnan(want_lp)]), (what, s)      # -inf exactly
        if first is None:
            first = (got_id, got_lp)
    return first


def randn(shape, dtype, seed, scale=4.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fewer_logits_than_slots(dtype):
    ids, lps = check(randn((2, 2, 3), dtype, 1), 5, splits=(0, 1, 2))
    assert (ids[..., 3:] == -1).all() and np.isneginf(lps[..., 3:]).all() and (ids[..., :3] >= 0).all()
    ids, lps = check(randn((3, 1, 1), dtype, 2), 5)
    assert (ids[..., 0] == 0).all() and (np.abs(lps[..., 0]) <= LP_ATOL).all() and (ids[..., 1:] == -1).all()


@pytest.mark.parametrize("n", [1, 5, 8])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unaligned_rows_every_split_count(dtype, n):
    """V = 1000 with an odd row stride: rows start off the 16-byte grid (scalar head and tail); 64 slices leave most empty."""
    x = randn((2, 3, 1000), dtype, 3)
    check(x, n, inv_t=1.0 / 0.7, splits=(1, 2, 7, 64), ld_row=1003, what="odd ld_row")
    check(x, n, splits=(1, 7), ld_row=1003, extra_rows=2, what="ld_seq > K1 ld_row")


def test_two_dimensional_logits_and_a_last_row_view():
    from asd_amd import kernels
    x = randn((3, 4, 1000), torch.bfloat16, 4).cuda()
    last = x[:, -1]                                        # [B, V] with the sequence stride of [B, 4, V]: what stage 0 hands over
    ids, lps = kernels.TopLogprobs(3, 1, 1000, torch.bfloat16, 5)(last)
    want_id, want_lp = ref_top_logprobs(last.float().cpu().numpy()[:, None], 5)
    assert ids.shape == (3, 1, 5) and np.array_equal(ids.cpu().numpy(), want_id)
    assert np.abs(lps.cpu().numpy() - want_lp).max() <= LP_ATOL


def test_largest_values_in_one_lane_and_in_one_vector():
    """V = 9004 bf16, rows on 16-byte boundaries (row stride 9008): lane 5 of a whole-row workgroup owns vectors 5 and 517 (ids
    40..47 and 4136..4143).  Row 0 has its 8 largest values spread over those two vectors, row 1 has them in ONE 16-byte vector,
    row 2 has its 4 largest in the scalar tail (ids 9000..9003)."""
    V = 9004
    x = randn((1, 3, V), torch.bfloat16, 5, scale=1.0)
    for j, i in enumerate([40, 42, 44, 46, 4137, 4139, 4141, 4143]):
        x[0, 0, i] = 20.0 + j
    for j in range(8):
        x[0, 1, 4136 + j] = 30.0 - j
    x[0, 2, 9000:9004] = torch.tensor([9.0, 9.5, 9.0, 9.5], dtype=torch.bfloat16)
    ids, _ = check(x, 8, splits=(1, 2, 3), ld_row=9008)
    assert sorted(ids[0, 0].tolist()) == [40, 42, 44, 46, 4137, 4139, 4141, 4143] and ids[0, 0, 0] == 4143
    assert ids[0, 1].tolist() == list(range(4136, 4144))
    assert ids[0, 2, :4].tolist() == [9001, 9003, 9000, 9002]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ties_go_to_the_lowest_id(dtype):
    x = torch.full((1, 3, 1000), 1.5, dtype=dtype)         # row 0: a constant row
    x[0, 1] = randn((1000,), dtype, 6)                      # row 1: equal maxima in different slices (7 slices of ~143)
    for i in (950, 20, 500, 300, 710):
        x[0, 1, i] = 50.0
    x[0, 2] = randn((1000,), dtype, 7)                      # row 2: two values, each many times over
    x[0, 2, 1::3] = 40.0
    x[0, 2, 2::5] = 41.0
    for ld in (1000, 1001):
        ids, lps = check(x, 8, splits=(1, 7, 64, 0), ld_row=ld)
        assert ids[0, 0].tolist() == list(range(8)) and np.abs(lps[0, 0] + np.log(1000.0)).max() < 1e-5
        assert ids[0, 1, :5].tolist() == [20, 300, 500, 710, 950]
        assert ids[0, 2].tolist() == [2, 7, 12, 17, 22, 27, 32, 37]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nan_and_minus_infinity_are_never_listed(dtype):
    x = randn((1, 4, 1000), dtype, 8)
    x[0, 0, ::2] = float("-inf")                            # row 0: -inf entries, finite log-probs
    x[0, 0, int(x[0, 0].float().argmax())] = float("-inf")
    x[0, 1, 5] = float("nan")                               # row 1: NaN entries, among them where the maximum was
    x[0, 1, int(torch.nan_to_num(x[0, 1].float(), nan=-1e9).argmax())] = float("nan")
    x[0, 1, 999] = float("nan")
    x[0, 2] = float("-inf")                                 # row 2: nothing to list
    x[0, 3] = float("-inf")                                 # row 3: three logits above -inf
    x[0, 3, [7, 600, 999]] = torch.tensor([1.0, 2.0, 1.0], dtype=dtype)
    for ld in (1000, 1001):
        ids, lps = check(x, 5, splits=(1, 2, 7), ld_row=ld)
        assert np.isfinite(lps[0, 0]).all() and not np.isin(ids[0, 0], np.arange(0, 1000, 2)).any()
        assert np.isnan(lps[0, 1]).all() and (ids[0, 1] >= 0).all() and not np.isin(ids[0, 1], [5, 999]).any()
        assert (ids[0, 2] == -1).all() and np.isneginf(lps[0, 2]).all()
        assert ids[0, 3].tolist() == [600, 7, 999, -1, -1]


def test_full_vocabulary_same_ids_in_every_geometry_and_slot_0_is_the_greedy_argmax():
    from asd_amd import kernels
    B, K1, V = 2, 3, 152064
    x = randn((B, K1, V), torch.bfloat16, 9)
    (ids, lps) = check(x, 5, inv_t=1.0 / 0.7, splits=(0, 8, 1))
    assert (ids >= 0).all() and (np.diff(lps, axis=-1) <= 0).all()
    view = x.cuda()
    tok = torch.randint(0, V, (B, K1 - 1), dtype=torch.int32).cuda()
    g = kernels.GreedyVerifier(B, K1 - 1, V, torch.bfloat16)(view, tok, 1.0 / 0.7)
    assert np.array_equal(g.argmax.cpu().numpy(), ids[..., 0])
    assert g.lp_argmax.cpu().numpy().tobytes() == np.ascontiguousarray(lps[..., 0]).tobytes()     # the same arithmetic, the same bits


def test_commit_scatter_bit_for_bit():
    from asd_amd import kernels
    g = torch.Generator().manual_seed(10)
    for B, K1, N, max_len in [(6, 5, 5, 16), (4, 1, 8, 9), (3, 9, 1, 12)]:
        top_id = torch.randint(-1, 1000, (B, K1, N), generator=g, dtype=torch.int32)
        top_lp = torch.randn((B, K1, N), generator=g)
        top_lp[0, 0, 0] = float("-inf")
        top_lp.view(torch.int32)[1, 0, 0] = 0x7FC12345      # a NaN with a payload: bits are copied
        n_commit = torch.randint(0, K1 + 1, (B,), generator=g, dtype=torch.int32)
        n_commit[0] = 0                                     # a finished sequence appends nothing
        n_commit[1] = K1
        seq_len = torch.randint(K1, max_len + 1, (B,), generator=g, dtype=torch.int32)
        seq_len[1] = max_len + 2                            # ... runs past max_len: the tail is not written
        seq_len[2] = max(int(n_commit[2]) - 1, 0)           # ... starts before position 0: the head is not written
        out_id = torch.randint(0, 9, (B, max_len, N), generator=g, dtype=torch.int32)
        out_lp = torch.randn((B, max_len, N), generator=g)
        want_id, want_lp = ref_commit_top(top_id.numpy(), top_lp.numpy(), seq_len.numpy(), n_commit.numpy(), out_id.numpy(),
                                          out_lp.numpy(), max_len)
        d_id, d_lp = out_id.cuda(), out_lp.cuda()
        kernels.commit_top_logprobs(top_id.cuda(), top_lp.cuda(), seq_len.cuda(), n_commit.cuda(), d_id, d_lp, max_len)
        assert np.array_equal(d_id.cpu().numpy(), want_id)
        assert d_lp.cpu().numpy().tobytes() == want_lp.tobytes()
