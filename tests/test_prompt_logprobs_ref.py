"""tests/prompt_logprobs_ref.py::ref_prompt_logprobs (numpy, f64; the reference every prompt log-prob test compares against)
against an independent formulation: torch.log_softmax in f64 for the log-probs and a STABLE descending sort for the ranks and the
table's ids, over random rows with planted ties, -inf and NaN."""
import numpy as np
import torch

from tests.prompt_logprobs_ref import ref_prompt_logprobs

B, T, V, N = 3, 6, 37, 8


def _rows():
    g = torch.Generator().manual_seed(5)
    x = torch.randn((B, T, V), generator=g).mul(3.0).bfloat16().float()          # few distinct values: natural ties as well
    x[0, 1, 5:20] = x[0, 1, 7]                                                   # a block of equal values
    x[0, 2] = 1.5                                                                # one repeated value
    x[1, 0, ::3] = float("-inf")
    x[1, 1, 4] = float("nan")                                                    # a NaN beside the target
    x[1, 2, 9] = float("nan")                                                    # ... and a NaN target (below)
    x[2, 3, :V - 2] = float("-inf")                                              # fewer than N listed
    target = torch.randint(0, V, (B, T), generator=g, dtype=torch.int32)
    target[0, 1], target[0, 2], target[1, 0], target[1, 2], target[2, 3] = 11, 18, 3, 9, V - 1
    target[2, 4], target[2, 5] = -1, V                                           # outside the vocabulary
    return x, target


def _independent(x, target, first, n):
    lp = np.zeros((B, T))
    rank = np.zeros((B, T), np.int32)
    top_id = np.full((B, T, n), -1, np.int32)
    top_lp = np.full((B, T, n), -np.inf)
    all_lp = torch.log_softmax(x.double(), dim=-1).numpy()
    for b in range(B):
        for t in range(T):
            if t < first[b]:
                continue
            row, g = x[b, t], int(target[b, t])
            live = torch.nonzero(~torch.isnan(row)).flatten()                    # a NaN is never counted or listed
            order = live[torch.sort(row[live], descending=True, stable=True).indices].tolist()
            listed = [v for v in order if row[v] > float("-inf")][:n]
            top_id[b, t, :len(listed)] = listed
            top_lp[b, t, :len(listed)] = all_lp[b, t, listed]
            if 0 <= g < V and g in order:
                lp[b, t], rank[b, t] = all_lp[b, t, g], order.index(g) + 1
            else:
                lp[b, t] = np.nan
    return lp, rank, top_id, top_lp


def test_reference_against_log_softmax_and_a_stable_sort():
    x, target = _rows()
    first = [0, 0, 2]
    for n in (0, 1, N):
        lp, rank, top_id, top_lp = ref_prompt_logprobs(x.numpy(), target.numpy(), first, n)
        w_lp, w_rank, w_id, w_top = _independent(x, target, first, n)
        assert np.array_equal(rank, w_rank) and np.array_equal(top_id, w_id)     # exact, on every row
        assert np.array_equal(np.isnan(lp), np.isnan(w_lp)) and np.array_equal(np.isneginf(lp), np.isneginf(w_lp))
        ok = np.isfinite(w_lp)
        assert np.abs(lp[ok] - w_lp[ok]).max() < 1e-12
        assert np.array_equal(np.isnan(top_lp), np.isnan(w_top)) and np.array_equal(np.isneginf(top_lp), np.isneginf(w_top))
        ok = np.isfinite(w_top)
        assert not ok.any() or np.abs(top_lp[ok] - w_top[ok]).max() < 1e-12
    # what the planted rows are there for
    assert rank[0, 2] == 18 + 1 and rank[0, 1] == 1 + int((x[0, 1] > x[0, 1, 11]).sum()) + (11 - 5)
    assert np.isneginf(lp[1, 0]) and rank[1, 0] == 1 + int((x[1, 0] > float("-inf")).sum()) + 1
    assert np.isnan(lp[1, 1]) and rank[1, 1] >= 1 and 4 not in top_id[1, 1]      # a NaN elsewhere: counted past, never listed
    assert np.isnan(lp[1, 2]) and rank[1, 2] == 0                                # a NaN target
    assert (top_id[2, 3] >= 0).sum() == 2 and rank[2, 3] in (1, 2)
    assert np.isnan(lp[2, 4]) and np.isnan(lp[2, 5]) and rank[2, 4] == rank[2, 5] == 0 and (top_id[2, 4] >= 0).all()
    assert (lp[2, :2] == 0).all() and (rank[2, :2] == 0).all() and (top_id[2, :2] == -1).all() and np.isneginf(top_lp[2, :2]).all()
