"""tests/entropy_cut_ref.py's ref_entropy_cut against transformers' TypicalLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper
behind TemperatureLogitsWarper (min_tokens_to_keep = 1), in f64 and f32: the kept sets are equal outside the boundary window.
And the documented order: the reference followed by HF's TopK, TopP and MinP equals HF's own classes chained Temperature ->
Typical -> TopK -> TopP -> MinP.  CPU only."""
import numpy as np
import pytest
import torch

from tests.entropy_cut_ref import EPSILON, ETA, OFF, TYPICAL, assert_cap, cut_row, ref_entropy_cut

T = 0.7
INV_T = float(np.float32(1.0 / T))
ROWS = 40


def _logits(V, seed):
    return (np.random.default_rng(seed).standard_normal((ROWS, V)) * 3.0).astype(np.float32)


def _warper(mode, value):
    from transformers.generation.logits_process import EpsilonLogitsWarper, EtaLogitsWarper, TypicalLogitsWarper
    if mode == TYPICAL:
        return TypicalLogitsWarper(mass=value)
    if mode == EPSILON:
        return EpsilonLogitsWarper(epsilon=value)
    return EtaLogitsWarper(epsilon=value, device="cpu")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("V", [64, 1000])
@pytest.mark.parametrize("mode,value", [(TYPICAL, 0.2), (TYPICAL, 0.9), (TYPICAL, 0.95), (EPSILON, 0.01), (EPSILON, 3e-4),
                                        (ETA, 0.02), (ETA, 0.5)])
def test_kept_sets_equal_transformers_outside_the_window(mode, value, V, dtype):
    from transformers.generation.logits_process import TemperatureLogitsWarper
    x = _logits(V, seed=V + mode)
    value = float(np.float32(value))
    keep, thr, und, touched = ref_entropy_cut(x, [(INV_T, mode, value)] * ROWS)
    assert touched.all() and keep.any(axis=1).all()
    assert_cap(und)
    scores = TemperatureLogitsWarper(1.0 / INV_T)(None, torch.from_numpy(x).to(dtype))
    out = _warper(mode, value)(None, scores)
    hf_keep = ~torch.isinf(out).numpy()
    assert np.array_equal(hf_keep[~und], keep[~und])
    assert (hf_keep.sum(axis=1) < V).any()                                   # the warper is live on these inputs


def test_documented_order_is_typical_then_top_k_top_p_min_p():
    from transformers.generation.logits_process import (LogitsProcessorList, MinPLogitsWarper, TemperatureLogitsWarper,
                                                        TopKLogitsWarper, TopPLogitsWarper, TypicalLogitsWarper)
    V, m = 1000, float(np.float32(0.9))
    x = _logits(V, seed=5)
    tail = lambda: [TopKLogitsWarper(top_k=20), TopPLogitsWarper(top_p=0.8), MinPLogitsWarper(min_p=0.05)]   # noqa: E731
    hf = LogitsProcessorList([TemperatureLogitsWarper(1.0 / INV_T), TypicalLogitsWarper(mass=m)] + tail())(
        None, torch.from_numpy(x).double())
    keep, _, und, _ = ref_entropy_cut(x, [(INV_T, TYPICAL, m)] * ROWS)
    assert not und.any()
    ours = torch.from_numpy(np.where(keep, x, -np.inf)).double()
    ours = LogitsProcessorList([TemperatureLogitsWarper(1.0 / INV_T)] + tail())(None, ours)
    assert torch.equal(torch.isinf(ours), torch.isinf(hf))
    # and it is NOT HF's generate order (Temperature -> TopK -> TopP -> MinP -> Typical) on these rows
    late = LogitsProcessorList([TemperatureLogitsWarper(1.0 / INV_T)] + tail() + [TypicalLogitsWarper(mass=m)])(
        None, torch.from_numpy(x).double())
    assert not torch.equal(torch.isinf(late), torch.isinf(hf))


def test_designed_rows():
    V = 64
    # p_0 = 0.3 over a uniform tail, small m: the arg-max is cut, the tail survives
    row = np.zeros(V, np.float32)
    row[0] = np.log(0.3 / (0.7 / (V - 1)))
    r = cut_row(row, 1.0, TYPICAL, 0.2)
    assert not r.keep[0] and r.keep[1:].all() and not r.undecided.any()
    # a flat row: every key is 0, everything is kept; epsilon 0.5: every token ties the maximum
    flat = np.full(V, 1.5, np.float32)
    for mode, value in ((TYPICAL, 0.3), (EPSILON, 0.5), (ETA, 0.5)):
        r = cut_row(flat, INV_T, mode, value)
        assert r.keep.all() and not r.undecided.any() and r.touched
    # m so close to 1 that the mass reaches it with the last token at the earliest, or never: everything is kept
    x = _logits(V, 9)[0]
    r = cut_row(x * 0.05, INV_T, TYPICAL, float(np.float32(1.0 - 2.0 ** -24)))
    assert r.keep.all()
    # one finite value; no finite value; a NaN; +inf; off
    one = np.full(V, -np.inf, np.float32)
    one[7] = 2.0
    assert cut_row(one, INV_T, TYPICAL, 0.5).keep.all() and cut_row(one, INV_T, EPSILON, 0.5).touched
    for bad in (np.full(V, -np.inf, np.float32), np.where(np.arange(V) == 3, np.nan, x), np.where(np.arange(V) == 3, np.inf, x)):
        assert not cut_row(bad, INV_T, TYPICAL, 0.5).touched
    assert not cut_row(x, INV_T, OFF, 0.0).touched
    # eta: sqrt(e) exp(-H) is the smaller term on a flat-ish row, e on a peaked one
    wide, peaked = x * 0.05, x * 3.0
    for row, smaller in ((wide, True), (peaked, False)):
        e = 0.02
        z = row.astype(np.float64) * INV_T
        p = np.exp(z - z.max()) / np.exp(z - z.max()).sum()
        H = -(p * np.log(p)).sum()
        assert (np.sqrt(e) * np.exp(-H) < e) == smaller
        r = cut_row(row, INV_T, ETA, e)
        assert abs(r.thr - min(e, np.sqrt(e) * np.exp(-H))) < 1e-9
        assert np.array_equal(r.keep[~r.undecided], ((p >= r.thr) | (row == row.max()))[~r.undecided])
