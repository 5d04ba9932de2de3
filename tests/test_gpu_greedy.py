"""asd_verify_greedy on the GPU against the numpy f64 reference (tests/greedy_ref.py): arg-max / accept / n_acc / drawn EXACT
for every row and every split count (the stored values are compared, so there are no near-ties to excuse), the log-probs within
the project's bar (tests/helpers.py LP_ATOL / LP_RTOL) of f64, lp_target's bits those of lp_argmax where accepted, the same call
twice the same bits; strides and misaligned bases, ties, NaN / all -inf rows, prefix patterns, a shared workspace."""
import functools

import numpy as np
import pytest
import torch

from tests.greedy_ref import ref_argmax, ref_verify_greedy
from tests.helpers import LP_ATOL, LP_RTOL

pytestmark = pytest.mark.gpu

SHAPES = [(1, 0, 1), (3, 0, 257), (2, 4, 1000), (5, 8, 4173), (2, 1, 152064)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SPLITS = (0, 1, 2, 3, 7, 16)
OUTS = ("argmax", "lp_argmax", "lp_target", "accept", "n_acc", "drawn", "lp_drawn")


@functools.lru_cache(maxsize=None)
def make_case(B, K, V, dtype, seed=7):
    """(logits [B,K+1,V] of `dtype` on the CPU, tok [B,K] i32: the row's arg-max w.p. 0.6, else any id)."""
    g = torch.Generator().manual_seed(seed + 1000 * B + 10 * K + V)
    x = (torch.randn((B, K + 1, V), generator=g) * 4.0).to(dtype)
    am = x[:, :K].float().argmax(-1)
    rnd = torch.randint(0, V, (B, K), generator=g)
    tok = torch.where(torch.rand((B, K), generator=g) < 0.6, am, rnd).to(torch.int32)
    return x, tok


def reference(x, tok, inv_t=1.0):
    return ref_verify_greedy(x.float().numpy(), None if tok.shape[1] == 0 else tok.numpy(), inv_t)


def run(verifier, x_dev, tok, inv_t=1.0, splits=0):
    r = verifier(x_dev, None if tok.shape[1] == 0 else tok.cuda(), inv_t, splits)
    return {k: getattr(r, k).cpu().numpy() for k in OUTS}


def assert_lp(got, want, what):
    got = got.astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=LP_RTOL, atol=LP_ATOL, err_msg=what)
    inf = ~fin & ~np.isnan(want)
    assert np.array_equal(got[inf], want[inf]), what                  # +-inf exactly


def assert_matches(got, ref, what=""):
    for k in ("argmax", "accept", "n_acc", "drawn"):                  # exact, every row
        assert np.array_equal(got[k], ref[k]), (what, k, got[k], ref[k])
    for k in ("lp_argmax", "lp_target", "lp_drawn"):
        assert_lp(got[k], ref[k], (what, k))
    acc = got["accept"].astype(bool)
    K = acc.shape[1]
    assert np.array_equal(got["lp_target"].view(np.uint32)[acc], got["lp_argmax"][:, :K].view(np.uint32)[acc]), what


def verifier_for(B, K, V, dtype):
    from asd_amd import kernels
    return kernels.GreedyVerifier(B, K, V, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matches_the_f64_reference_for_every_split_count(shape, dtype):
    B, K, V = shape
    x, tok = make_case(B, K, V, dtype)
    ref = reference(x, tok)
    v = verifier_for(B, K, V, dtype)
    xd = x.cuda()
    for splits in SPLITS:
        got = run(v, xd, tok, splits=splits)
        assert_matches(got, ref, f"splits={splits}")
        again = run(v, xd, tok, splits=splits)                        # the same call twice: identical bits
        for k in OUTS:
            assert got[k].tobytes() == again[k].tobytes(), (splits, k)


def test_a_slice_without_elements_is_neutral():
    B, K, V = 2, 3, 5
    for dtype in DTYPES:
        x, tok = make_case(B, K, V, dtype)
        assert_matches(run(verifier_for(B, K, V, dtype), x.cuda(), tok, splits=8), reference(x, tok), str(dtype))


def test_other_temperatures():
    B, K, V = 2, 4, 1000
    x, tok = make_case(B, K, V, torch.bfloat16)
    inv_t = float(np.float32(1.0 / 0.7))
    assert_matches(run(verifier_for(B, K, V, torch.bfloat16), x.cuda(), tok, inv_t=inv_t), reference(x, tok, inv_t))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_padded_strides_and_a_misaligned_base(dtype):
    B, K, V = 5, 8, 4173
    x, tok = make_case(B, K, V, dtype)
    ref = reference(x, tok)
    v = verifier_for(B, K, V, dtype)
    ld_row = V + 3
    ld_seq = (K + 1) * ld_row + 5
    for offset in (0, 1):                                             # the base offset by one element: no row is 16-byte aligned
        buf = torch.full((offset + B * ld_seq,), 1.0e4, dtype=dtype, device="cuda")      # the padding must never be read as vocabulary
        view = buf[offset:].as_strided((B, K + 1, V), (ld_seq, ld_row, 1))
        view.copy_(x.cuda())
        for splits in (0, 1, 3):
            assert_matches(run(v, view, tok, splits=splits), ref, f"offset={offset} splits={splits}")
    # ... and a contiguous tensor whose base is off by one element
    buf = torch.empty((1 + x.numel(),), dtype=dtype, device="cuda")
    view = buf[1:].view(B, K + 1, V)
    view.copy_(x.cuda())
    assert_matches(run(v, view, tok), ref, "contiguous, base + 1")


def test_ties_go_to_the_lowest_id():
    B, K, V = 2, 1, 4173
    x, tok = make_case(B, K, V, torch.bfloat16)
    x = x.clone()
    x[0, 0, [V - 1, 17, V // 2]] = 50.0
    x[1, 1, [V - 1, V // 2]] = 50.0
    tok = tok.clone()
    tok[0, 0] = 17
    ref = reference(x, tok)
    assert ref["argmax"][0, 0] == 17 and ref["argmax"][1, 1] == V // 2 and ref["n_acc"][0] == 1
    v = verifier_for(B, K, V, torch.bfloat16)
    for splits in SPLITS:
        got = run(v, x.cuda(), tok, splits=splits)
        assert got["argmax"][0, 0] == 17 and got["argmax"][1, 1] == V // 2, splits
        assert_matches(got, ref, f"splits={splits}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_nan_never_wins_and_an_all_minus_inf_row_gives_minus_one(dtype):
    B, K, V = 3, 4, 1000
    x, tok = make_case(B, K, V, dtype)
    x, tok = x.clone(), tok.clone()
    first = int(ref_argmax(x[0, 2].float().numpy()))
    x[0, 2, first] = float("nan")                                     # a NaN at the would-be maximum: the next id wins
    second = int(ref_argmax(x[0, 2].float().numpy()))
    x[1, 1] = float("-inf")                                           # nothing above -inf: argmax = -1, lp = NaN
    tok[1, 0] = int(ref_argmax(x[1, 0].float().numpy()))                         # ... and the sequence's prefix ends AT that row
    ref = reference(x, tok)
    assert ref["argmax"][0, 2] == second != first and ref["argmax"][1, 1] == -1
    assert ref["n_acc"][1] == 1 and ref["drawn"][1] == -1 and np.isnan(ref["lp_drawn"][1]) and ref["accept"][1, 1] == 0
    v = verifier_for(B, K, V, dtype)
    for splits in (0, 1, 3, 16):
        got = run(v, x.cuda(), tok, splits=splits)
        assert got["argmax"][0, 2] == second and got["argmax"][1, 1] == got["drawn"][1] == -1 and got["accept"][1, 1] == 0
        assert np.isnan(got["lp_argmax"][1, 1]) and np.isnan(got["lp_drawn"][1])
        assert_matches(got, ref, f"splits={splits}")                  # the other rows and sequences are untouched by it


def test_prefix_patterns():
    B, K, V = 5, 4, 257
    x, _ = make_case(B, K, V, torch.bfloat16)
    am = torch.from_numpy(ref_argmax(x[:, :K].float().numpy()))
    tok = am.clone()                                                  # sequence 0: all accepted, drawn from the bonus row
    tok[1, 0] = (am[1, 0] + 1) % V                                    # a reject at 0
    tok[2, 1] = (am[2, 1] + 1) % V                                    # a reject in the middle; the later matches must not count
    tok[3, 1] = -1                                                    # never matches
    tok[4, 2] = V + 5                                                 # outside the vocabulary
    ref = reference(x, tok)
    assert ref["n_acc"].tolist() == [4, 0, 1, 1, 2]
    assert ref["accept"].tolist() == [[1, 1, 1, 1], [0, 1, 1, 1], [1, 0, 1, 1], [1, 0, 1, 1], [1, 1, 0, 1]]
    assert np.isneginf(ref["lp_target"][3, 1]) and np.isneginf(ref["lp_target"][4, 2])
    v = verifier_for(B, K, V, torch.bfloat16)
    for splits in (0, 1, 2, 7):
        got = run(v, x.cuda(), tok, splits=splits)
        assert_matches(got, ref, f"splits={splits}")
        assert got["drawn"][0] == ref["argmax"][0, K]


def test_two_shapes_share_one_workspace():
    big, small = (5, 8, 4173), (2, 4, 1000)
    vb, vs = verifier_for(*big, torch.bfloat16), verifier_for(*small, torch.bfloat16)
    assert vb.bytes >= vs.bytes
    vs.buf, vs.bytes = vb.buf, vb.bytes                               # sized for the larger
    (xb, tb), (xs, ts) = make_case(*big, torch.bfloat16), make_case(*small, torch.bfloat16)
    xbd, xsd = xb.cuda(), xs.cuda()
    got = [run(vb, xbd, tb, splits=3), run(vs, xsd, ts, splits=7), run(vb, xbd, tb), run(vs, xsd, ts, splits=1)]
    for g, (x, t) in zip(got, [(xb, tb), (xs, ts), (xb, tb), (xs, ts)]):
        assert_matches(g, reference(x, t))


def test_hip_ops_front_end():
    from asd_amd.distributed import HipOps
    ops = HipOps()
    x, tok = make_case(2, 4, 1000, torch.bfloat16)
    ref = reference(x, tok)
    lp_t, n_acc, drawn, lp_drawn, argmax, lp_argmax = ops.verify_greedy(x.cuda(), tok.cuda())
    assert np.array_equal(argmax.cpu().numpy(), ref["argmax"]) and np.array_equal(n_acc.cpu().numpy(), ref["n_acc"])
    assert np.array_equal(drawn.cpu().numpy(), ref["drawn"])
    assert_lp(lp_t.cpu().numpy(), ref["lp_target"], "lp_t")
    assert_lp(lp_drawn.cpu().numpy(), ref["lp_drawn"], "lp_drawn")
    plain = ops.verify_greedy(x[:, 0].cuda())                         # [B, V]: K = 0
    assert np.array_equal(plain[2].cpu().numpy(), ref["argmax"][:, 0]) and plain[0].shape == (2, 0)
    assert_lp(plain[3].cpu().numpy(), ref["lp_argmax"][:, 0], "K = 0 lp_drawn")
    assert_lp(lp_argmax.cpu().numpy(), ref["lp_argmax"], "lp_argmax")
    with pytest.raises(ValueError):
        ops.verify_greedy(x.cuda().float()[..., ::2], tok.cuda())     # no unit stride along V
