"""asd_cfg_rows on the GPU against tests/cfg_ref.py.  B = 2 conditional and Bu = 2 unconditional sequences of K1 rows in
allocations of their own offsets and strides: the rows of a pair sit at different 16-byte phases.  Both WHOLE allocations are
compared: the unconditional one, the padding and every skipped row bit for bit, -inf where the rule puts it, a written element
within (|s| + |1 - s|) lp_bar + 4 ulp_f32(max(|s c'|, |(1 - s) u'|)) + 1/2 ulp_dtype(ref), lp_bar = 2e-5."""
import numpy as np
import pytest
import torch

from tests.cfg_ref import guide, live

pytestmark = pytest.mark.gpu

LP_BAR = 2e-5
FORMAT = {torch.bfloat16: (7, -126), torch.float16: (10, -14), torch.float32: (23, -126)}    # mantissa bits, lowest normal exponent
CAP = 19456 * 4                                          # f32 elements the resident kernel holds: ASD_CFG_RESIDENT_VECTORS (asserted below)
SCALES = [(0.0, 1.5), (0.5, 1.0), (7.5, 0.5)]
SHAPES = [(dt, V) for dt in FORMAT for V in (1, 7, 1000, 1001)] + [(torch.float32, V) for V in (CAP - 1, CAP, CAP + 1)]
NAN, INF = float("nan"), float("inf")


def ulp(x, mant, emin):
    with np.errstate(divide="ignore"):
        return 2.0 ** (np.maximum(np.floor(np.log2(np.abs(x))), emin) - mant)


def rows_of(dtype, K1, V, seed):
    """[allocation, its [2, K1, V] view, (strides, offset)] of c and of u: a sentinel in the padding, elements N(0, 4^2), -inf
    in c only, in u only and (11, 26, ...) in both."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for off, pad_row, pad_seq in ((1, 3, 5), (0, 6, 2)):
        lay = ((K1 * (V + pad_row) + pad_seq, V + pad_row, 1), off)
        buf = torch.full((off + 2 * lay[0][0] + 8,), 7.0, dtype=dtype)
        view = buf.as_strided((2, K1, V), *lay)
        view.copy_((torch.randn((2, K1, V), generator=g) * 4.0).to(dtype))
        out += [buf, view, lay]
    out[1][:, :, 1::5] = -np.inf
    out[4][:, :, 2::3] = -np.inf
    return out


def run(cbuf, clay, ubuf, ulay, table, K1, V):
    from asd_amd import kernels as K
    cd, ud = cbuf.cuda(), ubuf.cuda()
    K.cfg_rows(cd.as_strided((2, K1, V), *clay), ud.as_strided((2, K1, V), *ulay), table)
    torch.cuda.synchronize()
    return cd.cpu(), ud.cpu()


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def check(dtype, K1, V, recs, table, cbuf, c, clay, ubuf, u, ulay):
    """-> (the conditional allocation after the call, the rows the reference writes)."""
    got_c, got_u = run(cbuf, clay, ubuf, ulay, table, K1, V)
    assert torch.equal(bits(got_u), bits(ubuf)), "the unconditional allocation was written"
    want, tol = cbuf.double().clone(), torch.zeros(cbuf.shape, dtype=torch.float64)
    touched = torch.zeros(cbuf.shape, dtype=torch.bool)
    wv, tv, hv = (t.as_strided((2, K1, V), *clay) for t in (want, tol, touched))
    written = 0
    for b, (s, q) in enumerate(recs):
        for j in range(K1) if live(s, q, 2) else ():
            out = guide(c[b, j].double().numpy(), u[q, j].double().numpy(), s)
            if out is None:
                continue
            ref, a, t = out
            fin = np.isfinite(ref)
            bound = np.where(fin, (abs(s) + abs(1.0 - s)) * LP_BAR + 4.0 * ulp(np.maximum(np.abs(a), np.abs(t)), 23, -126)
                             + 0.5 * ulp(np.where(fin, ref, 1.0), *FORMAT[dtype]), 0.0)
            wv[b, j], tv[b, j], hv[b, j] = torch.from_numpy(ref), torch.from_numpy(bound), True
            written += 1
    got = got_c.double()
    assert torch.equal(bits(got_c)[~touched], bits(cbuf)[~touched]), "padding or a skipped row changed"
    exact = tol == 0.0                                   # in a written row: the rule's -inf
    assert bool(torch.isneginf(want[touched & exact]).all()) and torch.equal(got[touched & exact], want[touched & exact])
    err = (got - want)[~exact].abs()
    assert bool((err <= tol[~exact]).all())
    return got_c, written


@pytest.mark.parametrize("scales", SCALES, ids=str)
@pytest.mark.parametrize("K1", [1, 3])
@pytest.mark.parametrize("dtype,V", SHAPES, ids=str)
def test_guided_rows_against_f64(dtype, V, K1, scales):
    from asd_amd import _binding as B_, kernels as K
    assert B_.CFG_RESIDENT_VECTORS * 4 == CAP
    cbuf, c, clay, ubuf, u, ulay = rows_of(dtype, K1, V, V + K1)
    recs = [(scales[0], 1), (scales[1], 0)]
    table = K.pack_cfg([s for s, _ in recs], [q for _, q in recs], "cuda")
    first, written = check(dtype, K1, V, recs, table, cbuf, c, clay, ubuf, u, ulay)
    assert written == K1 * sum(s != 1.0 for s in scales)
    again, _ = run(cbuf, clay, ubuf, ulay, table, K1, V)
    assert torch.equal(bits(again), bits(first)), "a second call on fresh copies gives other bits"
    same = torch.full(cbuf.shape, 7.0, dtype=dtype)      # the unconditional rows at the conditional rows' own phases
    same.as_strided((2, K1, V), *clay).copy_(u)
    level, _ = run(cbuf, clay, same, clay, table, K1, V)
    assert torch.equal(bits(level), bits(first)), "the result depends on the rows' 16-byte phases"


# a flawed pair, (b = 0, j = 1) <-> unconditional (q = 1, j = 1): (the side, the value at element 777 or None: the row all -inf);
# 3e38: |x| log2 e leaves f32's range (+inf in f16).  An off or damaged record of sequence 0: (scale, index)
SKIPS = {"nan in c": ("c", NAN), "nan in u": ("u", NAN), "+inf in c": ("c", INF), "+inf in u": ("u", INF), "huge in c": ("c", 3e38),
         "huge in u": ("u", 3e38), "c all -inf": ("c", None), "u all -inf": ("u", None), "index < 0": (1.5, -1), "scale nan": (NAN, 1),
         "scale 150": (150.0, 1), "scale < 0": (-0.5, 1), "index >= Bu": (1.5, 2), "scale 1": (1.0, 1)}


@pytest.mark.parametrize("dtype", list(FORMAT), ids=str)
@pytest.mark.parametrize("skip", list(SKIPS))
def test_what_is_skipped_keeps_its_bits_and_its_neighbours_are_written(dtype, skip):
    from asd_amd import kernels as K
    K1, V = 3, 1001
    cbuf, c, clay, ubuf, u, ulay = rows_of(dtype, K1, V, 5)
    a, v = SKIPS[skip]
    if isinstance(a, str):
        row = c[0, 1] if a == "c" else u[1, 1]
        row[slice(None) if v is None else 777] = -np.inf if v is None else v
    recs = [(1.5, 1) if isinstance(a, str) else (a, v), (0.5, 0)]
    raw = np.array(recs, dtype=K._CFG_REC)               # pack_cfg refuses a damaged record: the table is built by hand
    table = K.Cfg(torch.from_numpy(raw.view(np.uint8).reshape(2, 8).copy()).cuda(), (recs[0][1], 0), 2, 2)
    _, written = check(dtype, K1, V, recs, table, cbuf, c, clay, ubuf, u, ulay)
    assert written == (2 * K1 - 1 if isinstance(a, str) else K1)
