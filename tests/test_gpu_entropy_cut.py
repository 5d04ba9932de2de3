"""asd_entropy_cut_rows on the GPU against tests/entropy_cut_ref.py (numpy f64, the header's text) on the stored values: a kept
token keeps its bits, a cut token is -inf, a row that is off or has no distribution is bit-equal to the input, and so is
everything around the tensor -- the WHOLE allocation is compared: a guard band in front, the rows' padding (ld_row = V + 13),
a guard band behind.  Only the tokens inside the boundary window of tests/entropy_cut_ref.py are excused, and every test asserts
on the reference alone, before it looks at the kernel, that at most 2 % of its rows hold such a token (the seeds below were
picked on the CPU so that this holds: N(0, 3^2) logits, T = 0.7).

Shapes: V = 3 (under one vector), 64 (one tile), 4099 (past a thread's first vector in f32), 8203 (past it in 16-bit), 32781
(past a thread's first unrolled trip); one case at V = 152064; bf16 / f16 / f32; [B, V], and [B, K1 = 3, V] strided views with
ld_row = V + 13 at an odd element offset, so rows start off the 16-byte grid; all three modes and off mixed in one call."""
import functools

import numpy as np
import pytest
import torch

from tests.entropy_cut_ref import EPSILON, ETA, OFF, TYPICAL, assert_cap, check_cut, ref_entropy_cut

pytestmark = pytest.mark.gpu

PAD, GUARD = 13, 257                             # GUARD is odd: the tensor starts at an odd element offset
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DTYPE_IDS = ["bf16", "f16", "f32"]
T = 0.7
INV_T = float(np.float32(1.0 / T))
f32 = lambda v: float(np.float32(v))             # noqa: E731
MIX = [(TYPICAL, f32(0.2)), (TYPICAL, f32(0.9)), (EPSILON, f32(0.01)), (ETA, f32(0.02)), (OFF, 0.0), (TYPICAL, f32(0.95)),
       (EPSILON, f32(3e-4)), (ETA, f32(0.5))]
B, K1 = len(MIX), 3
SEEDS = {(32781, "f32"): 2}                     # (V, dtype id) -> seed; 0 where none is named


@pytest.fixture(scope="module")
def K_():
    from asd_amd import kernels
    return kernels


def _esz(dtype):
    return 4 if dtype == torch.float32 else 2


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def _arena(dtype, nb, k1, v, seed, sigma=3.0):
    """-> (buf, view): a flat buffer with guard bands and the [nb, k1, v] strided view into it (ld_row = v + PAD)."""
    g = torch.Generator().manual_seed(seed)
    n = nb * k1 * (v + PAD)
    buf = (torch.randn(n + 2 * GUARD, generator=g) * sigma).to(dtype)
    return buf, (lambda b: b[GUARD:GUARD + n].view(nb, k1, v + PAD)[:, :, :v])


def _table(rows, inv_t=INV_T):
    inv = [inv_t] * len(rows) if np.ndim(inv_t) == 0 else list(inv_t)
    return [(f32(t), m, v) for t, (m, v) in zip(inv, rows)]


def _pack(K_, table):
    return K_.pack_entropy_cut([t for t, _, _ in table], [m for _, m, _ in table], [v for _, _, v in table], "cuda")


def _launch(K_, buf, view, table, squeeze=False):
    """Run the kernel on a device copy of the arena -> the arena afterwards (CPU)."""
    dev = buf.cuda()
    x = view(dev)
    out = K_.entropy_cut_rows(x[:, 0] if squeeze else x, _pack(K_, table))
    assert out.data_ptr() == x.data_ptr()
    torch.cuda.synchronize()
    return dev.cpu()


def _check_arena(buf, after, view, table, dtype, what):
    """Outside the view nothing changed; inside, check_cut."""
    outside = torch.ones(buf.shape, dtype=torch.bool)
    view(outside)[:] = False
    assert np.array_equal(_bits(buf)[outside.numpy()], _bits(after)[outside.numpy()]), (what, "a write outside the rows")
    x0, x1 = view(buf).float().numpy(), view(after).float().numpy()
    raw0, raw1 = _bits(view(buf)), _bits(view(after))
    changed = raw0 != raw1
    assert np.isneginf(x1[changed]).all(), (what, "a changed element is not -inf")      # (kept tokens keep their BITS)
    return check_cut(x0, x1, table, _esz(dtype), what)


@functools.lru_cache(maxsize=None)
def _random_case(V, dtype, k1):
    seed = SEEDS.get((V, DTYPE_IDS[DTYPES.index(dtype)]), 0)
    buf, view = _arena(dtype, B, k1, V, 1000 + seed)
    table = _table(MIX)
    und = ref_entropy_cut(view(buf).float().numpy(), table, _esz(dtype))[2]
    return buf, view, table, und


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("V", [3, 64, 4099, 8203, 32781])
def test_random_rows_all_modes_mixed(K_, V, dtype):
    cases = [_random_case(V, dtype, 1), _random_case(V, dtype, K1)]
    und_all = np.concatenate([c[3].reshape(-1, V) for c in cases])
    assert_cap(und_all, (V, dtype))                                          # on the reference alone, before the kernel runs
    for (buf, view, table, _), k1 in zip(cases, (1, K1)):
        after = _launch(K_, buf, view, table, squeeze=k1 == 1)
        keep, _, _ = _check_arena(buf, after, view, table, dtype, (V, dtype, k1))
        x1 = view(after).float().numpy()
        assert (x1 > -np.inf).any(axis=-1).all()                             # no row is emptied
        if V >= 64:
            assert (~keep).any()                                             # the cut is live
        assert np.array_equal(_bits(view(after))[MIX.index((OFF, 0.0))], _bits(view(buf))[MIX.index((OFF, 0.0))])
        again = _launch(K_, buf, view, table, squeeze=k1 == 1)               # the same call on a fresh copy: equal bytes
        assert np.array_equal(_bits(again), _bits(after))


def test_full_vocabulary(K_):
    V, dtype = 152064, torch.bfloat16
    rows = [(TYPICAL, f32(0.9)), (EPSILON, f32(3e-4)), (ETA, f32(0.002)), (TYPICAL, f32(0.2))]
    buf, view = _arena(dtype, len(rows), 2, V, 1000 + SEEDS.get((V, "bf16"), 0))
    table = _table(rows)
    assert_cap(ref_entropy_cut(view(buf).float().numpy(), table, 2)[2], "full vocabulary")
    after = _launch(K_, buf, view, table)
    keep, _, _ = _check_arena(buf, after, view, table, dtype, "full vocabulary")
    assert (~keep).any(axis=-1).all()


def _designed(dtype):
    """-> (x f32 [R, V] as stored in `dtype`, rows, names): the hand-made rows of one launch."""
    V = 2500                                     # 625 f32 vectors: lanes 0..624, ten waves
    rng = np.random.default_rng(3)
    base = rng.standard_normal(V) * 3.0
    xs, rows, names = [], [], []

    def add(name, x, mode, value, inv_t=INV_T):
        xs.append(np.asarray(x, np.float64))
        rows.append((f32(inv_t), mode, f32(value)))
        names.append(name)
    peak = np.zeros(V)
    peak[0] = np.log(0.3 / (0.7 / (V - 1)))
    add("argmax cut", peak, TYPICAL, 0.2, 1.0)                               # p_0 = 0.3 over a uniform tail, small m
    for mode, value in ((TYPICAL, 0.3), (EPSILON, 0.5), (ETA, 0.5)):
        add(f"flat {mode}", np.full(V, 1.5), mode, value)                    # every key is 0 / every token ties the maximum
    levels = np.array([4.0, 3.0, 2.0, 1.0, 0.0, -1.0, -2.0])                 # exact ties: seven stored values, scattered
    ties = levels[rng.integers(0, len(levels), V)]
    for m in (0.35, 0.8):
        add(f"ties {m}", ties, TYPICAL, m, 1.0)
    add("ties epsilon", ties, EPSILON, 1e-3, 1.0)
    add("m near 1", base * 0.05, TYPICAL, 1.0 - 2.0 ** -24)                  # the mass never reaches it before the last token
    one = np.full(V, -np.inf)
    one[1777] = 2.0
    add("one finite typical", one, TYPICAL, 0.5)
    add("one finite epsilon", one, EPSILON, 0.5)
    add("no finite", np.full(V, -np.inf), TYPICAL, 0.5)
    nan = base.copy()
    nan[1234] = np.nan
    add("nan typical", nan, TYPICAL, 0.5)
    add("nan epsilon", nan, EPSILON, 0.01)
    inf = base.copy()
    inf[99] = np.inf
    add("+inf", inf, ETA, 0.01)
    two = np.full(V, -np.inf)
    two[[5, 2100]] = [1.0, 0.4]
    add("two tokens typical", two, TYPICAL, 0.5)
    add("two tokens eta", two, ETA, 0.4)
    add("eta sqrt term", base * 0.05, ETA, 0.02)                             # a wide row: sqrt(e) exp(-H) < e
    add("eta e term", base * 3.0, ETA, 0.02)                                 # a peaked row: e < sqrt(e) exp(-H)
    add("off", base, OFF, 0.0)
    x = torch.from_numpy(np.stack(xs)).to(torch.float32).to(dtype)
    return x, rows, names


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_designed_rows(K_, dtype):
    x, rows, names = _designed(dtype)
    R, V = x.shape
    x0 = x.float().numpy()
    keep, thr, und, touched = ref_entropy_cut(x0, rows, _esz(dtype))
    assert_cap(und, "designed rows")
    at = names.index
    # what the reference says about the rows, before the kernel
    assert not keep[at("argmax cut"), 0] and keep[at("argmax cut"), 1:].all()
    for n in ("flat 1", "flat 2", "flat 3", "m near 1", "one finite typical", "one finite epsilon"):
        assert keep[at(n)].all() and touched[at(n)], n
    for n in ("no finite", "nan typical", "nan epsilon", "+inf", "off"):
        assert not touched[at(n)], n
    for n in ("ties 0.35", "ties 0.8", "ties epsilon"):
        r = at(n)
        assert (~keep[r]).any() and keep[r].any()
        for v in np.unique(x0[r]):
            assert len(set(keep[r][x0[r] == v].tolist())) == 1               # every tie shares its fate
    def H(r):
        z = x0[r].astype(np.float64) * INV_T
        p = np.exp(z - z.max()) / np.exp(z - z.max()).sum()
        return float(-(p[p > 0] * np.log(p[p > 0])).sum())
    e = f32(0.02)
    assert np.sqrt(e) * np.exp(-H(at("eta sqrt term"))) < e < np.sqrt(e) * np.exp(-H(at("eta e term")))
    dev = x.cuda()
    out = K_.entropy_cut_rows(dev, _pack(K_, rows))
    torch.cuda.synchronize()
    x1 = out.cpu().float().numpy()
    check_cut(x0, x1, rows, _esz(dtype), "designed rows")
    bits0, bits1 = _bits(x), _bits(out)
    for n in ("flat 1", "flat 2", "flat 3", "m near 1", "one finite typical", "one finite epsilon", "no finite", "nan typical",
              "nan epsilon", "+inf", "off"):
        assert np.array_equal(bits0[at(n)], bits1[at(n)]), n                 # bit-equal rows, NaN payloads included
    assert np.isneginf(x1[at("argmax cut"), 0]) and np.array_equal(bits0[at("argmax cut"), 1:], bits1[at("argmax cut"), 1:])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_per_row_temperatures_equal_the_scalar_calls(K_, dtype):
    V = 4099
    temps = [0.7, 1.0, 0.5, 1.3, 0.7, 2.0, 0.9, 0.6]
    inv = [f32(1.0 / t) for t in temps]
    buf, view = _arena(dtype, B, K1, V, 77)
    mixed = _launch(K_, buf, view, _table(MIX, inv))
    for b in sorted(set(range(B)) - {MIX.index((OFF, 0.0))}):
        scalar = _launch(K_, buf, view, _table(MIX, inv[b]))
        assert np.array_equal(_bits(view(scalar))[b], _bits(view(mixed))[b]), b
    assert not np.array_equal(_bits(view(_launch(K_, buf, view, _table(MIX, inv[2]))))[0], _bits(view(mixed))[0])
