"""The losslessness case of the entropy cuts on the harness and bars of tests/lossless.py (unchanged): V = 64, the draft rows cut
with typical_p = M_DRAFT and the target rows with another, typical_p = M_TARGET, by the ops object under test -- the oracle twin
of tests/entropy_cut_ref.py on the CPU (tests/test_lossless_entropy_cut.py), asd_entropy_cut_rows on the GPU
(tests/test_gpu_lossless_entropy_cut.py).  The cut rows then go through the plain draft / verify / residual chain, and every
committed-token histogram is held to the CUT TARGET distribution: softmax(x_t / T) restricted to the set `typical_keep` below
keeps and renormalised.  `typical_keep` is written here from the definition alone (a loop over the tokens in order of
|-ln p - H|) and shares no code with ref_entropy_cut or the kernel.  The geometry is flat enough that a cut target row keeps at
least 30 tokens with an expected count of 20 at the bonus position, which check_inputs asserts on the reference alone, and the
two cuts differ in both directions: the draft cuts tokens the target keeps, and the target cuts tokens the draft keeps.

TEST INFRASTRUCTURE: never importable from the package."""
import numpy as np

from tests import lossless as L

M_DRAFT, M_TARGET = 0.8, 0.9
GEOM = L.Geometry(V=64, K=2, B=4096, n_calls=40, scale=0.45, noise=0.3)
ROUTE = L.ROUTES["a"]                            # no top-k / top-p: the cut is the only truncation
ROW_SEED, DRAW_SEED = 1, 2024
TYPICAL = 1                                      # ASD_CUT_TYPICAL


def typical_keep(x_row, inv_t, m):
    """bool [V]: the tokens typical_p = m keeps of softmax(x * inv_t), from the definition: tokens in ascending order of
    d = |-ln p - H| are kept until their mass reaches m, and with them every token that ties the last one's d."""
    z = np.asarray(x_row, np.float64) * float(inv_t)
    logp = z - (z.max() + np.log(np.exp(z - z.max()).sum()))
    p = np.exp(logp)
    H = -float((p * logp).sum())
    d = np.abs(-logp - H)
    keep = np.zeros(z.size, bool)
    mass, d_last = 0.0, -1.0
    for v in sorted(range(z.size), key=lambda v: d[v]):
        if mass >= m and d[v] > d_last:
            break
        keep[v], mass, d_last = True, mass + p[v], d[v]
    return keep


def cut_reference(x, m):
    """x [..., V] f32 -> the same rows with every token typical_keep drops at -inf (f32)."""
    out = np.array(x, np.float32, copy=True)
    flat = out.reshape(-1, out.shape[-1])
    for r in range(flat.shape[0]):
        flat[r][~typical_keep(flat[r], L.INV_T, float(np.float32(m)))] = -np.inf
    return out


def rows_and_reference():
    """-> (xt, xd: the stored f32 rows of every class, uncut; ref: lossless.Reference of the CUT rows, from typical_keep; the
    cut rows themselves).  Asserts the harness's input conditions and that the two cuts differ in both directions."""
    xt, xd = L.make_rows(GEOM, "f32", ROW_SEED)
    ct, cd = cut_reference(xt, M_TARGET), cut_reference(xd, M_DRAFT)
    ref = L.reference(ct, cd, ROUTE)
    L.check_inputs(ref, ROUTE, GEOM.B * GEOM.n_calls // L.R_CLASSES)
    kt, kd = np.isfinite(ct[:, :GEOM.K]), np.isfinite(cd)
    assert (kt & ~kd).any() and (kd & ~kt).any() and (~np.isfinite(ct)).any(axis=-1).all() and (~kd).any(axis=-1).all()
    return xt, xd, ref, ct, cd


def cut_by(entropy_cut_rows, pack_entropy_cut, x, m, to_array, from_array):
    """x [R, J, V] f32 through the ops under test: one record per class, every row of the class under it."""
    t = from_array(np.ascontiguousarray(x, np.float32))
    table = pack_entropy_cut([L.INV_T] * x.shape[0], [TYPICAL] * x.shape[0], [float(np.float32(m))] * x.shape[0], t.device)
    return to_array(entropy_cut_rows(t, table))
