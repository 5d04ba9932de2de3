"""Mirostat's argument checks: both launchers' status codes in the header's order (they reject, or find nothing to do, before
anything is launched: no GPU, nothing dereferenced), then the ValueErrors of check_mirostat, kernels.check_mirostat_rows and
Stage.generate, which refuses before the prompts are encoded and before any ops call."""
import ctypes as C

import pytest

import asd_amd
from asd_amd import _binding as B
from asd_amd import kernels as K
from asd_amd.serving.stage_args import check_mirostat
from asd_amd.serving.stages import StageManager
from tests.mirostat_ref import VOCAB, MirostatOracleOps
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import NAMES, PROMPTS, stage_configs

OK, INVALID, UNSUPPORTED, ALIGNMENT = 0, -1, -2, -5
BUF = (C.c_ubyte * 512)()
P = (C.addressof(BUF) + 255) & ~255                                          # stands for every device buffer: aligned, never read


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def test_rows_status_codes():
    nb, K1, V = 4, 5, 1024

    def call(x=P, dt=B.DTYPE_BF16, b=nb, k1=K1, v=V, lds=K1 * V, ldr=V, table=P, mu=P, tok=P, ldt=K1 - 1, path=P, ws=P, wsb=nb * K1 * 16):
        return B.load_library().asd_mirostat_rows(x, dt, b, k1, v, lds, ldr, table, mu, tok, ldt, path, ws, wsb, None)
    assert call(b=-1) == call(k1=-1) == call(v=-1) == call(b=-1, k1=0) == INVALID        # ... before the empty call
    assert call(x=None, dt=99, b=0) == call(x=None, dt=99, k1=0) == call(x=None, dt=99, v=0) == OK
    assert call(dt=99) == call(x=None, dt=99) == UNSUPPORTED                             # unsupported before NULL
    assert call(b=65536) == call(k1=66, lds=66 * V) == call(x=None, v=2 ** 30, ldr=0) == UNSUPPORTED
    assert all(call(**{n: None}) == INVALID for n in ("x", "table", "mu", "path", "ws", "tok"))
    assert call(ldr=V - 1) == call(lds=K1 * V - 1) == call(ldt=K1 - 2) == call(wsb=nb * K1 * 16 - 1) == INVALID
    assert call(x=P + 1, wsb=0) == INVALID                                               # invalid before alignment
    assert call(tok=None, k1=1, lds=V, ldt=0, x=P + 1) == ALIGNMENT                      # K1 == 1 needs no proposals
    assert call(x=P + 1) == call(dt=B.DTYPE_F32, x=P + 2) == call(ws=P + 8) == ALIGNMENT
    assert all(call(**{n: P + 2}) == ALIGNMENT for n in ("table", "mu", "tok", "path"))
    assert (B.MIROSTAT_REC_BYTES, B.MIROSTAT_ROW_BYTES) == (12, 16)


def test_commit_status_codes():
    names = ("path", "n_acc", "lp", "seq_len", "n_commit", "table", "mu", "out")

    def call(b=4, k1=5, cap=32, **ptr):
        a = [ptr.get(n, P) for n in names]
        return B.load_library().asd_mirostat_commit(a[0], b, k1, *a[1:], cap, None)
    assert call(b=-1) == call(k1=0) == call(cap=0) == call(b=0, k1=0) == INVALID
    assert call(b=0, path=None) == OK
    assert all(call(**{n: None}) == INVALID and call(**{n: P + 2}) == ALIGNMENT for n in names)
    assert call(path=None, mu=P + 2) == INVALID                                          # NULL before alignment


def test_check_mirostat():
    assert check_mirostat(0.0, 0.1, 3) == [(0.0, 0.0)] * 3 and check_mirostat(5, 0.5, 2) == [(5.0, 0.5)] * 2
    assert check_mirostat([5.0, 0, 32], [1.0, 0.5, 0.25], 3) == [(5.0, 1.0), (0.0, 0.0), (32.0, 0.25)]
    for bad in (True, float("nan"), -1.0, 32.5, "5", None, [5.0], [5.0, True]):
        with pytest.raises(ValueError, match="mirostat_tau"):
            check_mirostat(bad, 0.1, 2)
    for bad in (False, float("nan"), 0.0, 1.5, "x", None, [0.1], [0.1, None]):
        with pytest.raises(ValueError, match="mirostat_eta"):
            check_mirostat(5.0, bad, 2)
    with pytest.raises(ValueError, match="without mirostat_tau"):
        check_mirostat([0.0, 0.0], 0.2, 2, eta_given=True)
    rec = K.check_mirostat_rows([1.0, 2.0], [0.0, 5.0], [0.0, 0.5])
    assert rec.dtype.itemsize == 12 and rec["tau"].tolist() == [0.0, 5.0] and rec["eta"].tolist() == [0.0, 0.5]
    for bad in (([1.0], [5.0, 5.0], [0.1, 0.1]), ([0.0], [5.0], [0.1]), ([float("inf")], [5.0], [0.1]), ([1.0], [33.0], [0.1]),
                ([1.0], [True], [0.1]), ([1.0], [5.0], [0.0]), ([1.0], [5.0], [float("nan")]), ([1.0], [float("nan")], [0.1])):
        with pytest.raises(ValueError):
            K.check_mirostat_rows(*bad)
    with pytest.raises(ValueError, match="mirostat_tau"):                                # a bad configuration: when the stage is built
        StageManager(stage_configs(vocab=VOCAB, mirostat_tau=33.0), ops=MirostatOracleOps())
    with pytest.raises(ValueError, match="mirostat_eta"):
        StageManager(stage_configs(vocab=VOCAB, target_mirostat_eta=0.0), ops=MirostatOracleOps())


@pytest.mark.parametrize("name", NAMES)
def test_generate_refuses_before_encoding(name):
    ops = MirostatOracleOps()
    stage = StageManager(stage_configs(vocab=VOCAB, top_p=1.0), ops=ops).get_stage(name)
    encoded = []
    stage._encode = lambda prompts, _orig=stage._encode: (encoded.append(1), _orig(prompts))[1]
    n, on = len(PROMPTS), dict(mirostat_tau=5.0)
    some = dict(mirostat_tau=[5.0] + [0.0] * (n - 1))
    for kw, match in ((dict(mirostat_tau=True), "mirostat_tau"), (dict(mirostat_tau=float("nan")), "mirostat_tau"),
                      (dict(mirostat_tau=40.0), "mirostat_tau"), (dict(mirostat_tau=[5.0] * (n - 1)), "mirostat_tau"),
                      (dict(on, mirostat_eta=0.0), "mirostat_eta"), (dict(on, mirostat_eta=2.0), "mirostat_eta"),
                      (dict(mirostat_eta=0.2), "without mirostat_tau"), (dict(on, top_k=40), "replaces"), (dict(on, top_p=0.9), "replaces"),
                      (dict(on, min_p=0.05), "replaces"), (dict(on, typical_p=0.9), "replaces"), (dict(on, epsilon_cutoff=1e-3), "replaces"),
                      (dict(on, eta_cutoff=1e-3), "replaces"), (dict(some, top_k=[40] + [0] * (n - 1)), "replaces")):
        for temperature in (0.7, 0.0):                                       # greedy ignores the values, not their errors
            with pytest.raises(ValueError, match=match):
                stage.generate(prompts=PROMPTS, max_tokens=2, temperature=temperature, **kw)
    assert not encoded and not ops.trace
    stage.generate(prompts=PROMPTS, max_tokens=2, temperature=0.7, mirostat_tau=[0.0] + [5.0] * (n - 1), top_k=[40] + [0] * (n - 1))
    assert encoded and {"pack_mirostat", "mirostat_rows", "mirostat_commit"} <= {c for c, _ in ops.trace}
