"""Tail-free sampling's argument checks, all without a GPU: both entry points' status codes and sizes, check_tail_free, and
Stage.generate, which refuses before the prompts are encoded and before any ops call and calls the pass only where a row is on."""
import ctypes as C

import pytest

import asd_amd
from asd_amd import _binding as B
from asd_amd.serving.stage_args import check_tail_free
from asd_amd.serving.stages import StageManager
from tests.mirostat_ref import VOCAB
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import NAMES, PROMPTS, stage_configs
from tests.tail_free_ref import TailFreeOracleOps

OK, INVALID, UNSUPPORTED, ALIGNMENT = 0, -1, -2, -5
BUF = (C.c_ubyte * 512)()
P = (C.addressof(BUF) + 255) & ~255                                          # stands for every device buffer: aligned, never read


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


def test_launcher_status_codes_and_workspace_size():
    lib = B.load_library()
    size = lambda b=4, k1=5, v=1024, dt=B.DTYPE_BF16: int(lib.asd_tail_free_workspace_bytes(b, k1, v, dt))   # noqa: E731

    def cut(x=P, dt=B.DTYPE_BF16, b=4, k1=5, v=1024, lds=5 * 1024, ldr=1024, table=P, ws=P, ws_bytes=None):
        return lib.asd_tail_free_rows(x, dt, b, k1, v, lds, ldr, table, ws, size(b, k1, v, dt) if ws_bytes is None else ws_bytes, None)
    assert cut(b=-1) == cut(k1=-1) == cut(v=-1) == INVALID
    assert cut(x=None, dt=99, b=0) == cut(x=None, dt=99, v=0) == OK
    assert cut(dt=99) == cut(x=None, v=2 ** 30, ldr=0) == UNSUPPORTED
    assert cut(x=None) == cut(table=None) == cut(ws=None) == cut(ldr=1023) == cut(lds=5 * 1024 - 1) == INVALID
    assert cut(ws_bytes=size() - 1) == INVALID
    assert cut(x=P + 1) == cut(dt=B.DTYPE_F32, x=P + 2) == cut(table=P + 2) == cut(ws=P + 128) == ALIGNMENT
    assert B.TAIL_FREE_REC_BYTES == 8
    assert size() == 4 * 5 * 2 * 2048 and size(dt=B.DTYPE_F32) == 2 * size() and size(v=3) == 4 * 5 * 2 * 256
    assert size(b=0) == size(v=-1) == size(dt=99) == 256
    assert all(size(b, k1, v, dt) % 256 == 0 for dt in (B.DTYPE_BF16, B.DTYPE_F16, B.DTYPE_F32) for b in (1, 7) for k1 in (1, 9)
               for v in (1, 127, 128, 129, 4099, 152064))
    assert size(5) >= size(4) and size(k1=6) >= size(k1=5) and all(size(v=v + 1) >= size(v=v) for v in range(1, 600))


def test_check_tail_free():
    assert check_tail_free(1, 2) == [1.0, 1.0] and check_tail_free([0.5, 1.0, 0.25], 3) == [0.5, 1.0, 0.25]
    for bad in (True, float("nan"), 0, 0.0, -0.5, 1.5, float("inf"), "0.5", None, [0.5], [0.5, 2.0]):
        with pytest.raises(ValueError, match="tfs"):
            check_tail_free(bad, 2)
    for field in ("tfs", "target_tfs"):                                          # a bad configuration: when the stage is built
        with pytest.raises(ValueError, match="tfs"):
            StageManager(stage_configs(vocab=VOCAB, **{field: 0.0}), ops=TailFreeOracleOps())


@pytest.mark.parametrize("name", NAMES)
def test_generate_refuses_before_encoding(name):
    ops = TailFreeOracleOps()
    stage = StageManager(stage_configs(vocab=VOCAB, top_p=1.0), ops=ops).get_stage(name)
    encoded = []
    stage._encode = lambda prompts, _orig=stage._encode: (encoded.append(1), _orig(prompts))[1]
    n = len(PROMPTS)
    for kw, match in ((dict(tfs=True), "tfs"), (dict(tfs=float("nan")), "tfs"), (dict(tfs=0), "tfs"), (dict(tfs=1.01), "tfs"),
                      (dict(tfs=[0.5] * (n - 1)), "tfs"),
                      (dict(tfs=0.9, top_n_sigma=1.0), "not built"), (dict(tfs=0.9, top_a=0.5), "not built"),
                      (dict(tfs=0.9, xtc_probability=0.5), "not built"), (dict(tfs=0.9, typical_p=0.9), "not built"),
                      (dict(tfs=0.9, epsilon_cutoff=1e-3), "not built"), (dict(tfs=0.9, eta_cutoff=1e-3), "not built"),
                      (dict(tfs=[1.0] * (n - 1) + [0.9], mirostat_tau=5.0), "Mirostat")):
        for temperature in (0.7, 0.0):                                       # greedy ignores the values, not their errors
            with pytest.raises(ValueError, match=match):
                stage.generate(prompts=PROMPTS, max_tokens=2, temperature=temperature, **kw)
    assert not encoded and not ops.trace


@pytest.mark.parametrize("name", NAMES[:2])
def test_calls_only_where_a_row_is_on(name):
    ops = TailFreeOracleOps()
    stage = StageManager(stage_configs(vocab=VOCAB, top_p=1.0), ops=ops).get_stage(name)
    run = lambda **kw: (ops.trace.clear(), stage.generate(**dict(dict(prompts=PROMPTS, max_tokens=3, temperature=0.7), **kw)),   # noqa: E731
                        [t[0] for t in ops.trace])[2]
    plain = run()
    assert run(tfs=1.0) == plain and run(tfs=[1.0] * len(PROMPTS)) == plain      # every row off: the calls it made before
    on = run(tfs=0.5)
    assert on.count("pack_tail_free") == 1 and [c for c in on if "tail_free" not in c] == plain
    assert not any("tail_free" in c for c in run(tfs=0.5, temperature=0.0))      # greedy ignores tfs and makes no call
