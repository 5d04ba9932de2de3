"""The numpy reference of asd_step_uniforms (tests/philox_ref.py) against the Random123 known-answer vectors of Philox4x32-10,
the float conversion at its ends, the counter layout of include/asd_hip.h, and the launcher's argument checks (host code:
every rejected call returns before anything is launched, so no GPU is needed)."""
import ctypes as C

import numpy as np
import pytest

from tests.philox_ref import philox4x32_10, step_uniforms_ref, to_uniform

# Random123's kat_vectors for philox4x32 with 10 rounds: counter, key, output
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_reference_reproduces_the_known_answer_vectors(counter, key, want):
    assert tuple(int(w) for w in philox4x32_10(counter, key)) == want


def test_reference_is_elementwise_over_arrays():
    ctr = np.array([k[0] for k in KAT], np.uint64)
    key = np.array([k[1] for k in KAT], np.uint64)
    got = philox4x32_10(tuple(ctr[:, i] for i in range(4)), (key[:, 0], key[:, 1]))
    assert got.dtype == np.uint32 and got.tolist() == [list(k[2]) for k in KAT]


def test_float_conversion_at_its_ends():
    f = to_uniform(np.array([0, 0xFF, 0x100, 0xFFFFFFFF], np.uint32))
    assert f.dtype == np.float32
    assert f[0] == 0.0 and f[1] == 0.0 and f[2] == np.float32(2.0 ** -24)
    assert f[3] < 1.0 and f[3] == np.float32(1.0 - 2.0 ** -24)
    scaled = f.astype(np.float64) * 2.0 ** 24                              # an exact multiple of 2^-24
    assert (scaled == np.round(scaled)).all()


def test_counter_layout():
    seeds = [0, 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1, 42]
    rd, u, rc = step_uniforms_ref(seeds, 7, 3, 4, 2)
    assert rd.shape == (4, 6) and u.shape == (6, 2) and rc.shape == (6,)
    assert all(a.dtype == np.float32 for a in (rd, u, rc))
    for b, s in enumerate(seeds):
        key = (s & 0xFFFFFFFF, s >> 32)
        for k in range(4):
            w = philox4x32_10((7, k, 3, 0), key)
            assert rd[k, b] == to_uniform(w[0])
            if k < 2:
                assert u[b, k] == to_uniform(w[1])
            if k == 0:
                assert rc[b] == to_uniform(w[2])
    # a row's draws depend on its seed, the step and the stage alone: not on its row, the batch or the K of the call
    rd2, u2, rc2 = step_uniforms_ref(seeds[::-1] + [5], 7, 3, 1, 4)
    assert np.array_equal(rd2[0, :6], rd[0, ::-1]) and np.array_equal(u2[:6, :2], u[::-1]) and np.array_equal(rc2[:6], rc[::-1])
    # ... and every one of (seed, step, stage) matters
    for other in (step_uniforms_ref(seeds, 8, 3, 4, 2), step_uniforms_ref(seeds, 7, 2, 4, 2),
                  step_uniforms_ref([s ^ 1 for s in seeds], 7, 3, 4, 2)):
        assert not any(np.array_equal(a, b) for a, b in zip(other, (rd, u, rc)))
    # int64 storage (two's complement above 2^63 - 1) reads back as the same key
    wrapped = np.array([s - 2 ** 64 if s >= 2 ** 63 else s for s in seeds], np.int64)
    assert all(np.array_equal(a, b) for a, b in zip(step_uniforms_ref(wrapped, 7, 3, 4, 2), (rd, u, rc)))


def test_uniforms_look_uniform():
    """A coarse sanity check of the wiring of words to outputs (not a test of Philox): 2^16 draws per output, mean and the
    correlation between the proposal and the accept uniform of the same slot."""
    rd, u, rc = step_uniforms_ref(np.arange(1 << 14, dtype=np.int64), 0, 1, 4, 4)
    for a in (rd, u, rc):
        assert abs(float(a.mean()) - 0.5) < 0.01 and a.min() >= 0.0 and a.max() < 1.0
    assert abs(np.corrcoef(rd.T.reshape(-1), u.reshape(-1))[0, 1]) < 0.02


def test_launcher_rejects_invalid_arguments_without_a_launch():
    from asd_amd import _binding as B
    lib = B.load_library()
    buf = (C.c_uint64 * 4)()
    p = C.addressof(buf)
    INVALID = -1

    def call(seeds=p, B_=4, Kd=2, Ka=2, rd=p, u=p, rc=p):
        return lib.asd_step_uniforms(seeds, 0, 0, B_, Kd, Ka, rd, u, rc, None)
    assert call(B_=0) == INVALID and call(B_=-1) == INVALID
    assert call(Kd=-1) == INVALID and call(Ka=-1) == INVALID
    assert call(Kd=B.MAX_DRAFT_LEN + 1) == INVALID and call(Ka=B.MAX_DRAFT_LEN + 1) == INVALID
    assert call(seeds=None) == INVALID
    assert call(rd=None, u=None, rc=None) == INVALID
    assert call(Kd=0) == INVALID and call(Ka=0) == INVALID              # an output without a slot to fill
    assert call(Kd=0, Ka=0, rd=None, u=None, rc=None) == INVALID
    assert b"invalid" in lib.asd_status_string(INVALID).lower()
