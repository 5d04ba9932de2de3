"""asd_step_uniforms on the GPU against the numpy Philox reference (tests/philox_ref.py), bit for bit: every output present and
every output left out in turn, seeds at the ends of the 64-bit range, steps at the ends of the 32-bit range, NaN-filled buffers
with guard bands around every output, and the launcher's argument checks on real device pointers."""
import numpy as np
import pytest
import torch

from tests.philox_ref import step_uniforms_ref

pytestmark = pytest.mark.gpu

GUARD = 64                                       # f32 elements of NaN on either side of every output
SPECIAL = [0, 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1]
CASES = [(1, 1, 0), (3, 1, 1), (33, 8, 8), (130, 64, 64), (257, 0, 5)]
STEPS = [0, 1, 2 ** 32 - 1]
STAGES = [0, 15]


@pytest.fixture(scope="module")
def K_():
    from asd_amd import kernels
    return kernels


def _seeds(B):
    """B seeds in [0, 2^64) that hold the special values (as many as fit), as Python ints and as the int64 upload."""
    rng = np.random.default_rng(B)
    vals = (SPECIAL + [int(x) for x in rng.integers(0, 2 ** 64, size=B, dtype=np.uint64)])[:B]
    if B < len(SPECIAL):
        vals = SPECIAL[-B:]
    dev = torch.tensor([v - 2 ** 64 if v >= 2 ** 63 else v for v in vals], dtype=torch.int64, device="cuda")
    return vals, dev


def _same_bits(t, ref):
    return t.cpu().numpy().tobytes() == np.ascontiguousarray(ref, np.float32).tobytes()


def _all_nan(t):
    return bool(torch.isnan(t).all())


class Arena:
    """One NaN-filled f32 buffer: guard | r_draft [Kd, B] | guard | u [B, Ka] | guard | r_commit [B] | guard."""

    def __init__(self, B, Kd, Ka):
        sizes = [Kd * B, B * Ka, B]
        self.buf = torch.full((sum(sizes) + 4 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        at, views = GUARD, []
        for n in sizes:
            views.append(self.buf[at:at + n])
            at += n + GUARD
        self.r_draft = views[0].view(Kd, B) if Kd else None
        self.u = views[1].view(B, Ka) if Ka else None
        self.r_commit = views[2]
        self.outputs = [v for v in (self.r_draft, self.u, self.r_commit) if v is not None]

    def guards_intact(self, written):
        """Everything outside the outputs in `written` is still NaN."""
        mask = torch.ones_like(self.buf, dtype=torch.bool)
        base = self.buf.data_ptr()
        for v in written:
            a = (v.data_ptr() - base) // 4
            mask[a:a + v.numel()] = False
        return _all_nan(self.buf[mask])


def test_seed_sets_hold_the_special_values():
    for B, _, _ in CASES:
        vals, dev = _seeds(B)
        assert len(vals) == B == dev.shape[0]
        if B >= len(SPECIAL):
            assert vals[:len(SPECIAL)] == SPECIAL
    assert _seeds(1)[0] == [2 ** 64 - 1] and _seeds(3)[0] == [2 ** 32, 2 ** 63, 2 ** 64 - 1]


@pytest.mark.parametrize("B,Kd,Ka", CASES)
def test_kernel_equals_the_reference_bit_for_bit(K_, B, Kd, Ka):
    vals, seeds = _seeds(B)
    names = ["r_draft"] * (Kd > 0) + ["u"] * (Ka > 0) + ["r_commit"]
    variants = [tuple(names)] + [tuple(n for n in names if n != drop) for drop in names if len(names) > 1]
    for step in STEPS:
        for stage in STAGES:
            ref = dict(zip(("r_draft", "u", "r_commit"), step_uniforms_ref(vals, step, stage, Kd, Ka)))
            for present in variants:
                arena = Arena(B, Kd, Ka)
                kw = {n: getattr(arena, n) for n in present}
                K_.step_uniforms(seeds, step, stage, **kw)
                torch.cuda.synchronize()
                for n in present:
                    assert _same_bits(kw[n], ref[n]), (n, step, stage, present)
                    assert float(kw[n].min()) >= 0.0 and float(kw[n].max()) < 1.0
                assert arena.guards_intact(list(kw.values())), (step, stage, present)      # skipped outputs and guards: NaN


def test_rows_depend_on_their_seed_alone(K_):
    """The same seeds in another order, in a larger batch and under other K: every row keeps its uniforms."""
    vals, seeds = _seeds(33)
    a = Arena(33, 8, 8)
    K_.step_uniforms(seeds, 5, 2, a.r_draft, a.u, a.r_commit)
    perm = torch.randperm(33, generator=torch.Generator().manual_seed(0))
    more = torch.cat([seeds[perm.cuda()], torch.arange(100, device="cuda")])
    b = Arena(133, 3, 64)
    K_.step_uniforms(more, 5, 2, b.r_draft, b.u, b.r_commit)
    torch.cuda.synchronize()
    p = perm.cuda()
    assert torch.equal(b.r_draft[:, :33], a.r_draft[:3][:, p]) and torch.equal(b.u[:33, :8], a.u[p])
    assert torch.equal(b.r_commit[:33], a.r_commit[p])


def test_hip_ops_returns_views_of_one_buffer():
    from asd_amd.distributed import HipOps
    ops = HipOps()
    vals, seeds = _seeds(33)
    ref = step_uniforms_ref(vals, 3, 1, 8, 8)
    out = torch.full(((8 + 8 + 1) * 33 + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    rd, u, rc = ops.step_uniforms(seeds, 3, 1, 8, 8, out=out)
    assert rd.shape == (8, 33) and u.shape == (33, 8) and rc.shape == (33,)
    assert rd.data_ptr() == out.data_ptr() and rc.data_ptr() == out.data_ptr() + 4 * 16 * 33
    assert all(_same_bits(t, r) for t, r in zip((rd, u, rc), ref)) and _all_nan(out[17 * 33:])
    rd, u, rc = ops.step_uniforms(seeds, 3, 1, 8, 8)                   # a fresh buffer
    assert all(_same_bits(t, r) for t, r in zip((rd, u, rc), ref))
    # stage 0's call: one proposal uniform, nothing else written
    out.fill_(float("nan"))
    rd, u, rc = ops.step_uniforms(seeds, 3, 1, 1, 0, commit=False, out=out)
    assert u is None and rc is None and _same_bits(rd, ref[0][:1]) and _all_nan(out[33:])
    rd, u, rc = ops.step_uniforms(seeds, 3, 1, 0, 5, out=out)
    assert rd is None and _same_bits(u, ref[1][:, :5]) and _same_bits(rc, ref[2])
    with pytest.raises(ValueError):
        ops.step_uniforms(seeds, 3, 1, 8, 8, out=out[:17 * 33 - 1])


def test_invalid_arguments_return_the_status_without_a_launch(K_):
    from asd_amd import _binding as B_
    lib = B_.load_library()
    B, Kd, Ka = 4, 2, 2
    arena = Arena(B, Kd, Ka)
    seeds = torch.arange(B, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    P = dict(seeds=seeds.data_ptr(), rd=arena.r_draft.data_ptr(), u=arena.u.data_ptr(), rc=arena.r_commit.data_ptr())
    INVALID = -1

    def call(B=B, Kd=Kd, Ka=Ka, **over):
        p = {**P, **over}
        return lib.asd_step_uniforms(p["seeds"], 0, 0, B, Kd, Ka, p["rd"], p["u"], p["rc"], st)
    assert call(B=0) == INVALID and call(B=-1) == INVALID
    assert call(Kd=-1) == INVALID and call(Ka=-1) == INVALID
    assert call(Kd=B_.MAX_DRAFT_LEN + 1) == INVALID and call(Ka=B_.MAX_DRAFT_LEN + 1) == INVALID
    assert call(seeds=None) == INVALID
    assert call(rd=None, u=None, rc=None) == INVALID
    assert call(Kd=0) == INVALID and call(Ka=0) == INVALID            # an output without a slot to fill
    assert call(Kd=0, Ka=0, rd=None, u=None, rc=None) == INVALID
    torch.cuda.synchronize()
    assert _all_nan(arena.buf)                                        # nothing was launched
    # the front end reports the same status
    with pytest.raises(B_.AsdError) as e:
        K_.step_uniforms(seeds, 0, 0, torch.empty((B_.MAX_DRAFT_LEN + 1, B), dtype=torch.float32, device="cuda"))
    assert e.value.status == INVALID
    with pytest.raises(B_.AsdError):
        K_.step_uniforms(seeds, 0, 0)
    with pytest.raises(ValueError):
        K_.step_uniforms(seeds, 2 ** 32, 0, r_commit=arena.r_commit)
    with pytest.raises(ValueError):
        K_.step_uniforms(seeds, 0, 0, r_commit=arena.r_commit[:3])
    assert call() == 0                                                # ... and the valid call runs
    torch.cuda.synchronize()
    ref = step_uniforms_ref(list(range(B)), 0, 0, Kd, Ka)
    assert all(_same_bits(t, r) for t, r in zip((arena.r_draft, arena.u, arena.r_commit), ref))
