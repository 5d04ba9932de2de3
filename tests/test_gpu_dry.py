"""asd_dry_rows on the GPU against tests/dry_ref.py, BIT-EQUAL over the whole allocation: a guard band in front, the tensor with
its row padding (ld_row = V + 7), a guard band behind.  B = 3: row 0 takes the case's values, row 1 is off and must stay
untouched, row 2 takes other values on the same history.  Every case is the smallest history that reaches the path its name
states; each runs with K1 in {1, 3} and n_prev in {0, 2} unless it names its own configurations."""
import numpy as np
import pytest
import torch

from tests.dry_ref import ref_dry

pytestmark = pytest.mark.gpu

V, PAD, GUARD, START, N_TOK = 257, 7, 128, 4, 5
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
CONFIGS = [(1, 0, False), (1, 2, True), (3, 0, True), (3, 2, True)]                  # (K1, n_prev, with step_tok)
TILE, SLOTS = 4096, 1024                         # the kernel's history tile and the followers one pass of its table holds


def case(real=(), gen=(), prop=(60, 61, 62, 63, 64), allowed=1, rng=0, brk=(), mul=0.8, base=1.75, v=V, poison=(), configs=CONFIGS, quiet=False):
    return dict(quiet=quiet, real=list(real), gen=list(gen), prop=list(prop), allowed=allowed, rng=rng, brk=brk, mul=mul, base=base, v=v,
                poison=poison, configs=configs)


CASES = {
    "length 0": case(quiet=True), "length 1": case(gen=[5], quiet=True), "length 2": case(gen=[5, 5]),
    "periodic: the match grows past allowed_length": case(gen=[1, 2, 3, 1, 2], prop=[3, 1, 2, 3, 1], allowed=3),
    "one follower at several match lengths: the max": case(gen=[9, 1, 2, 7, 8, 1, 2, 7, 3, 2, 7, 4, 2, 5, 1, 2]),
    "a match across tokens | step_tok": case(real=[1, 2], gen=[3, 4, 1, 2], prop=[3, 4, 1, 2, 3], allowed=2),
    "the padding is no history": case(real=[7, 0], quiet=True),
    "range cuts a match short": case(gen=[1, 2, 3, 9, 1, 2, 3], prop=[9, 1, 2, 3, 9], rng=5),
    "last is a breaker": case(gen=[1, 2, 1, 2], prop=[1, 2, 1, 2, 1], brk=(2,), quiet=True),
    "a breaker inside the suffix": case(gen=[1, 2, 3, 1, 2, 3], prop=[1, 2, 3, 1, 2], brk=(2, 200)),
    "a breaker as the follower": case(gen=[1, 2, 1], prop=[3, 1, 2, 1, 3], brk=(2,)),
    "followers outside [0, V)": case(gen=[1, V, 1, -1, 1, 2 ** 31 - 1, 1], prop=[V + 5, 1, 5, 1, 5]),
    "-inf and NaN at penalised ids": case(gen=[1, 2, 1, 3, 1, 4, 1], prop=[2, 1, 3, 1, 4], poison=((2, float("-inf")), (3, float("nan")))),
    "a penalty that clamps f16, and +inf that clamps all": case(gen=[1, 2, 1, 3, 1, 2, 1], prop=[2, 1, 3, 1, 2], mul=1.0e5, base=1.0e30),
    "all equal, past CAP and the tile": case(gen=[4] * (TILE + 70), prop=[4] * 5, allowed=2, configs=CONFIGS[3:]),
    # 2500 even followers and 300 odd ones: the classes (0, 2), (0, 4) and the right child (2, 4) overflow, the walk climbs
    # through two right children from (6, 8) to (1, 2)
    "more distinct followers than the table holds": case(gen=[t for f in range(2800) for t in (1, 2 + 2 * f if f < 2500 else 2 * f - 4997)] + [1],
                                                         prop=[7, 1, 8000, 1, 5], v=8192, configs=CONFIGS[3:]),
}


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy().tobytes()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("name", CASES)
def test_kernel_is_bit_equal_to_the_reference(name, dtype):
    from asd_amd import kernels as K_
    c, B = CASES[name], 3
    v, rows = c["v"], [(c["mul"], c["base"], c["allowed"], c["rng"]), (0.0, 1.75, 2, 0), (0.5 * c["mul"], 2.0, min(c["allowed"] + 1, 64), 0)]
    max_len = START + len(c["gen"]) + 2
    tokens = np.zeros((B, max_len + 3), dtype=np.int32)
    tokens[:, START - len(c["real"]):START] = c["real"]
    tokens[:, START:START + len(c["gen"])] = c["gen"]
    seq_len, step = [START + len(c["gen"])] * B, np.array([c["prop"]] * B, dtype=np.int32)
    packed = K_.pack_dry(*zip(*rows), c["brk"], [len(c["real"])] * B, START, "cuda")
    changed = False
    for K1, n_prev, with_tok in c["configs"]:
        n = B * K1 * (v + PAD)
        buf = (torch.randn(n + 2 * GUARD, generator=torch.Generator().manual_seed(K1 + n_prev)) * 4.0).to(dtype)
        view = lambda t: t[GUARD:GUARD + n].view(B, K1, v + PAD)[:, :, :v]            # noqa: E731
        for t, value in c["poison"]:
            view(buf)[:, :, t] = value
        want = buf.clone()
        ref_dry(view(want), rows, c["brk"], tokens, seq_len, [START - len(c["real"])] * B, START, max_len, step if with_tok else None, n_prev)
        dev = buf.cuda()
        K_.dry_rows(view(dev), packed, torch.from_numpy(tokens).cuda(), torch.tensor(seq_len, dtype=torch.int32).cuda(), max_len,
                    torch.from_numpy(step).cuda() if with_tok else None, n_prev)
        torch.cuda.synchronize()
        assert _bits(dev) == _bits(want), (K1, n_prev)
        assert _bits(view(dev)[1]) == _bits(view(buf)[1])                             # the row that is off
        changed |= _bits(want) != _bits(buf)
    assert changed != c["quiet"]                                                      # never vacuous: the case penalises something


INVALID, UNSUPPORTED, ALIGNMENT = -1, -2, -5


@pytest.mark.parametrize("kw,status", [
    (dict(B=-1), INVALID), (dict(B=0, logits=None), 0), (dict(dtype=7, logits=None), UNSUPPORTED), (dict(n_tok=65, ld_tok=65), UNSUPPORTED),
    (dict(max_len=2 ** 31 - 4000, ld_tokens=2 ** 31), UNSUPPORTED), (dict(recs=None), INVALID), (dict(ld_row=V - 1), INVALID),
    (dict(ld_tokens=7), INVALID), (dict(tok=None), INVALID), (dict(n_prev=4), INVALID), (dict(recs=2), ALIGNMENT), (dict(seq_len=2), ALIGNMENT),
    (dict(), 0)], ids=str)
def test_argument_checks_return_their_status(kw, status):
    from asd_amd import _binding, kernels as K_
    lib, B = _binding.load_library(), 3
    x = torch.randn((B, 2, V), device="cuda")
    keep = x.clone()
    packed = K_.pack_dry([1.0, 0.0, 1.0], [1.0] * 3, [1] * 3, [0] * 3, (), [0] * 3, 4, "cuda")
    tokens = torch.ones((B, 8), dtype=torch.int32, device="cuda")
    seq = torch.full((B,), 6, dtype=torch.int32, device="cuda")
    tok = torch.full((B, 4), 7, dtype=torch.int32, device="cuda")
    good = dict(logits=x.data_ptr(), dtype=0, ld_seq=2 * V, ld_row=V, B=B, K1=2, V=V, recs=packed.table.data_ptr(), row_start=None,
                tokens=tokens.data_ptr(), ld_tokens=8, seq_len=seq.data_ptr(), start=4, max_len=8, tok=tok.data_ptr(), ld_tok=4,
                n_tok=4, n_prev=3, stream=None)
    for name, v in kw.items():                                                        # (an int for a pointer: that many bytes off)
        good[name] = good[name] + v if name in ("recs", "seq_len") and v is not None else v
    assert lib.asd_dry_rows(*good.values()) == status
    torch.cuda.synchronize()
    if kw:
        assert torch.equal(x, keep)                                                   # nothing was launched
    else:                                                                             # H = 1 1 | 7 7 7: rows 0 and 2 lose 1 at id 7
        assert torch.equal(x[1], keep[1]) and torch.equal(x[::2, :, 7], keep[::2, :, 7] - 1.0) and torch.equal(x[..., :7], keep[..., :7]) and torch.equal(x[..., 8:], keep[..., 8:])
