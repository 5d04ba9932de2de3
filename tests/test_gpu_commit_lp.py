"""asd_commit_step_lp: asd_commit_step with the log-probs scattered beside the tokens.  Integer / bit-copy work, so everything
is exact: tokens, lengths and counts equal asd_commit_step's on the same inputs; out_lp carries the source BITS at exactly the
committed positions and the sentinel everywhere else; argument errors give asd_commit_step's status codes."""
import numpy as np
import pytest

from tests.stage_scenario import ref_commit_lp

pytestmark = pytest.mark.gpu

SENT_TOK = -123456
SENT_LP = np.float32(-7.25)


def _inputs(B, K, seed):
    rng = np.random.default_rng(seed)
    T = K + 12
    max_len = T - 2                                    # rows are longer than max_len: nothing past max_len may be written
    tok = rng.integers(0, 152064, (B, K)).astype(np.int32)
    lp_tok = (-rng.uniform(0, 20, (B, K))).astype(np.float32)
    if K:
        lp_tok.reshape(-1)[::3] = -np.inf              # bits, not values: -inf, NaN payloads and -0.0 travel unchanged
        lp_tok.reshape(-1)[1::5] = np.float32(-0.0)
    drawn = rng.integers(0, 152064, B).astype(np.int32)
    lp_drawn = (-rng.uniform(0, 20, B)).astype(np.float32)
    lp_drawn[::4] = np.nan
    n_acc = rng.integers(0, K + 1, B).astype(np.int32)
    n_acc[0] = 0
    n_acc[-1] = K
    if B >= 5:
        n_acc[1], n_acc[2] = -3, K + 5                 # out of range: clamped to [0, K]
    # lengths so that the clamp cuts inside the prefix, at the drawn token, before both, and not at all
    seq_len = rng.integers(0, 4, B).astype(np.int32)
    na = np.clip(n_acc, 0, K)
    for b in range(B):
        mode = b % 4
        if mode == 1:
            seq_len[b] = max_len - na[b]               # the drawn token is the first one dropped
        elif mode == 2:
            seq_len[b] = max(max_len - max(na[b] // 2, 0), 0) if na[b] else max_len    # cut inside the prefix
        elif mode == 3 and b % 8 == 3:
            seq_len[b] = max_len                       # nothing fits
    if B >= 5:
        seq_len[4] = max_len + 1                       # negative room (T = max_len + 2): the row is left as it is
    return tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, T, max_len


@pytest.mark.parametrize("K", [0, 1, 8, 64])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_commit_step_lp_matches_commit_step_and_the_scatter_reference(B, K):
    import torch
    from asd_amd import kernels as Kn
    tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, T, max_len = _inputs(B, K, seed=B * 100 + K)
    dev = lambda a: torch.from_numpy(a).cuda()            # noqa: E731
    out_tok0 = np.full((B, T), SENT_TOK, np.int32)
    out_lp0 = np.full((B, T), SENT_LP, np.float32)
    # the parent's call on the same inputs
    len_a, tok_a, nc_a = dev(seq_len.copy()), dev(out_tok0.copy()), torch.full((B,), -9, dtype=torch.int32, device="cuda")
    Kn.commit_step(dev(tok), dev(n_acc), dev(drawn), len_a, tok_a, nc_a, max_len=max_len)
    len_b, tok_b, lp_b = dev(seq_len.copy()), dev(out_tok0.copy()), dev(out_lp0.copy())
    nc_b = torch.full((B,), -9, dtype=torch.int32, device="cuda")
    Kn.commit_step_lp(dev(tok) if K else None, dev(lp_tok) if K else None, dev(n_acc), dev(drawn), dev(lp_drawn), len_b, tok_b,
                      lp_b, nc_b, max_len=max_len)
    torch.cuda.synchronize()
    assert torch.equal(len_a, len_b) and torch.equal(tok_a, tok_b) and torch.equal(nc_a, nc_b)
    want_len, want_tok, want_lp, want_nc = ref_commit_lp(tok if K else None, lp_tok if K else None, n_acc, drawn, lp_drawn, seq_len,
                                                         out_tok0, out_lp0, max_len)
    assert np.array_equal(len_b.cpu().numpy(), want_len) and np.array_equal(nc_b.cpu().numpy(), want_nc)
    assert np.array_equal(tok_b.cpu().numpy(), want_tok)
    got_lp = lp_b.cpu().numpy()
    assert got_lp.view(np.uint32).tobytes() == want_lp.view(np.uint32).tobytes()
    assert (got_lp[:, max_len:].view(np.uint32) == SENT_LP.view(np.uint32)).all()      # nothing past max_len
    written = got_lp.view(np.uint32) != SENT_LP.view(np.uint32)
    assert written.sum() <= want_nc.sum()              # the sentinel everywhere outside the committed positions
    # n_commit may be NULL
    len_c, tok_c, lp_c = dev(seq_len.copy()), dev(out_tok0.copy()), dev(out_lp0.copy())
    Kn.commit_step_lp(dev(tok) if K else None, dev(lp_tok) if K else None, dev(n_acc), dev(drawn), dev(lp_drawn), len_c, tok_c,
                      lp_c, None, max_len=max_len)
    torch.cuda.synchronize()
    assert torch.equal(len_c, len_b) and torch.equal(tok_c, tok_b) and lp_c.cpu().numpy().tobytes() == got_lp.tobytes()


def test_argument_errors_are_commit_steps():
    import torch
    from asd_amd import _binding
    lib = _binding.load_library()
    B, K, T = 4, 8, 32
    z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device="cuda")     # noqa: E731
    tok, lp_tok, n_acc, drawn, lp_drawn = z(B, K), z(B, K, dt=torch.float32), z(B), z(B), z(B, dt=torch.float32)
    seq_len, out, out_lp, nc = z(B), z(B, T), z(B, T, dt=torch.float32), z(B)
    p = lambda t: None if t is None else t.data_ptr()                          # noqa: E731

    def both(B_=B, K_=K, tok_=tok, n_acc_=n_acc, drawn_=drawn, seq_=seq_len, out_=out, ld=T, max_len=T):
        a = lib.asd_commit_step(p(tok_), p(n_acc_), p(drawn_), B_, K_, p(seq_), p(out_), ld, p(nc), max_len, None)
        b = lib.asd_commit_step_lp(p(tok_), p(lp_tok), p(n_acc_), p(drawn_), p(lp_drawn), B_, K_, p(seq_), p(out_), p(out_lp), ld,
                                   p(nc), max_len, None)
        return a, b

    cases = [dict(B_=-1), dict(K_=-1), dict(max_len=-1), dict(B_=0), dict(K_=65), dict(tok_=None), dict(n_acc_=None),
             dict(drawn_=None), dict(seq_=None), dict(out_=None), dict(ld=T - 1), dict(K_=0, tok_=None), dict()]
    seen = set()
    for kw in cases:
        a, b = both(**kw)
        assert a == b, (kw, a, b)
        seen.add(a)
    assert {0, -1} <= seen and len(seen) >= 3          # ok, invalid argument, unsupported
    # the arguments only the new call has
    bad = lib.asd_commit_step(None, p(n_acc), p(drawn), B, K, p(seq_len), p(out), T, p(nc), T, None)
    for kw in (dict(lp_tok=None), dict(lp_drawn=None), dict(out_lp=None)):
        a = dict(lp_tok=p(lp_tok), lp_drawn=p(lp_drawn), out_lp=p(out_lp))
        a.update(kw)
        rc = lib.asd_commit_step_lp(p(tok), a["lp_tok"], p(n_acc), p(drawn), a["lp_drawn"], B, K, p(seq_len), p(out), a["out_lp"],
                                    T, p(nc), T, None)
        assert rc == bad
    torch.cuda.synchronize()
