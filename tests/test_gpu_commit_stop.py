"""asd_commit_step_stop through kernels.commit_step_stop against the numpy reference of tests/stop_scenario.py.  Integer / bit-copy
work, so everything is exact: tokens, log-prob bits, seq_len, n_commit, finished, n_finished; the sentinel stays everywhere the
reference leaves it.  The inputs are CONSTRUCTED: every row of a case is given one scenario of `SCENARIOS` (where K and n_stop allow
it), and `test_every_scenario_occurs` checks on the reference's outputs that each of them really happens somewhere in the grid."""
import numpy as np
import pytest

from tests.stop_scenario import LENGTH, STOP, ref_commit_stop

pytestmark = pytest.mark.gpu

SENT_TOK = -123456
SENT_LP = np.float32(-7.25)
VOCAB = 152064
STOP_POOL = np.array([151645, 151643, 0, 7, 99, 31, 64, 2], np.int32)       # every random token is drawn from [100, 151000)
BS, KS, NSTOPS = (1, 5, 64), (0, 1, 8, 64), (0, 1, 2, 8)
N_FINISHED_0 = 5                                                            # the counter is added to, not set

SCENARIOS = ("stop_at_lane_0", "stop_at_lane_na_minus_1", "stop_is_drawn", "stop_in_prefix_and_drawn", "stop_only_rejected",
             "stop_on_last_free_slot", "stop_one_past_max_len", "enters_full", "enters_stopped", "enters_at_length", "drawn_minus_1",
             "n_acc_negative", "n_acc_above_k", "plain")


def _inputs(B, K, n_stop):
    rng = np.random.default_rng(B * 10000 + K * 100 + n_stop)
    T = K + 12
    max_len = T - 2                                    # rows are longer than max_len: nothing past max_len may be written
    stops = STOP_POOL[:n_stop].copy()
    tok = rng.integers(100, 151000, (B, K)).astype(np.int32)
    lp_tok = (-rng.uniform(0, 20, (B, K))).astype(np.float32)
    if K:
        lp_tok.reshape(-1)[::3] = -np.inf              # bits, not values
        lp_tok.reshape(-1)[1::5] = np.float32(-0.0)
    drawn = rng.integers(100, 151000, B).astype(np.int32)
    lp_drawn = (-rng.uniform(0, 20, B)).astype(np.float32)
    lp_drawn[::4] = np.nan
    n_acc = rng.integers(0, K + 1, B).astype(np.int32)
    seq_len = rng.integers(0, 4, B).astype(np.int32)
    finished = np.zeros(B, np.int32)
    first = (K + 3 * n_stop) % len(SCENARIOS)          # B = 1 and B = 5 start somewhere else in every case
    for b in range(B):
        name = SCENARIOS[(first + b) % len(SCENARIOS)]
        s = (lambda i: stops[i % n_stop]) if n_stop else None
        if name == "stop_at_lane_0" and s and K >= 1:
            n_acc[b], tok[b, 0] = min(K, 3), s(b)
        elif name == "stop_at_lane_na_minus_1" and s and K >= 2:
            n_acc[b], tok[b, K - 1] = K, s(b + 1)      # K = 64: lane 63, the top bit of the ballot
        elif name == "stop_is_drawn" and s:
            drawn[b] = s(n_stop // 2)
        elif name == "stop_in_prefix_and_drawn" and s and K >= 2:
            n_acc[b], tok[b, 1], drawn[b] = K, s(0), s(n_stop - 1)
        elif name == "stop_only_rejected" and s and K >= 2:
            n_acc[b], tok[b, 1:] = 1, s(b)
        elif name == "stop_on_last_free_slot" and s:
            drawn[b], seq_len[b] = s(b), max_len - n_acc[b] - 1
        elif name == "stop_one_past_max_len" and s and K >= 1:
            n_acc[b], drawn[b], seq_len[b] = K, s(b), max_len - K
        elif name == "enters_full":
            seq_len[b] = max_len
        elif name in ("enters_stopped", "enters_at_length"):
            finished[b] = STOP if name == "enters_stopped" else LENGTH
            if s:
                drawn[b] = s(0)
        elif name == "drawn_minus_1":
            drawn[b] = -1
        elif name == "n_acc_negative":
            n_acc[b] = -3
        elif name == "n_acc_above_k":
            n_acc[b] = K + 5
    if B >= 5:                                         # on top of row 4's scenario: negative room (T = max_len + 2)
        seq_len[4], finished[4] = max_len + 1, 0
    return dict(tok=tok, lp_tok=lp_tok, n_acc=n_acc, drawn=drawn, lp_drawn=lp_drawn, seq_len=seq_len, finished=finished,
                stops=stops, T=T, max_len=max_len)


def _reference(c, seq_len=None, out_tok=None, out_lp=None, finished=None, n_finished=N_FINISHED_0):
    B, K = c["tok"].shape
    return ref_commit_stop(c["tok"] if K else None, c["lp_tok"] if K else None, c["n_acc"], c["drawn"], c["lp_drawn"],
                           c["seq_len"] if seq_len is None else seq_len,
                           np.full((B, c["T"]), SENT_TOK, np.int32) if out_tok is None else out_tok,
                           np.full((B, c["T"]), SENT_LP, np.float32) if out_lp is None else out_lp,
                           c["finished"] if finished is None else finished, n_finished, c["stops"], c["max_len"])


def _what_happened(c, ref):
    """Labels of what the reference did with every row, from the inputs and its outputs alone (not from the scenario names)."""
    seen = set()
    B, K = c["tok"].shape
    stops = set(c["stops"].tolist())
    ln, _, _, nc, fin, _ = ref
    for b in range(B):
        if c["finished"][b]:
            assert nc[b] == 0 and ln[b] == c["seq_len"][b] and fin[b] == c["finished"][b]
            seen.add("enters_stopped" if c["finished"][b] == STOP else "enters_at_length")
            continue
        raw, length = int(c["n_acc"][b]), int(c["seq_len"][b])
        na = min(max(raw, 0), K)
        prefix_hits = [k for k in range(na) if int(c["tok"][b, k]) in stops]
        drawn_hit = int(c["drawn"][b]) in stops
        rejected_hits = [k for k in range(na, K) if int(c["tok"][b, k]) in stops]
        room = c["max_len"] - length
        if raw < 0:
            seen.add("n_acc_negative")
        if raw > K:
            seen.add("n_acc_above_k")
        if room == 0:
            assert fin[b] == LENGTH and nc[b] == 0
            seen.add("enters_full")
        if room < 0:                                   # ends for its length, nothing appended, counted like any row that ends
            assert fin[b] == LENGTH and nc[b] == 0 and ln[b] == length
            seen.add("enters_past_max_len")
        if c["drawn"][b] == -1 and stops and not prefix_hits:
            assert fin[b] != STOP
            seen.add("drawn_minus_1")
        if rejected_hits and not prefix_hits and not drawn_hit:
            assert fin[b] != STOP and nc[b] == min(na + 1, max(room, 0))
            seen.add("stop_only_rejected")
        if fin[b] == STOP:
            j = int(nc[b]) - 1
            if j == 0 and na >= 1:
                seen.add("stop_at_lane_0")
            if j == na - 1 and na >= 2:
                seen.add("stop_at_lane_na_minus_1")
            if j == 63 and na == 64:
                seen.add("stop_at_lane_63")
            if j == na:
                seen.add("stop_is_drawn")
            if j < na and drawn_hit and room > na:
                seen.add("stop_in_prefix_and_drawn")
            if length + j + 1 == c["max_len"]:
                seen.add("stop_on_last_free_slot")
        elif fin[b] == LENGTH and 0 < room <= na and not [k for k in prefix_hits if k < room]:
            cut = int(c["tok"][b, room]) if room < na else int(c["drawn"][b])
            if cut in stops:
                seen.add("stop_one_past_max_len")
    return seen


def test_every_scenario_occurs():
    seen = set()
    for B in BS:
        for K in KS:
            for n_stop in NSTOPS:
                c = _inputs(B, K, n_stop)
                seen |= _what_happened(c, _reference(c))
    assert seen >= (set(SCENARIOS) - {"plain"}) | {"stop_at_lane_63", "enters_past_max_len"}, sorted(set(SCENARIOS) - seen)


def _device_call(c, seq_len, out_tok, out_lp, finished, n_finished, n_commit=True):
    import torch
    from asd_amd import kernels as Kn
    K = c["tok"].shape[1]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()            # noqa: E731
    nc = torch.full((len(seq_len),), -9, dtype=torch.int32, device="cuda") if n_commit else None
    Kn.commit_step_stop(dev(c["tok"]) if K else None, dev(c["lp_tok"]) if K else None, dev(c["n_acc"]), dev(c["drawn"]),
                        dev(c["lp_drawn"]), seq_len, out_tok, out_lp, finished, stop_ids=dev(c["stops"]) if len(c["stops"]) else None,
                        n_finished=n_finished, n_commit=nc, max_len=c["max_len"])
    torch.cuda.synchronize()
    return nc


def _assert_equal(got, want):
    names = ("seq_len", "tokens", "lps", "n_commit", "finished", "n_finished")
    for name, g, w in zip(names, got, want):
        g = g.cpu().numpy()
        w = np.asarray(w, dtype=g.dtype).reshape(g.shape)
        assert g.tobytes() == w.tobytes(), name


@pytest.mark.parametrize("n_stop", NSTOPS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("B", BS)
def test_commit_step_stop_matches_the_reference(B, K, n_stop):
    import torch
    c = _inputs(B, K, n_stop)
    dev = lambda a: torch.from_numpy(a).cuda()            # noqa: E731
    seq_len, finished = dev(c["seq_len"].copy()), dev(c["finished"].copy())
    out_tok, out_lp = dev(np.full((B, c["T"]), SENT_TOK, np.int32)), dev(np.full((B, c["T"]), SENT_LP, np.float32))
    n_finished = torch.full((1,), N_FINISHED_0, dtype=torch.int32, device="cuda")
    nc = _device_call(c, seq_len, out_tok, out_lp, finished, n_finished)
    want = _reference(c)
    _assert_equal((seq_len, out_tok, out_lp, nc, finished, n_finished), want)
    assert (out_tok.cpu().numpy()[:, c["max_len"]:] == SENT_TOK).all()          # nothing past max_len
    # a second call on the outputs of the first: finished rows and what they added to the counter stay as they are
    first = [t.clone() for t in (seq_len, out_tok, out_lp, finished)]
    nc2 = _device_call(c, seq_len, out_tok, out_lp, finished, n_finished)
    want2 = _reference(c, *want[:3], finished=want[4], n_finished=want[5])
    _assert_equal((seq_len, out_tok, out_lp, nc2, finished, n_finished), want2)
    done = first[3] != 0
    assert torch.equal(finished[done], first[3][done]) and torch.equal(seq_len[done], first[0][done])
    assert torch.equal(out_tok[done], first[1][done]) and (nc2[done] == 0).all()
    assert out_lp[done].cpu().numpy().tobytes() == first[2][done].cpu().numpy().tobytes()
    assert int(n_finished.item()) == N_FINISHED_0 + int((finished != 0).sum().item()) - int(c["finished"].astype(bool).sum())
    # n_commit and n_finished may be NULL
    seq_c, fin_c = dev(c["seq_len"].copy()), dev(c["finished"].copy())
    tok_c, lp_c = dev(np.full((B, c["T"]), SENT_TOK, np.int32)), dev(np.full((B, c["T"]), SENT_LP, np.float32))
    _device_call(c, seq_c, tok_c, lp_c, fin_c, None, n_commit=False)
    _assert_equal((seq_c, tok_c, lp_c), want[:3])
    _assert_equal((fin_c,), want[4:5])


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("B", BS)
def test_without_a_stop_set_it_is_commit_step_lp(B, K):
    import torch
    from asd_amd import kernels as Kn
    c = _inputs(B, K, 0)
    c["finished"][:] = 0
    dev = lambda a: torch.from_numpy(a).cuda()            # noqa: E731
    outs = []
    for stop in (False, True):
        seq_len, nc = dev(c["seq_len"].copy()), torch.full((B,), -9, dtype=torch.int32, device="cuda")
        out_tok, out_lp = dev(np.full((B, c["T"]), SENT_TOK, np.int32)), dev(np.full((B, c["T"]), SENT_LP, np.float32))
        args = (dev(c["tok"]) if K else None, dev(c["lp_tok"]) if K else None, dev(c["n_acc"]), dev(c["drawn"]), dev(c["lp_drawn"]),
                seq_len, out_tok, out_lp)
        if stop:
            Kn.commit_step_stop(*args, torch.zeros((B,), dtype=torch.int32, device="cuda"), n_commit=nc, max_len=c["max_len"])
        else:
            Kn.commit_step_lp(*args, nc, max_len=c["max_len"])
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy().tobytes() for t in (out_tok, out_lp, seq_len, nc)])
    assert outs[0] == outs[1]


def test_argument_errors():
    import torch
    from asd_amd import _binding
    lib = _binding.load_library()
    B, K, T = 4, 8, 32
    z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device="cuda")     # noqa: E731
    tok, lp_tok, n_acc, drawn, lp_drawn = z(B, K), z(B, K, dt=torch.float32), z(B), z(B), z(B, dt=torch.float32)
    seq_len, out, out_lp, nc, fin, nfin, stops = z(B), z(B, T), z(B, T, dt=torch.float32), z(B), z(B), z(1), z(8) - 1
    p = lambda t: None if t is None else t.data_ptr()                          # noqa: E731

    def stop(B_=B, K_=K, tok_=tok, lp_tok_=lp_tok, n_acc_=n_acc, drawn_=drawn, lp_drawn_=lp_drawn, seq_=seq_len, out_=out,
             out_lp_=out_lp, ld=T, max_len=T, stops_=stops, n_stop=2, fin_=fin, nfin_=nfin, nc_=nc):
        return lib.asd_commit_step_stop(p(tok_), p(lp_tok_), p(n_acc_), p(drawn_), p(lp_drawn_), B_, K_, p(stops_), n_stop, p(seq_),
                                        p(out_), p(out_lp_), ld, p(nc_), p(fin_), p(nfin_), max_len, None)

    def lp(B_=B, K_=K, tok_=tok, lp_tok_=lp_tok, n_acc_=n_acc, drawn_=drawn, lp_drawn_=lp_drawn, seq_=seq_len, out_=out,
           out_lp_=out_lp, ld=T, max_len=T):
        return lib.asd_commit_step_lp(p(tok_), p(lp_tok_), p(n_acc_), p(drawn_), p(lp_drawn_), B_, K_, p(seq_), p(out_), p(out_lp_),
                                      ld, p(nc), max_len, None)

    # the cases of tests/test_gpu_commit_lp.py::test_argument_errors_are_commit_steps, and the pointers asd_commit_step_lp added
    cases = [dict(B_=-1), dict(K_=-1), dict(max_len=-1), dict(B_=0), dict(K_=65), dict(tok_=None), dict(n_acc_=None),
             dict(drawn_=None), dict(seq_=None), dict(out_=None), dict(ld=T - 1), dict(K_=0, tok_=None), dict(),
             dict(lp_tok_=None), dict(lp_drawn_=None), dict(out_lp_=None), dict(K_=0, tok_=None, lp_tok_=None)]
    seen = set()
    for kw in cases:
        a, b = lp(**kw), stop(**kw)
        assert a == b, (kw, a, b)
        seen.add(a)
    ok, invalid, unsupported = lp(), lp(B_=-1), lp(K_=65)
    assert ok == 0 and seen >= {ok, invalid, unsupported} and len({ok, invalid, unsupported}) == 3
    # the arguments only the new call has
    assert stop(fin_=None) == invalid
    assert stop(n_stop=-1) == invalid
    assert stop(stops_=None, n_stop=1) == invalid
    assert stop(n_stop=9) == unsupported
    assert stop(n_stop=8) == ok and stop(stops_=None, n_stop=0) == ok and stop(nfin_=None, nc_=None) == ok
    torch.cuda.synchronize()
