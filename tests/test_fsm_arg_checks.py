"""Guided decoding, host side (serving/guided.py, serving/stage_args.py, kernels.check_fsm_tables): every ValueError the module
docstring of serving/stages.py names under GUIDED DECODING, raised before any launch and before the prompts are encoded; the
compiled form of a small trie; state_bits against delta; the limits; the rule that a row keeps a token."""
import numpy as np
import pytest

import asd_amd
from asd_amd import kernels as K
from asd_amd.serving.guided import MAX_FSM_STATES, TokenFSM, compile_rows
from asd_amd.serving.stages import StageManager
from tests.fsm_ref import FsmOracleOps, ref_delta, ref_state_bits, tables_of
from tests.oracle_backend import OracleBackend
from tests.stage_scenario import NAMES, PROMPTS, stage_configs

V = 1000


@pytest.fixture(autouse=True)
def oracle_backend():
    asd_amd.set_backend(OracleBackend())
    yield
    asd_amd.set_backend(None)


class _NoLaunch(FsmOracleOps):
    def _note(self, name, args):
        raise AssertionError(f"{name} was called before the arguments were refused")


@pytest.fixture(scope="module")
def stage():
    return StageManager(stage_configs(), ops=_NoLaunch()).get_stage(NAMES[1])


def _refused(stage, match, **kw):
    def no_encode(*a, **k):
        raise AssertionError("the prompts were encoded before the arguments were refused")
    stage._encode, keep = no_encode, stage._encode
    try:
        with pytest.raises(ValueError, match=match):
            stage.generate(prompts=PROMPTS, max_tokens=8, **{"stop_token_ids": [2], **kw})
    finally:
        stage._encode = keep


def test_token_fsm_refuses_bad_ids_and_states():
    for bad in (dict(n_states=0), dict(n_states=True), dict(start=2), dict(start=-1), dict(start=True),
                dict(edges=[{True: 1}, {}]), dict(edges=[{1.5: 1}, {}]), dict(edges=[{-1: 1}, {}]), dict(edges=[{3: 2}, {}]),
                dict(edges=[{3: -2}, {}]), dict(edges=[{3: True}, {}]), dict(edges=[{}]), dict(edges={2: {1: 0}}),
                dict(other=[0]), dict(other=[0, 2]), dict(other=[0, 1.0]), dict(accepting=[2]), dict(accepting=[True]), dict(accepting="0")):
        with pytest.raises(ValueError):
            TokenFSM(**{**dict(n_states=2, start=0, edges=[{3: 1}, {}], other=None, accepting=[1]), **bad})
    f = TokenFSM(2, 0, {0: {3: 1}}, [-1, 1], accepting=(1,))                       # a dict of states; np integers pass
    assert f.edges == [{3: 1}, {}] and f.other == [-1, 1] and f == TokenFSM(2, np.int64(0), [{np.int32(3): 1}, None], [-1, 1], {1})


def test_from_choices_builds_the_trie():
    f = TokenFSM.from_choices([(5, 17, 300), [5, 17], (5, 900), (5, 17, 300)])     # the duplicate is dropped
    assert f.n_states == 5 and f.start == 0 and f.other == [-1] * 5
    assert f.edges == [{5: 1}, {17: 2, 900: 4}, {300: 3}, {}, {}] and f.accepting == {2, 3, 4}    # 2: a choice that is a prefix
    for bad in ("abc", 5, [], [()], [tuple(range(65))], [(1, True)], [(1, 2.0)], [(-1,)], [5], [[(1, 2)]], ["text"],
                [(i,) for i in range(257)]):
        with pytest.raises(ValueError):
            TokenFSM.from_choices(bad)
    assert TokenFSM.from_choices([(i,) for i in range(256)]).n_states == 257 and TokenFSM.from_choices([tuple(range(64))]).n_states == 65
    with pytest.raises(ValueError):
        TokenFSM.from_choices([(V,)], vocab=V)


def test_generate_refuses_before_any_launch(stage):
    ok = TokenFSM.from_choices([(5, 6)])
    _refused(stage, "vocab|lie in", guided_fsm=TokenFSM(1, 0, [{V: 0}]))
    _refused(stage, "lie in", guided_choice=[(V,)])
    _refused(stage, "guided_fsm", guided_fsm=[ok] * 4)
    _refused(stage, "guided_fsm", guided_fsm=[ok, None, "x", None, None])
    _refused(stage, "guided_fsm", guided_fsm="abc")
    _refused(stage, "guided_choice", guided_choice="abc")
    _refused(stage, "guided_choice_per_prompt", guided_choice_per_prompt=[[(1,)]] * 4)
    _refused(stage, "guided_choice_per_prompt", guided_choice_per_prompt=["abc", None, None, None, None])
    _refused(stage, "guided_choice_per_prompt", guided_choice_per_prompt="abcde")
    _refused(stage, "not both", guided_fsm=ok, guided_choice=[(1,)])
    _refused(stage, "not both", guided_fsm=[ok, None, None, None, None], guided_choice_per_prompt=[[(1,)], None, None, None, None])
    _refused(stage, "both name", guided_choice=[(1,)], guided_choice_per_prompt=[[(1,)], None, None, None, None])
    _refused(stage, "min_tokens", guided_choice=[(5, 6)], min_tokens=1)
    _refused(stage, "min_tokens", guided_choice_per_prompt=[None, [(5, 6)], None, None, None], min_tokens=[0, 2, 0, 0, 0])
    # a row's own min_tokens on an unguided row is fine; the call then fails only at the first op
    with pytest.raises(AssertionError, match="was called"):
        stage.generate(prompts=PROMPTS, max_tokens=8, stop_token_ids=[2], guided_choice_per_prompt=[None, [(5, 6)], None, None, None],
                       min_tokens=[3, 0, 0, 0, 0])


def test_choices_need_a_stop_id_and_a_dead_end_is_refused(stage):
    _refused(stage, "needs a stop id", guided_choice=[(5, 6)], stop_token_ids=[])
    _refused(stage, "needs a stop id", guided_choice=[(5, 6)], stop_token_ids=[], stop_sequences=[(2, 3)])    # no ONE-token entry
    _refused(stage, "keeps no token", guided_fsm=TokenFSM(2, 0, [{5: 1}, {}]))                     # a non-accepting dead end
    _refused(stage, "keeps no token", guided_fsm=TokenFSM(2, 0, [{5: 1}, {}], accepting=[1]), stop_token_ids=[])
    # ... against an allow-list, a ban and a bad word's last id, each emptying one reachable state
    _refused(stage, "keeps no token", guided_choice=[(5, 6), (7,)], allowed_token_ids=[5, 7, 2])
    _refused(stage, "keeps no token", guided_choice=[(5, 6), (7,)], banned_token_ids=[6])
    _refused(stage, "keeps no token", guided_choice=[(5, 6), (7,)], bad_words=[(900, 6)])
    _refused(stage, "keeps no token", guided_choice=[(5, 6), (7,)], banned_token_ids=[2])           # the accepting leaves keep only the stop id
    with pytest.raises(AssertionError, match="was called"):                                        # the same call with enough left passes
        stage.generate(prompts=PROMPTS, max_tokens=8, stop_token_ids=[2], guided_choice=[(5, 6), (7,)], allowed_token_ids=[5, 6, 7, 2],
                       banned_token_ids=[9], bad_words=[(900, 8)])
    # an unreachable state may be empty
    with pytest.raises(AssertionError, match="was called"):
        stage.generate(prompts=PROMPTS, max_tokens=8, stop_token_ids=[2], guided_fsm=TokenFSM(3, 0, [{5: 1}, {}, {}], accepting=[1]))


def test_the_compiled_form_of_a_small_trie():
    f = TokenFSM.from_choices([(5, 6), (5,)])                                      # 0 -5-> 1 (accepting) -6-> 2 (accepting)
    g = TokenFSM(2, 1, [{9: 1}, {}], other=[-1, 0], accepting=[0])                 # state 1: everything goes to 0; 0: 9 -> 1
    c = compile_rows([f, None, f, g, f], [[2, 3], [2], [3, 2], [2], [2]], V)
    # rows 0 and 2 share (f, {2, 3}): states 0..3 (END appended); g: 4..6, started in its state 1; row 4 has another Z: 7..10
    assert c.starts == [0, -1, 0, 4 + 1, 7] and c.S == 4 + 3 + 4
    first, tok, nxt = c.state_first.tolist(), c.edge_tok.tolist(), c.edge_next.tolist()
    edges = [dict(zip(tok[first[s]:first[s + 1]], nxt[first[s]:first[s + 1]])) for s in range(c.S)]
    assert edges[0] == {2: -1, 3: -1, 5: 1}                                        # not accepting: the stop ids are forbidden
    assert edges[1] == {2: 3, 3: 3, 6: 2} and edges[2] == {2: 3, 3: 3}             # accepting: stop edges to END
    assert edges[3] == {2: 3, 3: 3} and c.state_other[:4].tolist() == [-1] * 4     # END allows exactly Z and loops
    assert edges[7] == {2: -1, 5: 8} and edges[8] == {2: 10, 6: 9} and edges[9] == edges[10] == {2: 10}
    # g: in state 1 (not accepting) the stop id is forbidden EVEN UNDER `other`; in state 0 (accepting) it leads to END
    assert edges[4] == {2: 6, 9: 5} and edges[5] == {2: -1} and edges[6] == {2: 6} and c.state_other[4:7].tolist() == [-1, 4, -1]
    assert all(tok[first[s]:first[s + 1]] == sorted(set(tok[first[s]:first[s + 1]])) for s in range(c.S))
    assert c.step(5, 2) == 5 and c.step(5, 500) == 4 and c.step(4, 2) == 6 and c.step(6, 2) == 6 and c.step(6, 5) == 6
    assert c.step(-1, 5) == -1 and c.step(0, V) == 0 and c.step(0, 5) == 1
    # an explicit edge on a stop id stays as it was written
    h = compile_rows([TokenFSM(2, 0, [{2: 1, 3: -1}, {}], accepting=[0, 1])], [[2, 3]], V)
    assert dict(zip(h.edge_tok[:2].tolist(), h.edge_next[:2].tolist())) == {2: 1, 3: -1}


def test_state_bits_agree_with_delta_for_every_state_and_token():
    Vs = 70
    g = TokenFSM(3, 0, [{0: 1, 31: -1, 32: 2, 69: 0}, {5: -1, 64: 1}, {}], other=[-1, 2, -1], accepting=[2])
    c = compile_rows([g], [[33]], Vs)
    first, tok, nxt, other, bits, starts = K.check_fsm_tables(c.state_first, c.edge_tok, c.edge_next, c.state_other, c.starts, Vs)
    t = tables_of(first, tok, nxt, other, Vs)
    assert bits.shape == (4, 3) and bits.dtype == np.uint32 and np.array_equal(bits, ref_state_bits(t)) and starts == [0]
    for s in range(t.S):
        lo, hi = int(first[s]), int(first[s + 1])
        for v in range(Vs):
            to = dict(zip(tok[lo:hi].tolist(), nxt[lo:hi].tolist())).get(v, int(other[s]))
            bit = bool((int(bits[s, v >> 5]) >> (v & 31)) & 1)
            assert bit == (to >= 0) == bool(c.allowed(s)[v]), (s, v)
            assert ref_delta(t, s, v) == (to if to >= 0 else s) == c.step(s, v), (s, v)
        assert int(bits[s, 2]) >> (Vs - 64) == 0                                   # nothing set behind V
    for bad in (dict(state_first=[0, 1]), dict(edge_tok=c.edge_tok[::-1].copy()), dict(edge_next=[4] * c.E), dict(state_other=[-2, 0, 0, 0]),
                dict(starts=[4]), dict(V=60)):
        with pytest.raises(ValueError):
            K.check_fsm_tables(**{**dict(state_first=c.state_first, edge_tok=c.edge_tok, edge_next=c.edge_next, state_other=c.state_other,
                                         starts=c.starts, V=Vs), **bad})


def test_the_limits(stage):
    chain = lambda n: TokenFSM(n, 0, [{1: min(s + 1, n - 1)} for s in range(n)], accepting=[n - 1])     # noqa: E731
    assert compile_rows([chain(MAX_FSM_STATES - 1)], [[2]], V).S == MAX_FSM_STATES
    with pytest.raises(ValueError, match="at most 1024 states"):
        compile_rows([chain(MAX_FSM_STATES)], [[2]], V)
    with pytest.raises(ValueError, match="at most 1024 states"):                   # two automata of one call share the space
        compile_rows([chain(600), chain(601)], [[2], [2]], V)
    assert compile_rows([chain(600), chain(600)], [[2], [2]], V).S == 601           # ... unless they are the same one
    wide = TokenFSM(8, 0, [{t: s for t in range(152064 - 8)} for s in range(8)], accepting=[0])
    with pytest.raises(ValueError, match="edges"):
        compile_rows([wide], [[152063]], 152064)                                   # 8 x 152 056 > 2^20
    _refused(stage, "at most 1024 states", guided_fsm=chain(MAX_FSM_STATES))
