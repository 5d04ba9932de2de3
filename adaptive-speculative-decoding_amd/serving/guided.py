"""Guided decoding, host side (serving/stages.py, GUIDED DECODING; include/asd_hip.h, asd_fsm_*): `TokenFSM`, a token-level
deterministic automaton a caller writes down or gets from `TokenFSM.from_choices`, and `compile_rows`, which turns the
automata of one generate call and every row's stop ids into the ONE state space the device tables describe.  Nothing here
touches the device; kernels.pack_fsm uploads what compile_rows returns."""
from __future__ import annotations

from collections.abc import Mapping, Sequence
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

MAX_FSM_STATES = 1024                        # states of one generate call, every END state included
MAX_FSM_EDGES = 2 ** 20                      # edges of one generate call
MAX_CHOICES = 256                            # choices of one guided_choice list
MAX_CHOICE_LEN = 64                          # token ids of one choice


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _is_seq(v) -> bool:
    return isinstance(v, (Sequence, np.ndarray)) and not isinstance(v, (str, bytes))


class TokenFSM:
    """A deterministic automaton over token ids.  `edges[s]` is {token id: next state}, a next state of -1 meaning "this token
    is forbidden in s"; `other[s]` is the next state of every token without an edge in s, -1 (the default) meaning such tokens
    are forbidden; `accepting` holds the states in which a row may end (compile_rows gives them their stop edges).  Ids are
    checked against the vocabulary by `check_vocab`, which the stage calls: the automaton itself does not know it."""

    def __init__(self, n_states: int, start: int, edges, other=None, accepting=()):
        if not _is_int(n_states) or int(n_states) < 1:
            raise ValueError(f"a TokenFSM has at least one state, got n_states = {n_states!r}")
        n = self.n_states = int(n_states)

        def state(s, what, lowest=0):
            if not _is_int(s) or not lowest <= int(s) < n:
                raise ValueError(f"{what} must be an integer state in [{lowest}, {n}), got {s!r}")
            return int(s)
        self.start = state(start, "start")
        if isinstance(edges, Mapping):
            edges = [edges.get(s) for s in range(n)] if all(_is_int(s) and 0 <= int(s) < n for s in edges) else None
        if not _is_seq(edges) or len(edges) != n:
            raise ValueError(f"edges must hold one {{token id: next state}} dict per state ({n}); a state out of range is refused")
        self.edges: List[Dict[int, int]] = []
        for s, d in enumerate(edges):
            if d is not None and not isinstance(d, Mapping):
                raise ValueError(f"edges[{s}] must be a dict {{token id: next state}}, got {d!r}")
            row = {}
            for t, to in (d or {}).items():
                if not _is_int(t) or int(t) < 0:
                    raise ValueError(f"edges[{s}]: token ids must be integers >= 0, got {t!r}")
                row[int(t)] = state(to, f"edges[{s}][{t!r}]", -1)
            self.edges.append(row)
        if other is None:
            other = [-1] * n
        if not _is_seq(other) or len(other) != n:
            raise ValueError(f"other must hold one next state (or -1) per state ({n})")
        self.other = [state(o, f"other[{s}]", -1) for s, o in enumerate(other)]
        if isinstance(accepting, (str, bytes)) or not hasattr(accepting, "__iter__"):
            raise ValueError(f"accepting must be a collection of states, got {accepting!r}")
        self.accepting = frozenset(state(s, "an accepting state") for s in accepting)
        self.from_choice_list = False                    # from_choices: the error messages then speak of guided_choice
        self.key = (n, self.start, tuple(tuple(sorted(e.items())) for e in self.edges), tuple(self.other), tuple(sorted(self.accepting)))

    def __eq__(self, o):
        return isinstance(o, TokenFSM) and self.key == o.key

    def __hash__(self):
        return hash(self.key)

    def check_vocab(self, vocab: int) -> "TokenFSM":
        for s, e in enumerate(self.edges):
            if e and max(e) >= vocab:
                raise ValueError(f"edges[{s}]: token ids must lie in [0, {vocab}), got {max(e)}")
        return self

    @classmethod
    def from_choices(cls, choices, tokenizer=None, vocab: Optional[int] = None) -> "TokenFSM":
        """The trie of `choices`: a choice is a sequence of 1..64 token ids, or a str, which `tokenizer` encodes and `vocab`
        folds exactly as the stage folds a stop string (a stage passes its own; without them a str is refused).  Duplicates
        are dropped, at most 256 choices stay; a choice's end node is accepting -- an inner node too when one choice is a prefix
        of another."""
        if not _is_seq(choices):
            raise ValueError(f"guided choices must be a list of strings or token-id sequences, got {choices!r}")
        seqs = []
        for c in choices:
            if isinstance(c, str):
                if tokenizer is None or vocab is None:
                    raise ValueError(f"a str choice needs the stage's tokenizer: pass it to generate(guided_choice=...), got {c!r}")
                ids = [int(i) % int(vocab) for i in tokenizer.encode(c, return_tensors=None)]
            elif not _is_seq(c):
                raise ValueError(f"a guided choice is a string or a sequence of token ids, got {c!r}")
            else:
                if not all(_is_int(t) and int(t) >= 0 for t in c):
                    raise ValueError(f"a guided choice's token ids must be integers >= 0, got {c!r}")
                ids = [int(t) for t in c]
            if vocab is not None and any(t >= int(vocab) for t in ids):
                raise ValueError(f"a guided choice's token ids must lie in [0, {int(vocab)}), got {c!r}")
            if not 1 <= len(ids) <= MAX_CHOICE_LEN:
                raise ValueError(f"a guided choice must come to 1..{MAX_CHOICE_LEN} token ids, {c!r} gives {len(ids)}")
            seqs.append(tuple(ids))
        seqs = list(dict.fromkeys(seqs))
        if not seqs:
            raise ValueError("a guided choice list must hold at least one choice")
        if len(seqs) > MAX_CHOICES:
            raise ValueError(f"{len(seqs)} distinct guided choices, at most {MAX_CHOICES}")
        edges, accepting = [{}], set()
        for ids in seqs:
            s = 0
            for t in ids:
                if t not in edges[s]:
                    edges[s][t] = len(edges)
                    edges.append({})
                s = edges[s][t]
            accepting.add(s)
        fsm = cls(len(edges), 0, edges, None, accepting)
        fsm.from_choice_list = True
        return fsm


@dataclass
class CompiledFsm:
    """The automata of one generate call in one state space, as numpy arrays in the layout of include/asd_hip.h: state_first
    int32 [S + 1], edge_tok / edge_next int32 [E] (ids ascending within a state), state_other int32 [S]; starts: every row's
    global start state, -1 for a row without an automaton; row_states: every row's reachable states."""
    state_first: np.ndarray
    edge_tok: np.ndarray
    edge_next: np.ndarray
    state_other: np.ndarray
    starts: List[int]
    V: int

    @property
    def S(self) -> int:
        return int(self.state_other.shape[0])

    @property
    def E(self) -> int:
        return int(self.edge_tok.shape[0])

    def allowed(self, s: int) -> np.ndarray:
        """bool [V]: the tokens with a transition in state s that is not -1."""
        lo, hi = int(self.state_first[s]), int(self.state_first[s + 1])
        keep = np.full(self.V, bool(self.state_other[s] >= 0))
        keep[self.edge_tok[lo:hi]] = self.edge_next[lo:hi] >= 0
        return keep

    def step(self, s: int, t: int) -> int:
        """delta(s, t), by the header's table."""
        if not 0 <= s < self.S or not 0 <= t < self.V:
            return s
        lo, hi = int(self.state_first[s]), int(self.state_first[s + 1])
        i = lo + int(np.searchsorted(self.edge_tok[lo:hi], t))
        to = int(self.edge_next[i]) if i < hi and int(self.edge_tok[i]) == t else int(self.state_other[s])
        return to if 0 <= to < self.S else s


def _compile_one(fsm: TokenFSM, Z: Tuple[int, ...]):
    """One automaton under one stop set Z -> (edges per state, other per state) over fsm.n_states + 1 states, the last one END:
    END allows exactly Z and loops; an accepting state sends every z without an explicit edge to END; a non-accepting state
    forbids every z without an explicit edge, even under `other`."""
    end = fsm.n_states
    edges = []
    for s, e in enumerate(fsm.edges):
        e = dict(e)
        for z in Z:
            e.setdefault(z, end if s in fsm.accepting else -1)
        edges.append(e)
    edges.append({z: end for z in Z})
    return edges, list(fsm.other) + [-1]


def compile_rows(fsms: Sequence[Optional[TokenFSM]], stops: Sequence[Sequence[int]], vocab: int) -> CompiledFsm:
    """Every row's automaton (or None) and stop ids Z (its length-1 stop-list entries) -> one CompiledFsm.  Rows with the same
    automaton and the same Z share one compiled automaton; the limits are MAX_FSM_STATES states and MAX_FSM_EDGES edges per call."""
    first, toks, nexts, other, starts, base_of = [0], [], [], [], [], {}
    n_edges = 0
    for fsm, Z in zip(fsms, stops):
        if fsm is None:
            starts.append(-1)
            continue
        key = (fsm, tuple(sorted(set(int(z) for z in Z))))
        if key not in base_of:
            base = base_of[key] = len(other)
            edges, oth = _compile_one(fsm, key[1])
            n_edges += sum(len(e) for e in edges)
            if base + len(edges) > MAX_FSM_STATES or n_edges > MAX_FSM_EDGES:
                raise ValueError(f"the guided automata of one call hold at most {MAX_FSM_STATES} states (one END state per automaton "
                                 f"and stop set included) and {MAX_FSM_EDGES} edges")
            for e, o in zip(edges, oth):
                ids = np.fromiter(sorted(e), dtype=np.int32, count=len(e))
                to = np.fromiter((e[int(t)] for t in ids), dtype=np.int32, count=len(e))
                toks.append(ids)
                nexts.append(np.where(to >= 0, to + base, -1).astype(np.int32))
                other.append(o + base if o >= 0 else -1)
                first.append(first[-1] + len(e))
        starts.append(base_of[key] + fsm.start)
    cat = lambda parts: np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)     # noqa: E731
    return CompiledFsm(np.asarray(first, dtype=np.int32), cat(toks), cat(nexts), np.asarray(other, dtype=np.int32), starts, int(vocab))


def reachable(c: CompiledFsm, start: int) -> List[int]:
    seen, todo = {start}, [start]
    while todo:
        s = todo.pop()
        lo, hi = int(c.state_first[s]), int(c.state_first[s + 1])
        for to in set(c.edge_next[lo:hi].tolist()) | {int(c.state_other[s])}:
            if to >= 0 and to not in seen:
                seen.add(to)
                todo.append(to)
    return sorted(seen)


def check_guided_rows_keep_a_token(c: CompiledFsm, fsms, allowed, edit_rows, bad_rows) -> None:
    """THE ROW KEEPS A TOKEN, conservatively, because the state lives on the device: for every state reachable from a row's
    start, the state's allowed set, intersected with the row's allow-list, minus its permanent bans, minus the LAST ids of all
    its bad words, must be non-empty.  Covers a non-accepting dead end and an accepting leaf on a row without a stop id."""
    verdict = {}
    for b, (fsm, ids, entries, words) in enumerate(zip(fsms, allowed, edit_rows, bad_rows)):
        if fsm is None:
            continue
        gone = sorted({t for t, _, u in entries if u > 0} | {w[-1] for w in words})
        key = (c.starts[b], None if ids is None else tuple(ids), tuple(gone))
        if key not in verdict:
            verdict[key] = None
            for s in reachable(c, c.starts[b]):
                keep = c.allowed(s)
                if ids is not None:
                    only = np.zeros(c.V, dtype=bool)
                    only[list(ids)] = True
                    keep &= only
                keep[gone] = False
                if not keep.any():
                    verdict[key] = s - c.starts[b] + fsm.start
                    break
        if verdict[key] is not None:
            hint = " (guided_choice needs a stop id on the row: stop_token_ids or a one-token stop sequence ends a choice)" \
                if fsm.from_choice_list else ""
            raise ValueError(f"prompt {b}: state {verdict[key]} of its guided automaton keeps no token under the row's stop ids, "
                             f"allowed_token_ids, banned ids and the last ids of its bad_words{hint}")
