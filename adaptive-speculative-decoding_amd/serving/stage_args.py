"""The argument checks of Stage.generate (serving/stages.py, whose module docstring states every rule): host-side, before any
launch.  Every "one value, or one per prompt" argument goes through `_per_prompt`; a bad value raises ValueError."""
from __future__ import annotations

from collections.abc import Sequence          # (isinstance against this one, not typing's alias: several times cheaper)
from typing import Dict, List, Optional, Tuple

import numpy as np

from .guided import TokenFSM

MAX_STOP_IDS = 8                             # ASD_MAX_STOP_IDS of include/asd_hip.h
MAX_STOP_SEQS = 16                           # ASD_MAX_STOP_SEQS: entries of one row's list (stop ids included)
MAX_STOP_SEQ_LEN = 8                         # ASD_MAX_STOP_SEQ_LEN
MAX_TOP_LOGPROBS = 8                         # ASD_MAX_TOP_LOGPROBS
MAX_LOGIT_EDITS = 1024                       # ASD_MAX_LOGIT_EDITS: (id, bias, until) entries of one row after merging
MAX_BAD_WORDS = 256                          # ASD_MAX_BAD_WORDS: distinct words of one row (BAD WORDS)
MAX_BAD_WORD_LEN = 8                         # ASD_MAX_BAD_WORD_LEN
MAX_NGRAM = 8                                # ASD_MAX_NGRAM: the largest no_repeat_ngram_size (NO REPEAT N-GRAM)
MAX_LOGIT_BIAS = 100.0                      # |bias| <= 100, the range OpenAI documents
_EDIT_FOREVER = 2 ** 31 - 1                  # `until` of a permanent ban
_NUMBER = (int, float, np.integer, np.floating)


def _is_seq(v) -> bool:
    return isinstance(v, (Sequence, np.ndarray)) and not isinstance(v, (str, bytes))


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _per_prompt(value, n: int, one, what: str) -> list:
    """One value for all `n` prompts, or a sequence of n values, each passed through `one(v)` -> a list of n checked values."""
    if not _is_seq(value):
        return [one(value)] * n
    if len(value) != n:
        raise ValueError(f"{len(value)} {what} for {n} prompts")
    return [one(v) for v in value]


def _check_stop_ids(ids: Sequence[int], vocab: int) -> Tuple[int, ...]:
    ids = tuple(int(i) for i in ids)
    if len(ids) > MAX_STOP_IDS:
        raise ValueError(f"at most {MAX_STOP_IDS} stop token ids, got {len(ids)}")
    if len(set(ids)) != len(ids):
        raise ValueError("stop token ids must be distinct")
    if any(not 0 <= i < vocab for i in ids):
        raise ValueError(f"stop token ids must lie in [0, {vocab})")
    return ids


def check_max_tokens(max_tokens, n: int):
    """generate's `max_tokens`: an int (returned as it is), or a sequence of n ints >= 1 -> a list of n ints."""
    def one(v):
        if not _is_int(v) or int(v) < 1:
            raise ValueError(f"every per-prompt max_tokens must be an integer >= 1, got {max_tokens!r}")
        return int(v)
    if _is_int(max_tokens):
        return int(max_tokens)
    if not _is_seq(max_tokens):
        raise ValueError(f"max_tokens must be an integer or one integer per prompt, got {max_tokens!r}")
    return _per_prompt(max_tokens, n, one, "max_tokens values")


def _check_stop_sequences(entries, vocab: int, tokenizer) -> List[Tuple[int, ...]]:
    """One list of stop sequences: each entry a str (encoded by the stage's tokenizer, ids folded into the vocabulary as
    encode_prompts folds prompt ids) or a sequence of token ids; every entry must come to 1..8 ids in [0, vocab)."""
    if entries is None:
        return []
    if not _is_seq(entries):
        raise ValueError(f"stop sequences must be a list of strings or token-id sequences, got {entries!r}")
    out = []
    for e in entries:
        if isinstance(e, str):
            ids = [int(i) % vocab for i in tokenizer.encode(e, return_tensors=None)]
        elif not _is_seq(e):
            raise ValueError(f"a stop sequence is a string or a sequence of token ids, got {e!r}")
        else:
            if not all(_is_int(t) for t in e):
                raise ValueError(f"stop sequence token ids must be integers, got {e!r}")
            ids = [int(t) for t in e]
            if any(not 0 <= t < vocab for t in ids):
                raise ValueError(f"stop sequence token ids must lie in [0, {vocab})")
        if not 1 <= len(ids) <= MAX_STOP_SEQ_LEN:
            raise ValueError(f"a stop sequence must come to 1..{MAX_STOP_SEQ_LEN} token ids, {e!r} gives {len(ids)}")
        out.append(tuple(ids))
    return out


def _check_logprobs(n) -> int:
    if not _is_int(n) or not 0 <= int(n) <= MAX_TOP_LOGPROBS:
        raise ValueError(f"logprobs must be an integer in [0, {MAX_TOP_LOGPROBS}], got {n!r}")
    return int(n)


def _check_prompt_logprobs(n) -> Optional[int]:
    """None: off.  An int in [0, MAX_TOP_LOGPROBS]: on (0: the tokens' own log-prob and rank, no table)."""
    if n is None:
        return None
    if not _is_int(n) or not 0 <= int(n) <= MAX_TOP_LOGPROBS:
        raise ValueError(f"prompt_logprobs must be None or an integer in [0, {MAX_TOP_LOGPROBS}], got {n!r}")
    return int(n)


def _check_token_stats(v) -> Optional[bool]:
    """None stays None (the caller's default then holds); a bool is returned as given; anything else -- an int, a string, a
    sequence -- raises."""
    if v is None or isinstance(v, bool):
        return v
    raise ValueError(f"token_stats must be None or a bool, got {v!r}")


def _check_min_p(v, name: str = "min_p") -> float:
    if isinstance(v, bool) or not isinstance(v, _NUMBER) or not 0.0 <= float(v) <= 1.0:
        raise ValueError(f"{name} must be a number in [0, 1], got {v!r}")           # (NaN included)
    return float(v)


CUT_OFF, CUT_TYPICAL, CUT_EPSILON, CUT_ETA = 0, 1, 2, 3      # ASD_CUT_* of include/asd_hip.h: a row's mode (ENTROPY CUTS)


def check_entropy_cuts(typical_p, epsilon_cutoff, eta_cutoff, n: int) -> List[Tuple[int, float]]:
    """generate's `typical_p`, `epsilon_cutoff` and `eta_cutoff` (HF's warpers of those names): each one number for all `n`
    prompts or a sequence of n numbers -> every row's (mode, value).  typical_p lies in [0, 1], 0 and 1 are off; the other two
    lie in [0, 1), 0 is off.  A row has at most one mode.  A bool, a NaN, a value outside its range, the wrong length and a row
    with two modes ("not built") raise ValueError."""
    def number(name, top_closed):
        def one(v):
            ok = not isinstance(v, bool) and isinstance(v, _NUMBER) and (0.0 <= float(v) <= 1.0 if top_closed else 0.0 <= float(v) < 1.0)
            if not ok:                                                           # (NaN included)
                raise ValueError(f"{name} must be a number in [0, 1{']' if top_closed else ')'}, got {v!r}")
            v = float(np.float32(v))                                             # the value the device record holds
            return v if 0.0 < v < 1.0 else 0.0
        return one
    cols = []
    for name, value, closed in (("typical_p", typical_p, True), ("epsilon_cutoff", epsilon_cutoff, False),
                                ("eta_cutoff", eta_cutoff, False)):
        if isinstance(value, (str, bytes)):
            raise ValueError(f"{name} must be a number or one number per prompt, got {value!r}")
        cols.append(_per_prompt(value, n, number(name, closed), f"{name} values"))
    rows = []
    for b, values in enumerate(zip(*cols)):
        on = [(mode, v) for mode, v in zip((CUT_TYPICAL, CUT_EPSILON, CUT_ETA), values) if v > 0.0]
        if len(on) > 1:
            raise ValueError(f"prompt {b}: more than one of typical_p, epsilon_cutoff and eta_cutoff on one row is not built")
        rows.append(on[0] if on else (CUT_OFF, 0.0))
    return rows


def _check_sampling_value(v, name: str):
    """One temperature / top_p / top_k / min_p value of generate (PER-REQUEST SAMPLING)."""
    if name == "top_k":
        if not _is_int(v):
            raise ValueError(f"top_k must be an integer, got {v!r}")
        return int(v)
    if name == "min_p":
        return _check_min_p(v)
    if isinstance(v, bool) or not isinstance(v, _NUMBER) or float(v) != float(v):
        raise ValueError(f"{name} must be a number, got {v!r}")
    v = float(v)
    if name == "temperature" and not v >= 0.0:
        raise ValueError("temperature must be >= 0 (0: greedy decoding)")
    return v


def check_per_prompt(value, n: int, name: str):
    """generate's `temperature` / `top_p` / `top_k` / `min_p`: None (returned as it is), one value for all `n` prompts, or a
    sequence of n values.  -> the checked value, or a list of n checked values; a sequence whose values are all equal
    collapses to that value."""
    if value is None:
        return None
    if isinstance(value, (str, bytes)):
        raise ValueError(f"{name} must be a number or one number per prompt, got {value!r}")
    if not _is_seq(value):
        return _check_sampling_value(value, name)
    vals = _per_prompt(value, n, lambda v: _check_sampling_value(v, name), f"{name} values")   # (None inside a sequence raises)
    return vals[0] if vals and all(v == vals[0] for v in vals) else vals


def _check_token_id(t, vocab: int, what: str) -> int:
    if not _is_int(t) or not 0 <= int(t) < vocab:
        raise ValueError(f"{what} token ids must be integers in [0, {vocab}), got {t!r}")
    return int(t)


def check_logit_bias(value, n: int, vocab: int) -> List[Dict[int, float]]:
    """generate's `logit_bias`: None, one dict for all `n` prompts, or a sequence of n dicts / Nones -> n dicts."""
    def one(d):
        if d is None:
            return {}
        if not isinstance(d, dict):
            raise ValueError(f"logit_bias must be a dict {{token id: bias}} or one dict per prompt, got {d!r}")
        out = {}
        for t, b in d.items():
            t = _check_token_id(t, vocab, "logit_bias")
            if isinstance(b, bool) or not isinstance(b, _NUMBER) or not abs(float(b)) <= MAX_LOGIT_BIAS:      # (NaN included)
                raise ValueError(f"a logit bias must be a number in [-{MAX_LOGIT_BIAS:g}, {MAX_LOGIT_BIAS:g}], got {b!r}")
            out[t] = float(b)
        return out
    return _per_prompt(value, n, one, "logit_bias dicts")


def check_banned_token_ids(value, n: int, vocab: int) -> List[Tuple[int, ...]]:
    """generate's `banned_token_ids`: None, a sequence of ids for all `n` prompts, or a sequence of n such sequences -> n sorted
    tuples of distinct ids."""
    def one(ids):
        return tuple(sorted({_check_token_id(t, vocab, "banned") for t in (ids if ids is not None else ())}))
    if value is not None and not _is_seq(value):
        raise ValueError(f"banned_token_ids must be a sequence of token ids or one sequence per prompt, got {value!r}")
    per_prompt = [_is_seq(v) or v is None for v in (value if value is not None else ())]
    if not any(per_prompt):                              # a flat id list (or None): the same ban for every prompt
        return [one(value)] * n
    if not all(per_prompt):
        raise ValueError("banned_token_ids mixes token ids and per-prompt lists")
    return _per_prompt(list(value), n, one, "banned_token_ids lists")


def check_allowed_token_ids(value, n: int, vocab: int) -> List[Optional[Tuple[int, ...]]]:
    """generate's `allowed_token_ids`: None, a sequence of ids for all `n` prompts, or a sequence of n such sequences / Nones
    -> n sorted tuples of distinct ids, or None for a prompt without a list.  An EMPTY list raises: it allows nothing, and the
    samplers forbid a row without a finite logit."""
    def one(ids):
        if ids is None:
            return None
        out = tuple(sorted({_check_token_id(t, vocab, "allowed") for t in ids}))
        if not out:
            raise ValueError("an allowed_token_ids list must name at least one token (None: no list)")
        return out
    if value is None:
        return [None] * n
    if not _is_seq(value):
        raise ValueError(f"allowed_token_ids must be a sequence of token ids or one sequence per prompt, got {value!r}")
    per_prompt = [_is_seq(v) or v is None for v in value]
    if not any(per_prompt):                              # a flat id list: the same list for every prompt
        return [one(value)] * n
    if not all(per_prompt):
        raise ValueError("allowed_token_ids mixes token ids and per-prompt lists")
    return _per_prompt(list(value), n, one, "allowed_token_ids lists")


def check_rows_keep_a_token(allowed: List[Optional[Tuple[int, ...]]], edit_rows: List[List[Tuple[int, float, int]]],
                            bad_rows: Optional[List[List[Tuple[int, ...]]]] = None, vocab: Optional[int] = None) -> None:
    """A row's allow-list minus every merged edit entry with until > 0 -- the permanent bans AND the min_tokens bans, during
    whose hold-back the row would be all -inf -- must keep a token: ValueError naming the prompt otherwise.  With `bad_rows`
    (every row's bad words; BAD WORDS) the rule is conservative, because which word matches is decided on the device: the LAST id
    of every word of the row counts as banned, and a row without an allow-list must keep a token of the `vocab` ids."""
    bad_rows = [[] for _ in allowed] if bad_rows is None else bad_rows
    for b, (ids, entries, words) in enumerate(zip(allowed, edit_rows, bad_rows)):
        gone = {t for t, _, u in entries if u > 0} | {w[-1] for w in words}
        if ids is not None and not set(ids) - gone:
            raise ValueError(f"prompt {b}: the banned token ids (min_tokens' stop ids and the last ids of its bad_words "
                             f"included) leave no token of its allowed_token_ids ({len(ids)})")
        if ids is None and words and len(gone) >= vocab:
            raise ValueError(f"prompt {b}: the banned token ids and the last ids of its bad_words leave no token of the "
                             f"vocabulary ({vocab})")


def check_no_repeat_ngram_size(value, n: int) -> List[int]:
    """generate's `no_repeat_ngram_size` (HF generate's): an int in [0, MAX_NGRAM] for all `n` prompts (0: off), or a sequence
    of n such ints -> n ints.  A bool, a float, None inside a sequence, the wrong length and a value outside the range raise
    ValueError."""
    def one(v):
        if not _is_int(v) or not 0 <= int(v) <= MAX_NGRAM:
            raise ValueError(f"no_repeat_ngram_size must be an integer in [0, {MAX_NGRAM}], got {v!r}")
        return int(v)
    if isinstance(value, (str, bytes)):
        raise ValueError(f"no_repeat_ngram_size must be an integer or one integer per prompt, got {value!r}")
    return _per_prompt(value, n, one, "no_repeat_ngram_size values")


def check_ngram_rows_keep_a_token(ngram_rows: List[int], prompt_lens: List[int], limits, draft_len: int,
                                  allowed: List[Optional[Tuple[int, ...]]], edit_rows: List[List[Tuple[int, float, int]]],
                                  bad_rows: List[List[Tuple[int, ...]]], vocab: int) -> None:
    """THE ROW KEEPS A TOKEN under no_repeat_ngram_size (NO REPEAT N-GRAM).  A position bans at most one token per n-gram that
    starts in its history, so at most len(H) of them, and no position of row b sees a history longer than
        bound_b = prompt_lens[b] + limits[b] + draft_len
    (its real prompt ids, its max_tokens, one step's proposals).  With gone_b the set check_rows_keep_a_token counts -- the
    permanent bans, the stop ids under min_tokens, the last ids of the row's bad words -- a row with n > 0 and without an
    allow-list needs |gone_b| + bound_b < vocab, one with an allow-list |allowed_b - gone_b| > bound_b: ValueError naming the
    prompt otherwise.  Rows with n == 0 are not looked at."""
    for b, n in enumerate(ngram_rows):
        if n <= 0:
            continue
        bound = int(prompt_lens[b]) + int(limits[b]) + int(draft_len)
        gone = {t for t, _, u in edit_rows[b] if u > 0} | {w[-1] for w in bad_rows[b]}
        if allowed[b] is None and len(gone) + bound >= vocab:
            raise ValueError(f"prompt {b}: no_repeat_ngram_size can ban up to {bound} tokens (prompt {int(prompt_lens[b])} + "
                             f"max_tokens {int(limits[b])} + draft_len {int(draft_len)}), which with its {len(gone)} banned ids "
                             f"may leave no token of the vocabulary ({vocab})")
        if allowed[b] is not None and len(set(allowed[b]) - gone) <= bound:
            raise ValueError(f"prompt {b}: no_repeat_ngram_size can ban up to {bound} tokens (prompt {int(prompt_lens[b])} + "
                             f"max_tokens {int(limits[b])} + draft_len {int(draft_len)}), which may leave no token of its "
                             f"allowed_token_ids ({len(set(allowed[b]) - gone)} after its bans)")


def _check_bad_word_list(entries, vocab: int, tokenizer, what: str) -> List[Tuple[int, ...]]:
    """One list of bad words: each entry a str (encoded by the stage's tokenizer, ids folded into the vocabulary exactly as
    _check_stop_sequences folds a stop string) or a sequence of integer ids in [0, vocab); every entry must come to 1..8 ids."""
    if entries is None:
        return []
    if not _is_seq(entries):
        raise ValueError(f"{what} must be a list of strings or token-id sequences, got {entries!r}")
    out = []
    for e in entries:
        if isinstance(e, str):
            ids = [int(i) % vocab for i in tokenizer.encode(e, return_tensors=None)]
        elif not _is_seq(e):
            raise ValueError(f"an entry of {what} is a string or a sequence of token ids, got {e!r}")
        else:
            ids = [_check_token_id(t, vocab, "bad_words") for t in e]
        if not 1 <= len(ids) <= MAX_BAD_WORD_LEN:
            raise ValueError(f"an entry of {what} must come to 1..{MAX_BAD_WORD_LEN} token ids, {e!r} gives {len(ids)}")
        out.append(tuple(ids))
    return out


def check_bad_words(common, per_prompt, n: int, vocab: int, tokenizer) -> List[List[Tuple[int, ...]]]:
    """generate's `bad_words` (one list for every prompt, or None) and `bad_words_per_prompt` (n lists, or None) -> every row's
    words as tuples of ids: the common list followed by the row's own, duplicates dropped (the first occurrence stays), at
    most MAX_BAD_WORDS afterwards."""
    shared = _check_bad_word_list(common, vocab, tokenizer, "bad_words")
    own = [[] for _ in range(n)]
    if per_prompt is not None:
        if not _is_seq(per_prompt) or len(per_prompt) != n:
            raise ValueError(f"bad_words_per_prompt must hold one list per prompt ({n})")
        own = [_check_bad_word_list(e, vocab, tokenizer, "bad_words_per_prompt") for e in per_prompt]
    rows = []
    for b, o in enumerate(own):
        row = list(dict.fromkeys(shared + o))
        if len(row) > MAX_BAD_WORDS:
            raise ValueError(f"prompt {b}: {len(row)} distinct bad_words, at most {MAX_BAD_WORDS}")
        rows.append(row)
    return rows


def check_guided(guided_fsm, guided_choice, guided_choice_per_prompt, n: int, vocab: int, tokenizer) -> List[Optional[TokenFSM]]:
    """generate's `guided_fsm` (one TokenFSM for every prompt, or n entries, each a TokenFSM or None), `guided_choice` (one
    list of choices for every prompt) and `guided_choice_per_prompt` (n lists; None or an empty list: the row is unguided)
    -> every row's automaton, checked against the vocabulary, or None.  A row with both an automaton and choices raises."""
    rows: List[Optional[TokenFSM]] = [None] * n
    if guided_fsm is not None:
        if isinstance(guided_fsm, TokenFSM):
            rows = [guided_fsm.check_vocab(vocab)] * n
        elif not _is_seq(guided_fsm) or len(guided_fsm) != n or any(f is not None and not isinstance(f, TokenFSM) for f in guided_fsm):
            raise ValueError(f"guided_fsm must be a TokenFSM or one TokenFSM (or None) per prompt ({n}), got {guided_fsm!r}")
        else:
            rows = [None if f is None else f.check_vocab(vocab) for f in guided_fsm]

    def choices(value, what):
        if not _is_seq(value):
            raise ValueError(f"{what} must be a list of strings or token-id sequences, got {value!r}")
        return TokenFSM.from_choices(value, tokenizer, vocab)
    own: List[Optional[TokenFSM]] = [None] * n
    if guided_choice is not None:
        own = [choices(guided_choice, "guided_choice")] * n
    if guided_choice_per_prompt is not None:
        if not _is_seq(guided_choice_per_prompt) or len(guided_choice_per_prompt) != n:
            raise ValueError(f"guided_choice_per_prompt must hold one list per prompt ({n})")
        for b, e in enumerate(guided_choice_per_prompt):
            if e is None or (_is_seq(e) and len(e) == 0):
                continue
            if own[b] is not None:
                raise ValueError(f"prompt {b}: guided_choice and guided_choice_per_prompt both name choices")
            own[b] = choices(e, "an entry of guided_choice_per_prompt")
    for b, (f, c) in enumerate(zip(rows, own)):
        if f is not None and c is not None:
            raise ValueError(f"prompt {b}: a row takes a guided_fsm or guided choices, not both")
    return [f if f is not None else c for f, c in zip(rows, own)]


def check_min_tokens(value, n: int) -> List[int]:
    """generate's `min_tokens`: an int >= 0 for all `n` prompts, or a sequence of n such ints -> n ints."""
    def one(v):
        if not _is_int(v) or int(v) < 0:
            raise ValueError(f"min_tokens must be an integer >= 0, got {v!r}")
        return min(int(v), _EDIT_FOREVER - 1)
    return _per_prompt(value, n, one, "min_tokens values")


def _check_penalty(value, n: int, name: str, lo: float, hi: float, open_lo: bool) -> List[float]:
    """One penalty keyword of generate (PENALTIES): a number in the range for all `n` prompts, or a sequence of n such numbers
    -> n floats.  A bool, a NaN, anything that is no number (None inside a sequence included) and a value outside the range
    raise ValueError."""
    def one(v):
        ok = not isinstance(v, bool) and isinstance(v, _NUMBER) and (lo < float(v) if open_lo else lo <= float(v)) and float(v) <= hi
        if not ok:                                        # (NaN fails both comparisons)
            raise ValueError(f"{name} must be a number in {'(' if open_lo else '['}{lo:g}, {hi:g}], got {v!r}")
        return float(v)
    if isinstance(value, (str, bytes)):
        raise ValueError(f"{name} must be a number or one number per prompt, got {value!r}")
    return _per_prompt(value, n, one, f"{name} values")


def check_repetition_penalty(value, n: int) -> List[float]:
    """generate's `repetition_penalty` (vLLM's range): a number in (0, 2], or one per prompt -> n floats; 1 is neutral."""
    return _check_penalty(value, n, "repetition_penalty", 0.0, 2.0, True)


def check_presence_penalty(value, n: int) -> List[float]:
    """generate's `presence_penalty` (OpenAI's / vLLM's range): a number in [-2, 2], or one per prompt -> n floats; 0 is neutral."""
    return _check_penalty(value, n, "presence_penalty", -2.0, 2.0, False)


def check_frequency_penalty(value, n: int) -> List[float]:
    """generate's `frequency_penalty` (OpenAI's / vLLM's range): a number in [-2, 2], or one per prompt -> n floats; 0 is neutral."""
    return _check_penalty(value, n, "frequency_penalty", -2.0, 2.0, False)


def check_seeds(seed, n: int) -> Optional[List[int]]:
    """generate's `seed`: None, one int in [0, 2^64) for all `n` prompts, or a sequence of n such ints -> None or n ints."""
    def one(v):
        if not _is_int(v) or not 0 <= int(v) < 2 ** 64:
            raise ValueError(f"seed must be an integer in [0, 2^64), got {v!r}")
        return int(v)
    return None if seed is None else _per_prompt(seed, n, one, "seeds")


def merge_logit_edits(bias: List[Dict[int, float]], banned: List[Tuple[int, ...]], min_tokens: List[int],
                      row_seqs: List[List[Tuple[int, ...]]], vocab: int) -> List[List[Tuple[int, float, int]]]:
    """Per row, the distinct (id, bias, until) entries of asd_logit_edit_rows (LOGIT EDITS), sorted by id: a bias has until 0, a
    length-1 stop entry of a row with min_tokens > 0 has until = min_tokens (and keeps its bias), a banned id has
    until = INT32_MAX.  An entry that would do nothing (bias 0, until 0) is dropped."""
    rows = []
    for b, (d, ban, m, seqs) in enumerate(zip(bias, banned, min_tokens, row_seqs)):
        entries = {t: [v, 0] for t, v in d.items()}
        if m > 0:
            if any(len(s) > 1 for s in seqs):
                raise ValueError(f"prompt {b}: min_tokens > 0 is not built for a stop list that holds a multi-token stop sequence")
            for (t,) in seqs:
                entries.setdefault(t, [0.0, 0])[1] = m
        for t in ban:
            entries[t] = [0.0, _EDIT_FOREVER]
        row = [(t, v, u) for t, (v, u) in sorted(entries.items()) if v != 0.0 or u > 0]
        if len(row) > MAX_LOGIT_EDITS:
            raise ValueError(f"prompt {b}: {len(row)} logit edits after merging, at most {MAX_LOGIT_EDITS}")
        if sum(u > 0 for _, _, u in row) >= vocab:
            raise ValueError(f"prompt {b}: the banned token ids leave no token of the vocabulary ({vocab})")
        rows.append(row)
    return rows
