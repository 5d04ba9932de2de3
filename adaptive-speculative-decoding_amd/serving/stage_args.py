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
MAX_LOOKUP_TOKENS, MAX_LOOKUP_NGRAM = 16, 8  # ASD_MAX_LOOKUP_TOKENS, ASD_MAX_LOOKUP_NGRAM: prompt_lookup_num_tokens / _max_ngram (PROMPT LOOKUP)
MAX_GUIDANCE_SCALE = 100.0                   # ASD_MAX_GUIDANCE_SCALE: the largest guidance_scale (GUIDANCE)
DRY_MAX_MATCH = 64                           # ASD_DRY_MAX_MATCH: the longest match DRY measures, and the largest dry_allowed_length (DRY)
MAX_DRY_BREAKERS = 32                        # ASD_MAX_DRY_BREAKERS: distinct sequence-breaker ids of a call
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


def check_mirostat(tau, eta, n: int, eta_given: bool = False) -> List[Tuple[float, float]]:
    """generate's `mirostat_tau` and `mirostat_eta` (llama.cpp's mirostat_v2): each one number for all `n` prompts or a sequence
    of n numbers -> every row's (tau, eta), (0.0, 0.0) where the row is off.  tau lies in [0, 32] and is off at 0; eta lies in
    (0, 1].  eta_given: the call named an eta of its own, which needs a row that is on.  A bool, a NaN, a value outside its
    range, the wrong length and eta without tau raise ValueError."""
    def number(name, lo_open, hi):
        def one(v):
            ok = not isinstance(v, bool) and isinstance(v, _NUMBER) and (0.0 < float(v) if lo_open else 0.0 <= float(v)) and float(v) <= hi
            if not ok:                                                           # (NaN included)
                raise ValueError(f"{name} must be a number in {'(' if lo_open else '['}0, {hi:g}], got {v!r}")
            return float(np.float32(v))                                          # the value the device record holds
        return one
    for name, value in (("mirostat_tau", tau), ("mirostat_eta", eta)):
        if isinstance(value, (str, bytes)):
            raise ValueError(f"{name} must be a number or one number per prompt, got {value!r}")
    taus = _per_prompt(tau, n, number("mirostat_tau", False, 32.0), "mirostat_tau values")
    etas = _per_prompt(eta, n, number("mirostat_eta", True, 1.0), "mirostat_eta values")
    if eta_given and not any(t > 0.0 for t in taus):
        raise ValueError("mirostat_eta without mirostat_tau: no row of the call has Mirostat on")
    return [(t, e) if t > 0.0 else (0.0, 0.0) for t, e in zip(taus, etas)]


def check_mirostat_alone(miro_rows, top_k, top_p, min_p, cut_rows, rel_rows=None) -> None:
    """A row with Mirostat on runs it IN PLACE of the truncation chain (llama.cpp): top-k, top-p, min-p, typical-p, epsilon or
    eta on the same row and side raise ValueError.  top_k / top_p / min_p: one value or a list per row; cut_rows: every row's
    (mode, value) of the entropy cut; rel_rows: every row's (mode, a, b) of the relative cut, which Mirostat excludes too."""
    n = len(miro_rows)
    cols = [v if isinstance(v, list) else [v] * n for v in (top_k, top_p, min_p)]
    for b, ((tau, _), k, p, m, (mode, _)) in enumerate(zip(miro_rows, *cols, cut_rows)):
        if tau > 0.0 and (int(k) > 0 or 0.0 < float(p) < 1.0 or float(m) > 0.0 or mode != CUT_OFF):
            raise ValueError(f"prompt {b}: Mirostat replaces top-k, top-p, min-p, typical-p, epsilon_cutoff and eta_cutoff; "
                             "a row cannot have both")
        if tau > 0.0 and rel_rows is not None and rel_rows[b][0] != RELCUT_OFF:
            raise ValueError(f"prompt {b}: top_n_sigma, top_a or XTC together with Mirostat on one row is not built")


RELCUT_OFF, RELCUT_TOP_N_SIGMA, RELCUT_TOP_A, RELCUT_XTC = 0, 1, 2, 3    # ASD_RELCUT_* of include/asd_hip.h (RELATIVE CUTS)
XTC_THRESHOLD_MAX = 0.5                  # above it A = {p >= t} holds two tokens only through an exact tie: the row is off


def check_relative_cuts(top_n_sigma, top_a, xtc_threshold, xtc_probability, n: int,
                        xtc_probability_given: bool = False) -> List[Tuple[int, float, float]]:
    """generate's `top_n_sigma`, `top_a`, `xtc_threshold` and `xtc_probability` (llama.cpp's and koboldcpp's samplers of those
    names): each one number for all `n` prompts or a sequence of n numbers -> every row's (mode, a, b).  top_n_sigma is a
    finite number >= 0 (0: off); top_a and xtc_probability lie in [0, 1] (0: off); xtc_threshold lies in [0, 1] (None: 0.1),
    and a row whose threshold is 0 or above 0.5 has XTC off.  xtc_probability_given: the call named a probability of its own,
    which needs a row with a usable threshold.  A row has at most one mode.  A bool, a NaN, a value outside its range, the
    wrong length and a row with two modes ("not built") raise ValueError."""
    def number(name, hi):
        def one(v):
            ok = not isinstance(v, bool) and isinstance(v, _NUMBER) and 0.0 <= float(v) <= hi and float(v) < float("inf")
            if not ok:                                                           # (NaN included)
                raise ValueError(f"{name} must be a number in [0, {'1]' if hi == 1.0 else 'inf)'}, got {v!r}")
            return float(np.float32(v))                                          # the value the device record holds
        return one
    named = (("top_n_sigma", top_n_sigma, float("inf")), ("top_a", top_a, 1.0),
             ("xtc_threshold", 0.1 if xtc_threshold is None else xtc_threshold, 1.0), ("xtc_probability", xtc_probability, 1.0))
    cols = []
    for name, value, hi in named:
        if isinstance(value, (str, bytes)):
            raise ValueError(f"{name} must be a number or one number per prompt, got {value!r}")
        cols.append(_per_prompt(value, n, number(name, hi), f"{name} values"))
    usable = [0.0 < t <= XTC_THRESHOLD_MAX for t in cols[2]]
    if xtc_probability_given and any(q > 0.0 for q in cols[3]) and not any(u and q > 0.0 for u, q in zip(usable, cols[3])):
        raise ValueError("xtc_probability without a usable xtc_threshold (in (0, 0.5]): no row of the call has XTC on")
    rows = []
    for b, (sig, a, t, q) in enumerate(zip(*cols)):
        on = [(RELCUT_TOP_N_SIGMA, sig, 0.0)] * (sig > 0.0) + [(RELCUT_TOP_A, a, 0.0)] * (a > 0.0) + \
            [(RELCUT_XTC, t, q)] * (q > 0.0 and usable[b])
        if len(on) > 1:
            raise ValueError(f"prompt {b}: more than one of top_n_sigma, top_a and XTC on one row is not built")
        rows.append(on[0] if on else (RELCUT_OFF, 0.0, 0.0))
    return rows


def check_relative_cut_alone(rel_rows, cut_rows) -> None:
    """A row takes ONE cut: a relative cut together with typical_p, epsilon_cutoff or eta_cutoff on the same row and side is
    not built and raises ValueError.  rel_rows: every row's (mode, a, b); cut_rows: every row's (mode, value)."""
    for b, ((rel, _, _), (cut, _)) in enumerate(zip(rel_rows, cut_rows)):
        if rel != RELCUT_OFF and cut != CUT_OFF:
            raise ValueError(f"prompt {b}: top_n_sigma, top_a or XTC together with typical_p, epsilon_cutoff or eta_cutoff "
                             "on one row is not built")


def check_tail_free(tfs, n: int) -> List[float]:
    """generate's `tfs` (tail-free sampling: webui's / koboldcpp's / Aphrodite's `tfs`, llama.cpp's old `tfs_z`): one number
    for all `n` prompts or a sequence of n numbers, each in (0, 1] (1: off) -> every row's value as the device record holds
    it.  A bool, a NaN, 0, a value outside (0, 1] and the wrong length raise ValueError."""
    def one(v):
        ok = not isinstance(v, bool) and isinstance(v, _NUMBER) and 0.0 < float(np.float32(v)) <= 1.0   # (NaN included)
        if not ok:
            raise ValueError(f"tfs must be a number in (0, 1] (1: off), got {v!r}")
        return float(np.float32(v))
    if isinstance(tfs, (str, bytes)):
        raise ValueError(f"tfs must be a number or one number per prompt, got {tfs!r}")
    return _per_prompt(tfs, n, one, "tfs values")


def check_tail_free_alone(tfs_rows, rel_rows, cut_rows, miro_rows=None, side: str = "") -> None:
    """A row takes ONE cut: tfs below 1 together with a relative cut, an entropy cut or Mirostat on the same row and side is
    not built and raises ValueError.  tfs_rows: every row's z; rel_rows: (mode, a, b); cut_rows: (mode, value); miro_rows:
    (tau, eta)."""
    for b, z in enumerate(tfs_rows):
        if z >= 1.0:
            continue
        if (rel_rows and rel_rows[b][0] != RELCUT_OFF) or (cut_rows and cut_rows[b][0] != CUT_OFF):
            raise ValueError(f"prompt {b}: {side}tfs together with top_n_sigma, top_a, XTC, typical_p, epsilon_cutoff or "
                             "eta_cutoff on one row is not built")
        if miro_rows is not None and miro_rows[b][0] > 0.0:
            raise ValueError(f"prompt {b}: tfs together with Mirostat on one row is not built")


TYPICAL_ACCEPT_THRESHOLD, TYPICAL_ACCEPT_ALPHA = 0.09, 0.3     # Medusa's posterior_threshold / posterior_alpha defaults
TYPICAL_ACCEPT_MAX_K = 16                                      # ASD_TYPICAL_ACCEPT_MAX_K of include/asd_hip.h


def check_typical_accept(threshold, alpha, n: int) -> Optional[List[Tuple[float, float]]]:
    """generate's `typical_acceptance_threshold` (eps, in (0, 1]) and `typical_acceptance_alpha` (in (0, 100]): each None (off),
    one number for all `n` prompts or a sequence of n entries -> every row's (eps, alpha), or None when every row is off.  A row
    is on when either of its two values is given; the one that is missing takes Medusa's default (0.09 / 0.3).  A bool, a NaN,
    a value outside its range, the wrong length, and a list that mixes rows that are on with rows that are off ("not built")
    raise ValueError."""
    def number(name, hi):
        def one(v):
            if v is None:
                return None
            ok = not isinstance(v, bool) and isinstance(v, _NUMBER) and 0.0 < float(v) <= hi      # (NaN included)
            if not ok:
                raise ValueError(f"{name} must be a number in (0, {hi:g}] or None (off), got {v!r}")
            return float(v)
        return one
    for name, value in (("typical_acceptance_threshold", threshold), ("typical_acceptance_alpha", alpha)):
        if isinstance(value, (str, bytes)):
            raise ValueError(f"{name} must be a number or one number per prompt, got {value!r}")
    eps = _per_prompt(threshold, n, number("typical_acceptance_threshold", 1.0), "typical_acceptance_threshold values")
    alphas = _per_prompt(alpha, n, number("typical_acceptance_alpha", 100.0), "typical_acceptance_alpha values")
    on = [e is not None or a is not None for e, a in zip(eps, alphas)]
    if not any(on):
        return None
    if not all(on):
        raise ValueError("typical acceptance on some prompts and the lossless rule on others in one call is not built: "
                         f"prompt {on.index(False)} has neither typical_acceptance_threshold nor typical_acceptance_alpha")
    return [(TYPICAL_ACCEPT_THRESHOLD if e is None else e, TYPICAL_ACCEPT_ALPHA if a is None else a) for e, a in zip(eps, alphas)]


def check_typical_accept_alone(rows, top_k, top_p, min_p, miro_rows, draft_len: int) -> None:
    """Typical acceptance reads the target's whole processed row: target-side top-k, top-p or min-p, or Mirostat, on a row of
    the call is not built and raises ValueError, as does a step of more than 16 proposals.  rows: check_typical_accept's (not
    None); top_k / top_p / min_p: one value or a list per row; miro_rows: every row's (tau, eta)."""
    n = len(rows)
    if draft_len > TYPICAL_ACCEPT_MAX_K:
        raise ValueError(f"typical acceptance verifies at most {TYPICAL_ACCEPT_MAX_K} proposals per step, got {draft_len}")
    cols = [v if isinstance(v, list) else [v] * n for v in (top_k, top_p, min_p)]
    for b, (k, p, m) in enumerate(zip(*cols)):
        if int(k) > 0 or 0.0 < float(p) < 1.0 or float(m) > 0.0:
            raise ValueError(f"prompt {b}: typical acceptance together with target-side top-k, top-p or min-p on one row is not built")
        if miro_rows and miro_rows[b][0] > 0.0:
            raise ValueError(f"prompt {b}: typical acceptance together with Mirostat on one row is not built")


SHAPE_OFF, SHAPE_DYNATEMP, SHAPE_QUADRATIC = 0, 1, 2     # ASD_SHAPE_* of include/asd_hip.h (SHAPING)


def check_logit_shapes(dynatemp_range, dynatemp_exponent, smoothing_factor, smoothing_curve, n: int,
                       exponent_given: bool = False, curve_given: bool = False) -> List[Tuple[int, float, float]]:
    """generate's `dynatemp_range`, `dynatemp_exponent`, `smoothing_factor` and `smoothing_curve` (llama.cpp's / koboldcpp's
    dynamic temperature; text-generation-webui's / koboldcpp's / Aphrodite's quadratic sampling): each one number for all `n`
    prompts or a sequence of n numbers -> every row's (mode, a, b), the values the f32 numbers the device record holds.
    dynatemp_range and smoothing_factor are finite numbers >= 0 (0: off); dynatemp_exponent is a finite number > 0;
    smoothing_curve lies in [1, 3].  exponent_given / curve_given: the call named the value itself, which needs a row that
    uses it (the mirostat_eta rule).  A row has at most one mode.  A bool, a NaN, a value outside its range, the wrong
    length and a row with both modes ("not built") raise ValueError."""
    inf = float("inf")

    def number(name, ok, text):
        def one(v):
            if isinstance(v, bool) or not isinstance(v, _NUMBER) or not ok(float(np.float32(v))):     # (NaN included)
                raise ValueError(f"{name} must be {text}, got {v!r}")
            return float(np.float32(v))
        return one
    named = (("dynatemp_range", dynatemp_range, lambda v: 0.0 <= v < inf, "a finite number >= 0"),
             ("dynatemp_exponent", dynatemp_exponent, lambda v: 0.0 < v < inf, "a finite number > 0"),
             ("smoothing_factor", smoothing_factor, lambda v: 0.0 <= v < inf, "a finite number >= 0"),
             ("smoothing_curve", smoothing_curve, lambda v: 1.0 <= v <= 3.0, "a number in [1, 3]"))
    cols = []
    for name, value, ok, text in named:
        if isinstance(value, (str, bytes)):
            raise ValueError(f"{name} must be a number or one number per prompt, got {value!r}")
        cols.append(_per_prompt(value, n, number(name, ok, text), f"{name} values"))
    if exponent_given and not any(r > 0.0 for r in cols[0]):
        raise ValueError("dynatemp_exponent without a dynatemp_range > 0: no row of the call has dynamic temperature on")
    if curve_given and not any(f > 0.0 for f in cols[2]):
        raise ValueError("smoothing_curve without a smoothing_factor > 0: no row of the call has quadratic sampling on")
    rows = []
    for b, (r, e, f, c) in enumerate(zip(*cols)):
        if r > 0.0 and f > 0.0:
            raise ValueError(f"prompt {b}: dynamic temperature and quadratic sampling on one row is not built")
        rows.append((SHAPE_DYNATEMP, r, e) if r > 0.0 else (SHAPE_QUADRATIC, f, c) if f > 0.0 else (SHAPE_OFF, 0.0, 0.0))
    return rows


def check_logit_shape_alone(shape_rows, miro_rows=None, temps=None, side: str = "") -> None:
    """What a shaped row excludes: Mirostat on the same row (its carried mu is defined on the distribution it cut) is not built;
    a dynatemp_range must lie strictly below the row's temperature (temps: every row's, None: a greedy call, which ignores the
    values), so that T_dyn > 0 -- a range that reaches temperature 0 is not built.  ValueError for either."""
    for b, (mode, a, _) in enumerate(shape_rows):
        if mode != SHAPE_OFF and miro_rows is not None and miro_rows[b][0] > 0.0:
            raise ValueError(f"prompt {b}: dynamic temperature or quadratic sampling together with Mirostat on one row is not built")
        if mode == SHAPE_DYNATEMP and temps is not None and not a < float(np.float32(temps[b])):
            raise ValueError(f"prompt {b}: {side}dynatemp_range {a} must lie strictly below the row's temperature {temps[b]}: "
                             "a range that reaches temperature 0 is not built")


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


def check_dry(multiplier, base, allowed_length, dry_range, breakers, n: int, vocab: int, tokenizer):
    """generate's `dry_multiplier` (a finite number >= 0; 0: off), `dry_base` (a finite number >= 1), `dry_allowed_length` (an
    int in [1, DRY_MAX_MATCH]) and `dry_range` (an int >= 0; 0: the whole history), each one value for all `n` prompts or a
    sequence of n values, and `dry_sequence_breakers`: ONE list for the call (or None), each entry a token id in [0, vocab) or
    a string that the stage's tokenizer encodes (ids folded as a stop string's are) to exactly ONE id -> (n multipliers, n
    bases, n allowed lengths, n ranges, the tuple of at most MAX_DRY_BREAKERS distinct breaker ids).  A bool, a NaN, a value
    outside its range, the wrong length, more than MAX_DRY_BREAKERS ids and a string of 0 or several ids raise ValueError."""
    def number(name, lo):
        def one(v):
            if isinstance(v, bool) or not isinstance(v, _NUMBER) or not lo <= float(v) < float("inf"):     # (NaN included)
                raise ValueError(f"{name} must be a finite number >= {lo:g}, got {v!r}")
            return float(v)
        return one

    def integer(name, lo, hi):
        def one(v):
            if not _is_int(v) or not lo <= int(v) <= hi:
                raise ValueError(f"{name} must be an integer in [{lo}, {hi}], got {v!r}")
            return int(v)
        return one
    cols = []
    for name, value, one in (("dry_multiplier", multiplier, number("dry_multiplier", 0.0)), ("dry_base", base, number("dry_base", 1.0)),
                             ("dry_allowed_length", allowed_length, integer("dry_allowed_length", 1, DRY_MAX_MATCH)),
                             ("dry_range", dry_range, integer("dry_range", 0, 2 ** 31 - 1))):
        if isinstance(value, (str, bytes)):
            raise ValueError(f"{name} must be one value or one per prompt, got {value!r}")
        cols.append(_per_prompt(value, n, one, f"{name} values"))
    ids = []
    if breakers is not None:
        if not _is_seq(breakers):
            raise ValueError(f"dry_sequence_breakers must be a list of token ids or strings, got {breakers!r}")
        for e in breakers:
            if isinstance(e, str):
                got = [int(i) % vocab for i in tokenizer.encode(e, return_tensors=None)]
                if len(got) != 1:
                    raise ValueError(f"a dry_sequence_breakers string must come to exactly one token id, {e!r} gives {len(got)} "
                                     "(multi-token breakers are not built)")
                ids.append(got[0])
            else:
                ids.append(_check_token_id(e, vocab, "dry_sequence_breakers"))
    ids = tuple(dict.fromkeys(ids))
    if len(ids) > MAX_DRY_BREAKERS:
        raise ValueError(f"{len(ids)} distinct dry_sequence_breakers, at most {MAX_DRY_BREAKERS}")
    return (*cols, ids)


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


def check_watermark(key, delta, gamma, context, n: int, named: bool = False):
    """generate's `watermark_key` (None: off; an int in [0, 2^64); or a sequence of n entries, each an int or None = that row
    off), `watermark_delta` (a finite number in (0, 100], raw logit units: logit_bias' range), `watermark_gamma` (in (0, 1)) and
    `watermark_context` (1, 2 or 3), each one value for all `n` prompts or a sequence of n values -> (n keys, n deltas, n
    gammas, n context widths).  `named`: the call itself names a delta, gamma or context; without a key on any row that is an
    error, as are a bool, a NaN, a value outside its range and the wrong length: ValueError."""
    def one_key(v):
        if v is not None and (not _is_int(v) or not 0 <= int(v) < 2 ** 64):
            raise ValueError(f"watermark_key must be None or an integer in [0, 2^64), got {v!r}")
        return None if v is None else int(v)

    def one_delta(v):
        if isinstance(v, bool) or not isinstance(v, _NUMBER) or not 0.0 < float(v) <= MAX_LOGIT_BIAS:      # (NaN included)
            raise ValueError(f"watermark_delta must be a number in (0, {MAX_LOGIT_BIAS:g}], got {v!r}")
        return float(v)

    def one_gamma(v):
        if isinstance(v, bool) or not isinstance(v, _NUMBER) or not 0.0 < float(v) < 1.0:
            raise ValueError(f"watermark_gamma must be a number in (0, 1), got {v!r}")
        return float(v)

    def one_context(v):
        if not _is_int(v) or not 1 <= int(v) <= 3:
            raise ValueError(f"watermark_context must be 1, 2 or 3 (wider contexts are not built), got {v!r}")
        return int(v)
    cols = []
    for name, value, one in (("watermark_key", key, one_key), ("watermark_delta", delta, one_delta),
                             ("watermark_gamma", gamma, one_gamma), ("watermark_context", context, one_context)):
        if isinstance(value, (str, bytes)):
            raise ValueError(f"{name} must be one value or one per prompt, got {value!r}")
        cols.append(_per_prompt(value, n, one, f"{name} values"))
    if named and all(k is None for k in cols[0]):
        raise ValueError("watermark_delta, watermark_gamma and watermark_context need a watermark_key on some row")
    return tuple(cols)


def check_prompt_lookup(num_tokens, max_ngram, min_ngram, named: bool = False) -> Optional[Tuple[int, int, int]]:
    """generate's `prompt_lookup_num_tokens` (K: an int in [0, MAX_LOOKUP_TOKENS], 0 = off), `prompt_lookup_max_ngram` (N: an int
    in [1, MAX_LOOKUP_NGRAM]) and `prompt_lookup_min_ngram` (an int in [1, N]) -> (K, N, n0), or None when K is 0.  Each is ONE
    value per call: K shapes the step.  `named`: the call itself names a max or min n-gram; with K == 0 that is an error, as
    are a bool, a float, a sequence, a value outside its range and min above max: ValueError."""
    out = []
    for name, v, lo, hi in (("prompt_lookup_num_tokens", num_tokens, 0, MAX_LOOKUP_TOKENS),
                            ("prompt_lookup_max_ngram", max_ngram, 1, MAX_LOOKUP_NGRAM),
                            ("prompt_lookup_min_ngram", min_ngram, 1, MAX_LOOKUP_NGRAM)):
        if not _is_int(v) or not lo <= int(v) <= hi:
            raise ValueError(f"{name} must be one integer in [{lo}, {hi}] for the call, got {v!r}")
        out.append(int(v))
    if out[2] > out[1]:
        raise ValueError(f"prompt_lookup_min_ngram ({out[2]}) must not exceed prompt_lookup_max_ngram ({out[1]})")
    if out[0] == 0:
        if named:
            raise ValueError("prompt_lookup_max_ngram and prompt_lookup_min_ngram need prompt_lookup_num_tokens > 0")
        return None
    return tuple(out)


def check_guidance(scale, negative, n: int) -> Optional[Tuple[List[float], List[Optional[str]]]]:
    """generate's `guidance_scale` (one finite number in [0, MAX_GUIDANCE_SCALE] for the call or one per prompt, held as f32;
    1 = the row is off) and `negative_prompt` (None, one string for the call, or one string or None per prompt) ->
    (scales, negatives) with one entry per prompt, or None when every row's scale is 1.  A bool, a NaN, a value out of range,
    the wrong length, a negative prompt that is no string, and a negative prompt without a row whose scale differs from 1
    (the mirostat_eta rule): ValueError."""
    def one(v):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or \
                not 0.0 <= float(np.float32(v)) <= MAX_GUIDANCE_SCALE:                   # (NaN fails both comparisons)
            raise ValueError(f"guidance_scale must be a finite number in [0, {MAX_GUIDANCE_SCALE:g}] (1: off) for the call or "
                             f"one per prompt, got {scale!r}")
        return float(np.float32(v))

    def text(v):
        if v is not None and not isinstance(v, str):
            raise ValueError(f"negative_prompt must be None, one string for the call, or one string or None per prompt, got {negative!r}")
        return v
    scales = _per_prompt(scale, n, one, "guidance_scale values")
    negatives = _per_prompt(negative, n, text, "negative_prompt entries")
    if all(s == 1.0 for s in scales):
        if any(v is not None for v in negatives):
            raise ValueError("negative_prompt needs a row whose guidance_scale differs from 1")
        return None
    return scales, negatives


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
