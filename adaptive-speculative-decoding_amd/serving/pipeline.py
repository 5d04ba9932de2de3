"""Adaptive cascade pipeline -- API of the reference's src/serving/pipeline.py, with the decision
arithmetic of the stage loop (Bayes adjustment, DP stop rule) done by batched kernels.

    PipelineConfig                  pipeline.py:22-31   (+ stop_rule, stage_names, stop_token_ids, stop_sequences, logprobs: build
                                                         extensions)
    RequestResult                   pipeline.py:34-45
    AdaptiveSpeculativePipeline     pipeline.py:48-423
        process_request / process_request_async / batch_process / update_lambda / get_stats /
        reset_stats / warmup / shutdown

Per-request seeds (build extension; SamplingParams(seed=...)): `process_request(..., seed=)` and `batch_process(..., seeds=)`
take ints in [0, 2^64) (serving/stages.py, SEEDS; a batch passes a seed for every request or none).  A request's seed travels
with it through every regrouping -- the `predicted_stage` groups, the cache split, the requests that leave the cascade -- and
reaches every stage as `stage.generate(seed=[...])`, so its draws do not depend on the requests it happens to be batched with.
Without seeds the keyword is not passed.

Per-request length limits (the reference's GenerationRequest.max_tokens, src/serving/server.py:43): `batch_process(max_tokens=)`
takes an int or one int >= 1 per request.  A request keeps its own limit (`_Active.max_tokens`) through the same regroupings and
every stage sees `stage.generate(max_tokens=[...])` with the values of that call's rows; with an int the stage sees the int, as
before.  `PipelineConfig.stop_sequences` (also read from the YAML `pipeline:` section) is handed to every stage.generate call as
`stop_sequences=`, only when set (serving/stages.py, HOW A ROW ENDS).

Per-request sampling parameters (the reference's GenerationRequest.temperature / top_p, src/serving/server.py:44-45,67; top_k and
min_p as in vLLM's SamplingParams): `batch_process(temperature=, top_p=, top_k=, min_p=)` take one value or one per request, and
`process_request` takes `top_p=`, `top_k=`, `min_p=`.  A request keeps its values (`_Active`) through the same regroupings and
across stages; a stage sees lists only where the batch carries lists, and one value given for the whole batch as that value, so
calls without them are the calls made before (serving/stages.py, PER-REQUEST SAMPLING).  A stage call cannot mix greedy
(temperature 0) and sampled rows: `batch_process` runs such a batch as a greedy and a sampled sub-batch -- the one place mixing
is handled -- and returns the results in request order.

Logit edits (OpenAI's `logit_bias`, vLLM's `bad_words` / `min_tokens`; serving/stages.py, LOGIT EDITS): `batch_process(logit_bias=,
banned_token_ids=, min_tokens=)` take one value for the batch -- a dict, a sequence of token ids, an int -- or one per request
(a sequence of dicts / Nones, a sequence of id sequences, a sequence of ints), and `process_request` takes the same three for its
one request.  `allowed_token_ids=` (vLLM's; serving/stages.py, ALLOW-LISTS) travels the same way: a sequence of ids for the
batch, or one sequence (or None: no list) per request.  A per-request value travels with the request like its `top_p`; a keyword
reaches `stage.generate` only when it was given.  The values are checked by the stage (which knows the vocabulary); only the per-request lengths are checked here.
`repetition_penalty=`, `presence_penalty=`, `frequency_penalty=` (vLLM's; serving/stages.py, PENALTIES) travel the same way: one
number for the batch or one per request, kept by the request through every regrouping, handed on only when given.
`bad_words=` (vLLM's; serving/stages.py, BAD WORDS) likewise: one list of words for the batch, which reaches the stages as
`bad_words`, or one list (or None) per request, which a request keeps and the stages receive as `bad_words_per_prompt`.
`guided_choice=` (serving/stages.py, GUIDED DECODING) likewise: one list of choices for the batch, which reaches the stages as
`guided_choice`, or one list (or None: the request is free) per request, which a request keeps and the stages receive as
`guided_choice_per_prompt`.
`no_repeat_ngram_size=` (HF generate's; serving/stages.py, NO REPEAT N-GRAM) travels like a penalty: one int in [0, 8] for the
batch or one per request, kept by the request through every regrouping, handed on only when it is set (here or as
`PipelineConfig.no_repeat_ngram_size`).
`PipelineConfig.typical_p` / `epsilon_cutoff` / `eta_cutoff` (HF's warpers of those names; serving/stages.py, ENTROPY CUTS) are
configuration only: a value that is set is handed to every stage's generate call as the keyword of that name, None is not passed.

What the reference's loop does per request (pipeline.py:165-286), and what this one keeps:
  for each stage i:  outputs, logprobs = stage.generate(prompts=[prompt_i], ..., return_logprobs=True)
                     p_i = predictor.predict(...)  (1.0 at the last stage)        :225-241
                     p_i = bayesian_adjustment(p_i, max(100, total_requests), a, b)   :234-238
                     k*  = optimal_stopping_rule(p[:i+1], C[:i+1], lambda)            :251-256
                     stop when k* == i, else prompt_{i+1} = prompt + " " + output     :259-266

`batch_process` really batches: all still-active requests of a stage go through ONE stage.generate call, ONE Bayes
launch and ONE DP launch (`batch_grouping="none"`, the default: one batch, as the reference's call shape implies).
Opt-in `batch_grouping="predicted_stage"` implements the reference's TODO (:331-338: "intelligent batching based on
predicted stages"): the predictor is asked for every request's acceptance probability at every stage from the
PROMPT alone, ONE DP launch over [n, L] turns that into a predicted stop stage, requests are grouped by it and the
groups run shallowest first (a group's requests leave the cascade together, so the stage calls of a group stay
full and easy requests are not held back by hard ones; but it means up to L stage-0 calls on smaller batches and
n * (L - 1) prompt-only predictor calls up front -- one per stage with a predictor that offers `predict_batch` -- so it
is not the default).

stop_rule:
  "prefix" -- the reference's rule verbatim.  Because the DP is run on the prefix p[:i+1], and a
              one-stage problem always stops, this ALWAYS stops at stage 0.
  "full"   -- (default) the DP sees all L stages: observed probabilities for stages <= i, prior
              `stage_priors` for the later ones (1.0 for the last).  This is the behaviour the
              reference's paper describes.
The reference's `_process_stages` also references an undefined `start_time` (NameError, F5); the
latency here is measured from the start of the request.
"""
from __future__ import annotations

import asyncio
import logging
import threading
import time
import uuid
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from ..backend import get_backend
from .cache import RequestCache
from .stages import _is_seq, check_max_tokens, check_per_prompt, check_seeds

logger = logging.getLogger(__name__)

_EDIT_KEYS = ("logit_bias", "banned_token_ids", "min_tokens", "allowed_token_ids")
_PENALTY_KEYS = ("repetition_penalty", "presence_penalty", "frequency_penalty")


def check_logit_edit_args(logit_bias, banned_token_ids, min_tokens, n: int, allowed_token_ids=None) -> Dict[str, Any]:
    """The logit-edit keywords of batch_process (the three sparse ones and the allow-list) -> {name: value} of those that were
    given: a `list` of n values where the batch carries one per request, anything else (a dict, a tuple of ids, an int) is one
    value for the batch.  Only the shapes are looked at here; stage.generate checks the values."""
    out: Dict[str, Any] = {}
    if logit_bias is not None:
        if _is_seq(logit_bias):
            if len(logit_bias) != n:
                raise ValueError(f"{len(logit_bias)} logit_bias dicts for {n} requests")
            out["logit_bias"] = list(logit_bias)
        else:
            out["logit_bias"] = logit_bias
    for name, ids in (("banned_token_ids", banned_token_ids), ("allowed_token_ids", allowed_token_ids)):
        if ids is None:
            continue
        if not _is_seq(ids):
            raise ValueError(f"{name} must be a sequence of token ids or one sequence per request, got {ids!r}")
        vals = list(ids)
        if any(_is_seq(v) or v is None for v in vals):
            if len(vals) != n:
                raise ValueError(f"{len(vals)} {name} lists for {n} requests")
            out[name] = vals
        else:
            out[name] = tuple(vals)
    if min_tokens is not None:
        if _is_seq(min_tokens):
            if len(min_tokens) != n:
                raise ValueError(f"{len(min_tokens)} min_tokens values for {n} requests")
            out["min_tokens"] = list(min_tokens)
        else:
            out["min_tokens"] = min_tokens
    return out


def check_penalty_args(values: Dict[str, Any], n: int) -> Dict[str, Any]:
    """The penalty keywords of batch_process -> {name: value} of those that were given: a `list` of n values where the batch
    carries one per request, anything else is one value for the batch.  Only the shapes are looked at here; stage.generate checks
    the values."""
    out: Dict[str, Any] = {}
    for name, v in values.items():
        if v is None:
            continue
        if _is_seq(v):
            if len(v) != n:
                raise ValueError(f"{len(v)} {name} values for {n} requests")
            out[name] = list(v)
        else:
            out[name] = v
    return out


def check_bad_words_arg(bad_words, n: int) -> Dict[str, Any]:
    """The `bad_words` keyword of batch_process -> {} when it was not given, else {"bad_words": value}: a `list` of n lists where
    the batch carries one list per request (an element that is None, empty or itself holds words), else a tuple of words, the
    batch's one list.  A word is a str or a sequence of token ids.  Only the shapes are looked at here; stage.generate checks
    the values."""
    if bad_words is None:
        return {}
    if not _is_seq(bad_words):
        raise ValueError(f"bad_words must be a list of words or one list per request, got {bad_words!r}")
    vals = list(bad_words)
    per_request = [v is None or (_is_seq(v) and (len(v) == 0 or any(isinstance(x, str) or _is_seq(x) for x in v))) for v in vals]
    if not any(per_request):
        return {"bad_words": tuple(vals)}
    if not all(per_request):
        raise ValueError("bad_words mixes words and per-request lists")
    if len(vals) != n:
        raise ValueError(f"{len(vals)} bad_words lists for {n} requests")
    return {"bad_words": [[] if v is None else list(v) for v in vals]}


def check_guided_choice_arg(guided_choice, n: int) -> Dict[str, Any]:
    """The `guided_choice` keyword of batch_process -> {} when it was not given, else {"guided_choice": value}: a `list` of n
    entries where the batch carries one list per request (an entry that is None, empty or itself holds choices), else a tuple of
    choices, the batch's one list.  A choice is a str or a sequence of token ids.  Only the shapes are looked at here;
    stage.generate checks the values."""
    if guided_choice is None:
        return {}
    if not _is_seq(guided_choice):
        raise ValueError(f"guided_choice must be a list of choices or one list per request, got {guided_choice!r}")
    vals = list(guided_choice)
    per_request = [v is None or (_is_seq(v) and (len(v) == 0 or any(isinstance(x, str) or _is_seq(x) for x in v))) for v in vals]
    if not any(per_request):
        return {"guided_choice": tuple(vals)}
    if not all(per_request):
        raise ValueError("guided_choice mixes choices and per-request lists")
    if len(vals) != n:
        raise ValueError(f"{len(vals)} guided_choice lists for {n} requests")
    return {"guided_choice": [None if v is None else list(v) for v in vals]}


_PER_PROMPT_KEYWORD = {"bad_words": "bad_words_per_prompt", "guided_choice": "guided_choice_per_prompt"}
DEFAULT_STAGE_NAMES = ("8b", "13b", "34b", "70b")          # pipeline.py:175


@dataclass
class PipelineConfig:
    lambda_value: float = 1.0
    risk_adjustment: bool = True
    risk_alpha: float = 1.0
    risk_beta: float = 1.0
    enable_caching: bool = True
    max_concurrent_requests: int = 100
    batch_timeout_ms: float = 50.0
    # --- build extensions (defaults keep the reference's call sites working) ---
    stop_rule: str = "full"                                 # "full" | "prefix" (see module docstring)
    stage_names: Sequence[str] = DEFAULT_STAGE_NAMES
    stage_priors: Optional[Sequence[float]] = None          # prior p for not-yet-run stages ("full")
    batch_grouping: str = "none"                            # batch_process: "none" (one batch, the reference's shape) | "predicted_stage"
    stop_token_ids: Optional[Sequence[int]] = None          # EOS ids handed to stage.generate(stop_token_ids=); None: the keyword is not passed
    # top-N log-probs (the specification's SamplingParams(logprobs=5), RESEARCH_PROTOCOL.md:272-277): handed to
    # stage.generate(logprobs=); the predictor then receives the [n_tokens, N] table as `draft_logprobs` (what
    # FeatureExtractor.extract is written for) in place of the 1-D vector.  None: the keyword is not passed
    logprobs: Optional[int] = None
    # stop strings / token-id sequences handed to stage.generate(stop_sequences=); None: the keyword is not passed
    stop_sequences: Optional[Sequence] = None
    # HF generate's no_repeat_ngram_size, handed to stage.generate(no_repeat_ngram_size=) unless the call names its own; None:
    # the keyword is not passed
    no_repeat_ngram_size: Optional[int] = None
    # HF's typical_p / epsilon_cutoff / eta_cutoff, handed to stage.generate(typical_p=, epsilon_cutoff=, eta_cutoff=); None: the
    # keyword is not passed (serving/stages.py, ENTROPY CUTS)
    typical_p: Optional[float] = None
    epsilon_cutoff: Optional[float] = None
    eta_cutoff: Optional[float] = None
    # vLLM's prompt_logprobs (serving/stages.py, PROMPT LOG-PROBS), handed to every stage.generate(prompt_logprobs=): each
    # stage's entry then carries "prompt_logprobs" and "prompt_ranks"; not fed to the predictor.  None: the keyword is not passed
    prompt_logprobs: Optional[int] = None
    # the per-token statistics (serving/stages.py, TOKEN STATS), handed to every stage.generate(token_stats=): each stage's
    # entry then carries "token_entropy", "token_max_logprobs", "token_ranks" and "features" (the row of the stage's
    # predictor_features), and a predictor with predict_features is fed that row.  None: the keyword is not passed
    token_stats: Optional[bool] = None

    @classmethod
    def from_yaml(cls, path: str) -> "PipelineConfig":
        """Read the `pipeline:` section of a serving YAML (reference schema: configs/serving.yaml:10-30;
        server.py:97-99 reads the same file raw).  Unknown keys are ignored."""
        import yaml
        with open(path, "r") as f:
            sec = (yaml.safe_load(f) or {}).get("pipeline", {}) or {}
        risk = sec.get("risk_adjustment", {})
        if isinstance(risk, bool):
            risk = {"enabled": risk}
        kw = dict(lambda_value=float(sec.get("lambda_value", 1.0)), risk_adjustment=bool(risk.get("enabled", True)),
                  risk_alpha=float(risk.get("alpha", 1.0)), risk_beta=float(risk.get("beta", 1.0)),
                  enable_caching=bool((sec.get("cache", {}) or {}).get("enable_kv_cache", True)),
                  batch_timeout_ms=float((sec.get("batching", {}) or {}).get("batch_timeout_ms", 50.0)))
        if "max_concurrent_requests" in sec:
            kw["max_concurrent_requests"] = int(sec["max_concurrent_requests"])
        if "stop_rule" in sec:
            kw["stop_rule"] = str(sec["stop_rule"])
        if "stage_names" in sec:
            kw["stage_names"] = tuple(sec["stage_names"])
        if "stage_priors" in sec:
            kw["stage_priors"] = tuple(float(x) for x in sec["stage_priors"])
        if "batch_grouping" in sec:
            kw["batch_grouping"] = str(sec["batch_grouping"])
        if sec.get("stop_token_ids") is not None:
            kw["stop_token_ids"] = tuple(int(x) for x in sec["stop_token_ids"])
        if sec.get("logprobs") is not None:
            kw["logprobs"] = int(sec["logprobs"])
        if sec.get("stop_sequences") is not None:
            kw["stop_sequences"] = tuple(e if isinstance(e, str) else tuple(int(t) for t in e) for e in sec["stop_sequences"])
        if sec.get("no_repeat_ngram_size") is not None:
            kw["no_repeat_ngram_size"] = int(sec["no_repeat_ngram_size"])
        for name in ("typical_p", "epsilon_cutoff", "eta_cutoff"):
            if sec.get(name) is not None:
                kw[name] = float(sec[name])
        if sec.get("prompt_logprobs") is not None:
            kw["prompt_logprobs"] = int(sec["prompt_logprobs"])
        if sec.get("token_stats") is not None:
            kw["token_stats"] = bool(sec["token_stats"])
        return cls(**kw)


@dataclass
class RequestResult:
    request_id: str
    output: str
    stopped_at_stage: int
    latency_ms: float
    stage_probabilities: List[float]
    stage_costs: List[float]
    cache_hits: int
    total_tokens: int
    tokens_per_second: float
    # --- build extensions (trailing, defaulted: the reference's positional construction still works) ---
    stages_run: int = 0                                     # stages actually executed (>= stopped_at_stage + 1)
    executed_costs: List[float] = field(default_factory=list)   # cost_per_token of every executed stage
    predicted_stage: int = -1                               # batch_process grouping key (-1: not predicted)


@dataclass
class _Active:
    """Book-keeping of one in-flight request inside a batch."""
    request_id: str
    prompt: str
    current_prompt: str
    start_time: float
    probabilities: List[float] = field(default_factory=list)
    costs: List[float] = field(default_factory=list)
    outputs: List[str] = field(default_factory=list)
    cache_hits: int = 0
    total_tokens: int = 0
    k_star: int = -1
    predicted_stage: int = -1
    seed: Optional[int] = None                              # the request's sampling seed (None: the stage's own generator)
    max_tokens: Optional[int] = None                        # the request's own length limit (None: the batch's one int)
    # the request's own sampling parameters (None: the batch's one value, or the stage's configuration)
    temperature: Optional[float] = None
    top_p: Optional[float] = None
    top_k: Optional[int] = None
    min_p: Optional[float] = None
    edits: Dict[str, Any] = field(default_factory=dict)     # the request's own logit_bias / banned_token_ids / min_tokens / allowed_token_ids / penalties / bad_words / guided_choice / no_repeat_ngram_size


def _fresh_stats(n_stages: int) -> Dict[str, Any]:
    return {"total_requests": 0, "stage_stops": [0] * n_stages, "avg_latency": 0.0,
            "avg_tokens_per_second": 0.0, "total_tokens": 0, "avg_stage_probabilities": [0.0] * n_stages,
            "error_count": 0}


class AdaptiveSpeculativePipeline:
    def __init__(self, stage_manager, predictor, feature_extractor, config: PipelineConfig, cache_manager=None):
        self.stage_manager = stage_manager
        self.predictor = predictor
        self.feature_extractor = feature_extractor
        self.config = config
        if cache_manager is None and config.enable_caching:
            cache_manager = RequestCache()
        self.cache_manager = cache_manager
        self._n_stages = len(config.stage_names)
        self.stats = _fresh_stats(max(4, self._n_stages))
        self._stats_lock = threading.Lock()            # the reference mutates stats from 100 threads unlocked
        self.executor = ThreadPoolExecutor(max_workers=config.max_concurrent_requests)
        self.active_requests: Dict[str, Dict[str, Any]] = {}
        if config.stop_rule not in ("full", "prefix"):
            raise ValueError("stop_rule must be 'full' or 'prefix'")
        if config.batch_grouping not in ("predicted_stage", "none"):
            raise ValueError("batch_grouping must be 'predicted_stage' or 'none'")
        logger.info("AdaptiveSpeculativePipeline initialized")

    # ------------------------------------------------------------------ public API
    def process_request(self, prompt: str, max_tokens: int = 512, temperature: float = 0.7,
                        request_id: Optional[str] = None, seed: Optional[int] = None, top_p: Optional[float] = None,
                        top_k: Optional[int] = None, min_p: Optional[float] = None, logit_bias=None, banned_token_ids=None,
                        min_tokens=None, allowed_token_ids=None, repetition_penalty=None, presence_penalty=None,
                        frequency_penalty=None, bad_words=None, guided_choice=None,
                        no_repeat_ngram_size=None) -> RequestResult:
        """seed: None, or an int in [0, 2^64): the request's sampling seed at every stage (module docstring).
        top_p / top_k / min_p: None = every stage's configuration, else the request's own value at every stage
        (stage.generate(top_p=, top_k=, min_p=)).  logit_bias (a dict) / banned_token_ids (token ids) / min_tokens (an int):
        None = every stage's configuration, else handed to every stage.generate call (module docstring, Logit edits);
        allowed_token_ids (token ids) likewise; repetition_penalty / presence_penalty / frequency_penalty (one number each:
        serving/stages.py, PENALTIES) likewise; bad_words (one list of words, a word a str or a sequence of token ids:
        serving/stages.py, BAD WORDS) likewise; guided_choice (one list of choices, a choice a str or a sequence of token ids:
        serving/stages.py, GUIDED DECODING) likewise; no_repeat_ngram_size (one int in [0, 8]: serving/stages.py, NO REPEAT
        N-GRAM) likewise."""
        if seed is not None and not isinstance(seed, (int, np.integer)):
            raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
        sampling = {k: check_per_prompt(v, 1, k) for k, v in (("top_p", top_p), ("top_k", top_k), ("min_p", min_p))}
        edits = {k: v for k, v in zip(_EDIT_KEYS, (logit_bias, banned_token_ids, min_tokens, allowed_token_ids)) if v is not None}
        for name in ("banned_token_ids", "allowed_token_ids"):
            if _is_seq(edits.get(name)):
                edits[name] = tuple(edits[name])                                 # (one value for the batch of one, never a list)
        if _is_seq(edits.get("logit_bias")) or _is_seq(edits.get("min_tokens")):
            raise ValueError("process_request takes one logit_bias dict and one min_tokens int")
        for name, v in zip(_PENALTY_KEYS, (repetition_penalty, presence_penalty, frequency_penalty)):
            if _is_seq(v):
                raise ValueError(f"process_request takes one {name} number")
            if v is not None:
                edits[name] = v
        words = check_bad_words_arg(bad_words, 1)
        if isinstance(words.get("bad_words"), list):
            raise ValueError("process_request takes one bad_words list of words")
        edits.update(words)
        choices = check_guided_choice_arg(guided_choice, 1)
        if isinstance(choices.get("guided_choice"), list):
            raise ValueError("process_request takes one guided_choice list of choices")
        edits.update(choices)
        if _is_seq(no_repeat_ngram_size):
            raise ValueError("process_request takes one no_repeat_ngram_size integer")
        if no_repeat_ngram_size is not None:
            edits["no_repeat_ngram_size"] = no_repeat_ngram_size
        return self._run_batch([prompt], max_tokens, temperature, [request_id], seeds=check_seeds(seed, 1), sampling=sampling,
                               edits=edits)[0]

    async def process_request_async(self, prompt: str, max_tokens: int = 512, temperature: float = 0.7,
                                    request_id: Optional[str] = None, seed: Optional[int] = None) -> RequestResult:
        loop = asyncio.get_event_loop()
        return await loop.run_in_executor(self.executor, self.process_request, prompt, max_tokens, temperature,
                                          request_id, seed)

    def batch_process(self, prompts: List[str], max_tokens=512, temperature=0.7,
                      seeds=None, top_p=None, top_k=None, min_p=None, logit_bias=None, banned_token_ids=None,
                      min_tokens=None, allowed_token_ids=None, repetition_penalty=None, presence_penalty=None,
                      frequency_penalty=None, bad_words=None, guided_choice=None,
                      no_repeat_ngram_size=None) -> List[RequestResult]:
        """seeds: None, one int in [0, 2^64) for every request, or one per request (all or none: a sequence that holds None
        raises ValueError); request i keeps seeds[i] through every regrouping (module docstring).  max_tokens: an int, or one
        int >= 1 per request, kept by the request in the same way.
        temperature, top_p, top_k, min_p: one value for the batch (None: every stage's configuration), or one per request,
        kept by the request through every regrouping and handed to stage.generate as a list only where the batch has one
        (serving/stages.py, PER-REQUEST SAMPLING).  A stage call cannot mix greedy (temperature 0) and sampled rows: a batch
        whose temperatures do is run as a greedy and a sampled sub-batch here, and the results come back in request order.
        logit_bias, banned_token_ids, min_tokens, allowed_token_ids: None (the keyword is not handed to the stages), one value
        for the batch, or one per request, kept by the request through every regrouping (module docstring, Logit edits).
        repetition_penalty, presence_penalty, frequency_penalty: None (not handed on), one number for the batch, or one per
        request, travelling like the edits (serving/stages.py, PENALTIES).
        bad_words: None (not handed on), one list of words for the batch (stage.generate(bad_words=)), or one list (or None:
        no word) per request, kept by the request and handed on as bad_words_per_prompt (serving/stages.py, BAD WORDS).
        guided_choice: None (not handed on), one list of choices for the batch (stage.generate(guided_choice=)), or one list (or
        None: the request is free) per request, kept by the request and handed on as guided_choice_per_prompt (serving/stages.py,
        GUIDED DECODING).
        no_repeat_ngram_size: None (not handed on, unless the configuration sets one), one int in [0, 8] for the batch, or one
        per request, travelling like a penalty (serving/stages.py, NO REPEAT N-GRAM)."""
        prompts = list(prompts)
        n = len(prompts)
        seeds = check_seeds(seeds, n)
        max_tokens = check_max_tokens(max_tokens, n)
        sampling = {k: check_per_prompt(v, n, k) for k, v in (("top_p", top_p), ("top_k", top_k), ("min_p", min_p))}
        edits = check_logit_edit_args(logit_bias, banned_token_ids, min_tokens, n, allowed_token_ids)
        edits.update(check_penalty_args(dict(zip(_PENALTY_KEYS, (repetition_penalty, presence_penalty, frequency_penalty))), n))
        edits.update(check_bad_words_arg(bad_words, n))
        edits.update(check_guided_choice_arg(guided_choice, n))
        edits.update(check_penalty_args({"no_repeat_ngram_size": no_repeat_ngram_size}, n))
        if isinstance(temperature, (Sequence, np.ndarray)) and not isinstance(temperature, (str, bytes)):
            temperature = check_per_prompt(temperature, n, "temperature")
        if isinstance(temperature, list) and any(t == 0.0 for t in temperature):
            # the one place greedy and sampled requests are mixed: two sub-batches, results in request order
            results: List[Optional[RequestResult]] = [None] * n
            for greedy in (True, False):
                idx = [i for i, t in enumerate(temperature) if (t == 0.0) == greedy]
                pick = lambda v: [v[i] for i in idx] if isinstance(v, list) else v      # noqa: E731
                out = self.batch_process([prompts[i] for i in idx], pick(max_tokens), pick(temperature), pick(seeds),
                                         **{k: pick(v) for k, v in sampling.items()}, **{k: pick(v) for k, v in edits.items()})
                for i, r in zip(idx, out):
                    results[i] = r
            return results  # type: ignore[return-value]
        if self.config.batch_grouping != "predicted_stage" or n < 2 or self.config.stop_rule == "prefix":
            return self._run_batch(prompts, max_tokens, temperature, [None] * n, seeds=seeds, sampling=sampling, edits=edits)
        pred = self.predict_stop_stages(prompts)
        results = [None] * n
        for stage in sorted(set(pred.tolist())):                       # shallowest group first
            idx = [i for i, s in enumerate(pred) if s == stage]
            pick = lambda v: [v[i] for i in idx] if isinstance(v, list) else v          # noqa: E731
            out = self._run_batch([prompts[i] for i in idx], pick(max_tokens), pick(temperature),
                                  [None] * len(idx),
                                  predicted=[int(stage)] * len(idx), seeds=None if seeds is None else [seeds[i] for i in idx],
                                  sampling={k: pick(v) for k, v in sampling.items()},
                                  edits={k: pick(v) for k, v in edits.items()})
            for i, r in zip(idx, out):
                results[i] = r
        return results  # type: ignore[return-value]

    def predict_stop_stages(self, prompts: Sequence[str]) -> np.ndarray:
        """The grouping key of batch_process: the stage the DP rule would stop at if every stage's acceptance
        probability were what the predictor says from the prompt alone (no output, no log-probs yet).  One Bayes
        launch and ONE DP launch for all n requests x L stages."""
        cfg = self.config
        names = list(cfg.stage_names)
        L = len(names)
        P = np.ones((len(prompts), L), dtype=np.float64)
        batched = getattr(self.predictor, "predict_batch", None)
        for i in range(L - 1):
            if batched is not None:                                     # ONE predictor forward per stage for the whole batch
                P[:, i] = np.asarray(batched(prompts=list(prompts), draft_outputs=[""] * len(prompts), draft_logprobs=None,
                                             stage_id=i, feature_extractor=self.feature_extractor), dtype=np.float64)
            else:                                                       # the reference's per-request predictor interface
                for j, prompt in enumerate(prompts):
                    P[j, i] = float(self.predictor.predict(prompt=prompt, draft_output="", draft_logprobs=None, stage_id=i,
                                                           feature_extractor=self.feature_extractor))
        backend = get_backend()
        if cfg.risk_adjustment:
            with self._stats_lock:
                n_obs = max(100, self.stats["total_requests"])
            P[:, :L - 1] = backend.bayes_adjust(P[:, :L - 1].reshape(-1), n_obs, cfg.risk_alpha, cfg.risk_beta).reshape(-1, L - 1)
        costs = np.array([float(self.stage_manager.get_stage(n).cost_per_token) for n in names])
        k_star, _ = backend.optimal_stopping(P, costs, cfg.lambda_value, False, 1.0, 1.0)
        return np.asarray(k_star, dtype=np.int64)

    def update_lambda(self, new_lambda: float):
        old = self.config.lambda_value
        self.config.lambda_value = new_lambda
        logger.info("Updated lambda: %.3f -> %.3f", old, new_lambda)

    def get_stats(self) -> Dict[str, Any]:
        with self._stats_lock:
            stats = dict(self.stats)
            stats["stage_stops"] = list(stats["stage_stops"])
            stats["avg_stage_probabilities"] = list(stats["avg_stage_probabilities"])
        n = stats["total_requests"]
        if n > 0:
            stats["stage_distribution"] = [c / n for c in stats["stage_stops"]]
            stats["avg_tokens_per_request"] = stats["total_tokens"] / n
        else:
            stats["stage_distribution"] = [0.0] * len(stats["stage_stops"])
            stats["avg_tokens_per_request"] = 0.0
        if self.cache_manager:
            stats["cache_stats"] = self.cache_manager.get_stats()
        stats["active_requests"] = len(self.active_requests)
        # telemetry of the token-level hot path behind the stages, when one is attached ("keep get_stats() keys;
        # add hbm_gbps, kernel_us"): the last verify step of a profiling HipOps
        hot = getattr(self, "hot_path_ops", None)
        if hot is not None:
            stats.update({k: v for k, v in hot.stats().items() if k in ("kernel_us", "hbm_gbps")})
        return stats

    def attach_hot_path(self, ops) -> None:
        """ops: the distributed.HipOps (profile=True) the stages verify with; get_stats() then carries `kernel_us` and
        `hbm_gbps` of its last verify step."""
        self.hot_path_ops = ops

    def reset_stats(self):
        with self._stats_lock:
            self.stats = _fresh_stats(max(4, self._n_stages))
        logger.info("Pipeline statistics reset")

    def warmup(self, num_requests: int = 5):
        prompts = ["Hello, how are you today?", "What is the capital of France?",
                   "Explain machine learning in simple terms.", "Write a short poem about nature.",
                   "What are the benefits of renewable energy?"]
        for i in range(num_requests):
            try:
                self.process_request(prompt=prompts[i % len(prompts)], max_tokens=50, temperature=0.7)
            except Exception as e:  # noqa: BLE001  (reference: log and continue, pipeline.py:407-408)
                logger.warning("Warmup request %d failed: %s", i + 1, e)

    def shutdown(self):
        self.executor.shutdown(wait=True)
        logger.info("Pipeline shutdown completed")

    # ------------------------------------------------------------------ the stage loop, batched
    def _run_batch(self, prompts: List[str], max_tokens, temperature,
                   request_ids: List[Optional[str]], predicted: Optional[List[int]] = None,
                   seeds: Optional[List[int]] = None, sampling: Optional[Dict[str, Any]] = None,
                   edits: Optional[Dict[str, Any]] = None) -> List[RequestResult]:
        now = time.time()
        reqs = [_Active(request_id=rid or str(uuid.uuid4()), prompt=p, current_prompt=p, start_time=now)
                for p, rid in zip(prompts, request_ids)]
        if predicted is not None:
            for r, s in zip(reqs, predicted):
                r.predicted_stage = s
        if seeds is not None:
            for r, s in zip(reqs, seeds):
                r.seed = s
        if isinstance(max_tokens, list):
            for r, n in zip(reqs, max_tokens):
                r.max_tokens = n
        # per-request sampling parameters: kept by the request where the batch has a list; a batch-wide value stays batch-wide
        sampling = dict(sampling or {})
        shared = {k: v for k, v in sampling.items() if v is not None and not isinstance(v, list)}
        for name, v in list(sampling.items()) + [("temperature", temperature)]:
            if isinstance(v, list):
                for r, x in zip(reqs, v):
                    setattr(r, name, x)
        # logit edits likewise: a list is one value per request, anything else is the batch's one value
        for name, v in (edits or {}).items():
            if isinstance(v, list):
                for r, x in zip(reqs, v):
                    r.edits[name] = x
            else:
                shared[name] = v
        for r in reqs:
            self.active_requests[r.request_id] = {"start_time": r.start_time,
                                                  "prompt": r.prompt[:100] + "..." if len(r.prompt) > 100 else r.prompt}
        try:
            self._process_stages(reqs, max_tokens, temperature, shared)
            results = [self._finish(r) for r in reqs]
            for res in results:
                self._update_stats(res)
            return results
        except Exception as e:
            logger.error("Batch of %d request(s) failed: %s", len(reqs), e)
            with self._stats_lock:
                self.stats["error_count"] += len(reqs)
            raise
        finally:
            for r in reqs:
                self.active_requests.pop(r.request_id, None)
                if self.cache_manager:
                    self.cache_manager.cleanup_request(r.request_id)

    def _predict(self, r: _Active, stage_idx: int, output: str, logprobs, features=None) -> float:
        if features is not None and hasattr(self.predictor, "predict_features"):       # the stage's own feature row (TOKEN STATS)
            return float(self.predictor.predict_features(np.asarray(features, dtype=np.float32)[None, :])[0])
        return float(self.predictor.predict(prompt=r.current_prompt, draft_output=output, draft_logprobs=logprobs,
                                            stage_id=stage_idx, feature_extractor=self.feature_extractor))

    def _process_stages(self, reqs: List[_Active], max_tokens, temperature, shared: Optional[Dict[str, Any]] = None) -> None:
        cfg = self.config
        names = list(cfg.stage_names)
        L = len(names)
        backend = get_backend()
        active = list(reqs)
        for i, name in enumerate(names):
            if not active:
                break
            stage = self.stage_manager.get_stage(name)
            last_stage = i == L - 1
            # -- generation: cached outputs first, one generate() call for the rest
            todo, cached = [], {}
            for r in active:
                hit = self.cache_manager.get_cache(r.request_id, i) if self.cache_manager else None
                if hit:
                    r.cache_hits += 1                                              # any cached entry counts (pipeline.py:192-194)
                if hit and hit.get("output"):
                    cached[r.request_id] = hit["output"]
                else:
                    todo.append(r)
            gen_out: Dict[str, Any] = {}
            feat_out: Dict[str, Any] = {}                               # token_stats: every generated request's feature row
            if todo:
                stop_kw = {} if cfg.stop_token_ids is None else {"stop_token_ids": tuple(cfg.stop_token_ids)}
                if cfg.logprobs is not None:
                    stop_kw["logprobs"] = int(cfg.logprobs)
                if todo[0].seed is not None:                            # (a batch carries seeds for all of its requests or for none)
                    stop_kw["seed"] = [r.seed for r in todo]
                if cfg.stop_sequences is not None:
                    stop_kw["stop_sequences"] = list(cfg.stop_sequences)
                if cfg.no_repeat_ngram_size is not None:                # (the call's own value, shared or per request, replaces it below)
                    stop_kw["no_repeat_ngram_size"] = int(cfg.no_repeat_ngram_size)
                for name in ("typical_p", "epsilon_cutoff", "eta_cutoff"):      # the entropy cuts: only those that are set
                    if getattr(cfg, name) is not None:
                        stop_kw[name] = getattr(cfg, name)
                if cfg.prompt_logprobs is not None:
                    stop_kw["prompt_logprobs"] = cfg.prompt_logprobs
                if cfg.token_stats is not None:
                    stop_kw["token_stats"] = cfg.token_stats
                # (limits likewise: one per request of the batch, or the batch's one int)
                limit = [r.max_tokens for r in todo] if isinstance(max_tokens, list) else max_tokens
                # (sampling parameters likewise: a list only where the batch carries one, so other calls are unchanged)
                stop_kw.update(shared or {})
                for name in ("top_p", "top_k", "min_p"):
                    if getattr(todo[0], name) is not None:
                        stop_kw[name] = [getattr(r, name) for r in todo]
                for name in todo[0].edits:                              # (a batch carries a per-request edit for all requests or none)
                    # (per-request bad words and choices have keywords of their own at the stage: `bad_words` is its common list,
                    # `guided_choice` the one list of every row)
                    stop_kw[_PER_PROMPT_KEYWORD.get(name, name)] = [r.edits[name] for r in todo]
                temp = [r.temperature for r in todo] if isinstance(temperature, list) else temperature
                texts, logprobs, stage_stats = stage.generate(prompts=[r.current_prompt for r in todo],
                                                              max_tokens=limit, temperature=temp,
                                                              return_logprobs=True, **stop_kw)
                tables = (stage_stats or {}).get("top_logprobs") if cfg.logprobs else None
                for j, r in enumerate(todo):
                    lp = logprobs[j] if logprobs is not None and len(logprobs) > j else np.array([])
                    entry = {"output": texts[j], "logprobs": lp}
                    if tables is not None:                              # the [n_j, N] table takes the vector's place at the predictor
                        entry["top_logprobs"] = lp = tables[j]
                    if cfg.prompt_logprobs is not None and "prompt_logprobs" in (stage_stats or {}):
                        entry["prompt_logprobs"] = stage_stats["prompt_logprobs"][j]       # (kept with the entry, not predicted on)
                        entry["prompt_ranks"] = stage_stats["prompt_ranks"][j]
                    if cfg.token_stats is not None and "predictor_features" in (stage_stats or {}):
                        for key in ("token_entropy", "token_max_logprobs", "token_ranks"):
                            entry[key] = stage_stats[key][j]
                        entry["features"] = feat_out[r.request_id] = stage_stats["predictor_features"][j]
                    gen_out[r.request_id] = (texts[j], lp)
                    if self.cache_manager:
                        self.cache_manager.allocate(r.request_id, i, entry)
                logger.debug("Stage %d: %d generated, time=%.1fms", i, len(todo),
                             float(stage_stats.get("generation_time_ms", 0.0)) if stage_stats else 0.0)
            # -- predictor (host objects, per request as in the reference) ...
            probs = np.ones(len(active), dtype=np.float64)
            for j, r in enumerate(active):
                text, lp = gen_out.get(r.request_id, (cached.get(r.request_id), np.array([])))
                r.outputs.append(text)
                r.costs.append(float(stage.cost_per_token))
                r.total_tokens += len(text.split())
                if not last_stage:
                    probs[j] = self._predict(r, i, text, lp if len(lp) else None, feat_out.get(r.request_id))
            # ... then ONE Bayes launch and ONE DP launch for the whole batch
            if not last_stage and cfg.risk_adjustment:
                with self._stats_lock:
                    n_obs = max(100, self.stats["total_requests"])                 # pipeline.py:235
                probs = backend.bayes_adjust(probs, n_obs, cfg.risk_alpha, cfg.risk_beta)
            for j, r in enumerate(active):
                r.probabilities.append(float(probs[j]))
            if cfg.stop_rule == "prefix":
                P = np.array([r.probabilities for r in active], dtype=np.float64)       # [n, i+1]
                costs = np.array(active[0].costs, dtype=np.float64)
            else:
                P = np.ones((len(active), L), dtype=np.float64)
                if cfg.stage_priors is not None:
                    P[:, :] = np.asarray(cfg.stage_priors, dtype=np.float64)[None, :L]
                P[:, L - 1] = 1.0
                P[:, :i + 1] = np.array([r.probabilities for r in active], dtype=np.float64)
                costs = np.array([float(self.stage_manager.get_stage(n).cost_per_token) for n in names])
            k_star, _ = backend.optimal_stopping(P, costs, cfg.lambda_value, False, 1.0, 1.0)
            still = []
            for j, r in enumerate(active):
                r.k_star = int(k_star[j])
                if last_stage:
                    continue
                # "prefix": the reference's test verbatim (k* == i, pipeline.py:259-261).  "full": k* <= i also
                # stops -- the rule says the best stopping point is already behind us; its output is returned.
                stop = (r.k_star == i) if cfg.stop_rule == "prefix" else (r.k_star <= i)
                if stop:
                    continue
                r.current_prompt = r.prompt + " " + r.outputs[-1]                 # pipeline.py:266
                still.append(r)
            active = still

    def _finish(self, r: _Active) -> RequestResult:
        k = r.k_star if 0 <= r.k_star < len(r.outputs) else len(r.outputs) - 1
        total_ms = (time.time() - r.start_time) * 1000
        tps = r.total_tokens / (total_ms / 1000) if total_ms > 0 else 0
        if self.cache_manager:
            self.cache_manager.truncate_at_stage(r.request_id, k)
        return RequestResult(request_id=r.request_id, output=r.outputs[k], stopped_at_stage=k, latency_ms=total_ms,
                             stage_probabilities=r.probabilities, stage_costs=r.costs[:k + 1],
                             cache_hits=r.cache_hits, total_tokens=r.total_tokens, tokens_per_second=tps,
                             stages_run=len(r.outputs), executed_costs=list(r.costs), predicted_stage=r.predicted_stage)

    def _update_stats(self, result: RequestResult):
        a = 0.01                                                                   # pipeline.py:295
        with self._stats_lock:
            st = self.stats
            st["total_requests"] += 1
            if result.stopped_at_stage < len(st["stage_stops"]):
                st["stage_stops"][result.stopped_at_stage] += 1
            st["total_tokens"] += result.total_tokens
            st["avg_latency"] = (1 - a) * st["avg_latency"] + a * result.latency_ms
            st["avg_tokens_per_second"] = (1 - a) * st["avg_tokens_per_second"] + a * result.tokens_per_second
            for i, prob in enumerate(result.stage_probabilities):
                if i < len(st["avg_stage_probabilities"]):
                    st["avg_stage_probabilities"][i] = (1 - a) * st["avg_stage_probabilities"][i] + a * prob
