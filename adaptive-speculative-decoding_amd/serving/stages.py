"""Stages behind the pipeline: `StageConfig`, `Stage`, `StageManager` -- the reference's missing src/models/stage.py
(imported by src/serving/pipeline.py:14, constructed by src/serving/server.py:131-202, sketched in
docs/guides/RESEARCH_PROTOCOL.md:233-304), with the token-level HIP loop underneath.

`AdaptiveSpeculativePipeline` asks a stage for `generate(prompts=, max_tokens=, temperature=, return_logprobs=True)
-> (texts, logprobs, stats)` (pipeline.py:204-221) and feeds the per-token log-probs to the quality predictor.  Here a stage
is a `SyntheticLM` (model execution is plumbing, third party in the reference) and the decoding around it is the kernels':

  stage 0     plain sampled decoding.  Per step: one model pass, one asd_draft_sample[_top_k] call (token + log q(token)),
              one asd_commit_step_lp call with K = 0 (token and log-prob appended on the device).
  stage s>0   speculative decoding with stage s-1's model as the draft: the ragged draft -> verify -> commit loop in the
              step order of serving/speculative.py::speculative_generate_ragged, written on the `ops` abstraction
              (distributed.HipOps; the CPU tests inject an oracle twin).  The commit draw is asd_residual_sample_lp and the
              commit is asd_commit_step_lp, so every committed token arrives with its TARGET log-prob: the verify's lp_target
              for the accepted draft tokens, log p_t^N(drawn) for the token drawn behind them.  The output is distributed as
              stage s's own model samples (the loop is lossless), and its log-probs are that model's -- what the reference's
              stage would report.

Nothing synchronises inside a step; the host reads min(seq_len) every `sync_every` steps, and `ops.check_status()` runs before
results are returned.

STOP TOKENS (EOS).  With a stop set (`StageConfig.stop_token_ids`, or `generate(stop_token_ids=...)`; at most 8 distinct ids) both
loops commit through asd_commit_step_stop: a sequence ends behind the first COMMITTED token that is a stop id -- the token is kept,
with its log-prob; a rejected draft token never ends anything -- or at `max_tokens`.  The kernel keeps a per-sequence flag
(1 stop, 2 length) and a counter of finished sequences; the host reads that ONE int32 every `sync_every` steps (in place of
min(seq_len); the plain loop gains the same read) and leaves the loop when it equals the batch size.  A finished sequence stays in
the batch: its length, and so every position it is fed at, is frozen, its draws are discarded by the commit and its model work is
wasted -- compacting the batch is not done here.  texts[i] / logprobs[i] then hold n_i tokens, 1 <= n_i <= max_tokens, and `stats`
says why each sequence ended.  Without a stop set a stage runs the asd_commit_step_lp path and every sequence returns exactly
`max_tokens` tokens and log-probs.

HOW A ROW ENDS (per request).  `generate(max_tokens=[...])` gives every prompt its own limit (buffers are sized by the largest),
`generate(stop_sequences=[...])` / `StageConfig.stop_sequences` adds stop strings or token-id sequences of 1..8 ids for every
prompt, and `generate(stop_sequences_per_prompt=[[...], ...])` adds a list for each prompt alone.  A string is encoded by the
stage's tokenizer and folded into the vocabulary like a prompt.  A row's list is its stop ids (as length-1 sequences), then the
common sequences, then its own: at most 16 distinct entries.  With unequal limits or any sequence, both loops commit through
asd_commit_step_finish in place of asd_commit_step_stop: a step commits up to draft_len + 1 tokens, so a sequence may end inside
the accepted prefix, on the drawn token, or begin in tokens an earlier step committed; the kernel matches over the row's
committed stream and the step's committed candidates only -- never a rejected draft token, never a prompt token, never a token
the row's limit cuts off -- and keeps the matched tokens, with their log-probs.  The loop ends on the same one-counter read.
stats["stop_matches"][i] names the sequence that ended row i ((id,) for a stop id, None for "length"), so a caller can trim it.
With one limit and no sequence a stage makes exactly the calls described above.  Not built: removing finished rows from the
batch, and serving/hierarchy.py's loop (`min_tokens` is built: LOGIT EDITS below).  Bad values raise ValueError before any launch.

GREEDY DECODING.  `temperature == 0.0` (the reference's server and core types allow it; it is the setting of reproducible
evaluation runs) selects arg-max decoding on ops.verify_greedy (asd_verify_greedy): stage 0 makes one K = 0 call per step, a
verifying stage drafts with K = 0 calls on the draft's logits and makes ONE call on the target's [B, K+1, V] output, in place.
The generator is not consumed (the result does not depend on StageConfig.seed), top_p / top_k / target_top_p / target_top_k are
ignored (the arg-max is in every nucleus), and the log-probs are the model's at temperature 1 (what vLLM returns for
temperature 0).  Ties go to the lowest id.  Stop tokens work as above.  Negative temperatures raise.

TOP-N LOG-PROBS.  `generate(logprobs=N)` (or `StageConfig.logprobs`), 1 <= N <= 8, is the specification's
`SamplingParams(logprobs=N)` (RESEARCH_PROTOCOL.md:272-277): for every committed token, the N most likely tokens of the
distribution it came from and their log-probs, in `stats["top_token_ids"]` / `stats["top_logprobs"]`.  Every loop adds one
ops.top_logprobs call per step (asd_top_logprobs) -- a verifying stage on the target's [B, K+1, V] output as returned, stage 0
on its [B, V] logits -- and one ops.commit_top_logprobs call behind the step's commit, which moves row j of the step to the
position of the step's j-th committed token on the device (accepted draft token j was scored by row j, the token drawn behind
the prefix by row n_acc).  The draft model's proposal rows get no table.  Nothing is read back inside a step, the generator is
not consumed, and tokens and log-probs are the same bits with and without the table.  The table is the UNTRUNCATED
temperature-scaled distribution (temperature 1 when greedy): with top-k / top-p active the committed token's own log-prob is
renormalised over the nucleus and so is not less than its table entry, and a committed token always lies inside the nucleus.
COST: a sampled verifying step then reads the target rows three times (verify, residual draw, top-N), about one more verify
kernel's time in a step dominated by the model passes; with `logprobs` off (0, the default) a stage runs exactly the launches
it ran before.

MIN-P.  `StageConfig.min_p` (the stage's own draws: stage 0, and the proposals its model makes for the stage above) and
`StageConfig.target_min_p` (a verifying stage's own distribution), or `generate(min_p=...)` for the call, are HF's
MinPLogitsWarper / vLLM's `min_p`, last in the chain Temperature -> TopK -> TopP -> MinP: a token is kept when its probability is
at least min_p times the row's largest.  On raw logits that is one more threshold, x_max + T ln(min_p), so the draw, the verify
and the commit draw take max(top-k / top-p threshold, that) from one select (asd_draft_sample_min_p, asd_verify_accept_min_p,
asd_residual_sample_lp_min_p) and the loop stays lossless.  0 (the default) is off: a stage then makes exactly the calls it
made before.  Values outside [0, 1] raise ValueError.  Greedy decoding ignores min-p, and the top-N table stays the
untruncated distribution.

SEEDS.  `generate(seed=...)` is the serving parameter `SamplingParams(seed=...)`: one int in [0, 2^64) for every prompt of the
call, or one per prompt.  A seeded call draws nothing from the stage's torch.Generator and launches no torch.rand: every step
makes ONE ops.step_uniforms call (asd_step_uniforms, Philox4x32-10 keyed by the row's seed, counter (step, slot, stage, 0)) that
writes all the uniforms of the step -- stage 0 its one proposal uniform, a verifying stage the draft_len proposal uniforms, the
[B, draft_len] accept uniforms and the commit uniform -- where a sampled verifying step of an unseeded call launches
draft_len + 2 torch.rand kernels.  `step` is the loop's own 0-based step index (a finished sequence keeps stepping with the
batch, so it is every sequence's own step count) and `stage` is the stage's index; every draw has its own counter and output
word, so the loop stays lossless.  What a seed guarantees: a row's uniforms depend only on its seed, the stage index and the
step -- not on its row index, the batch size, the other requests, earlier calls, StageConfig.seed or draft_len.  What it does
not: left-padding still makes a row's LOGITS depend on the longest prompt of the call, and the model kernels may pick other
tilings at another batch size.  So bit-equal text is promised for the same call repeated, and for a permuted batch of
equal-length prompts (seeds permuted with them); it is not promised across batch sizes.  `seed=None` (the default) is the
behaviour described above, with exactly the ops calls and generator use it had; greedy decoding makes no call and ignores the
seed.  A bool, a float, a negative value, a value >= 2^64, a sequence of the wrong length or one that holds None raise ValueError.

PER-REQUEST SAMPLING.  `generate(temperature=, top_p=, top_k=, min_p=)` each take one value for the call, as before, or one
value per prompt: a batch is a set of independent requests (the reference's GenerationRequest carries temperature and top_p
per request, src/serving/server.py:44-45,67; vLLM's SamplingParams and HF generate add top_k and min_p).  `top_k` (None = the
configuration's) overrides StageConfig.top_k at stage 0 and target_top_k at a verifying stage, the rule top_p and min_p
follow.  Off, per prompt: top_k <= 0 or >= vocabulary, top_p outside (0, 1), min_p == 0.  A sequence whose values are all equal
is that one value, and a call without an unequal sequence makes exactly the ops calls it made before.  With any unequal
sequence the call takes the ROWS route: the stage packs, once, a table `own` (each row's temperature with its own top-k / top-p
/ min-p) and, at a verifying stage, a table `draft` (each row's temperature with the DRAFT stage's configured top_k / top_p /
min_p), through ops.pack_sampling_rows (asd_sampling_rows_pack); per step it then calls ops.draft_sample_rows for every
proposal (stage 0 with `own`, a verifying stage with `draft`), ops.verify_accept_rows(score, tok, lp_d, u, own),
ops.residual_sample_lp_rows(..., own, d_threshold, t_threshold) and, with logprobs = N, ops.top_logprobs_rows with the rows'
own temperatures.  Row b of such a call is computed as the call with row b's four values computes it (the kernels branch per
workgroup into the select of the row's mode: the same bits), except that the verify of a row that truncates nothing runs the
select kernel too and agrees with the plain verify kernel to 1e-5, not bit for bit.  Commits, stop handling, seeds, the kept
step records and the host reads are unchanged; nothing new is read back inside a step.  A temperature sequence of zeros is the
greedy call.  NOT BUILT: greedy and sampled rows in one call (a temperature sequence that mixes 0 with positive values raises
ValueError; AdaptiveSpeculativePipeline.batch_process splits such a batch in two), per-request truncation of the DRAFT side
(the proposals of a verifying stage use the draft stage's configuration), and serving/hierarchy.py's loop.  A bool, a NaN, a
negative temperature, a min_p outside [0, 1], a non-integer top_k, a sequence of the wrong length or one that holds None raise
ValueError before any launch.

LOGIT EDITS.  `generate(logit_bias=, banned_token_ids=, min_tokens=)` (or the StageConfig fields of those names; a keyword of
None takes the configuration's value) change the distribution itself, ahead of every sampler: the order is edit -> temperature
-> top-k -> top-p -> min-p.  `logit_bias` is OpenAI's / vLLM's: {token id: bias} for every prompt, or one dict (or None) per
prompt; the bias is in RAW logit units, added before the temperature, a finite number in [-100, 100] (the range OpenAI
documents; inside it an f16 logit cannot be pushed to +inf, which the samplers forbid).  `banned_token_ids` (vLLM's `bad_words`
for single tokens) is a sequence of ids for every prompt, or one sequence per prompt: the logit becomes -inf; a banned id wins
over a bias on the same id.  `min_tokens` (vLLM's) is an int >= 0, or one per prompt: while row i has generated fewer than
min_tokens[i] tokens, every length-1 entry of its stop list -- the stop ids and the one-token stop sequences -- is banned, so
such a row ends by "stop" with n_i >= min_tokens[i] + 1, or by "length".  All three are ONE operation, a sparse edit of a few
logits per row: the host merges them per row into distinct (id, bias, until) entries -- a banned id gets until = INT32_MAX, a
stop id under min_tokens gets until = min_tokens and keeps its bias for afterwards, a plain bias has until = 0; at most
MAX_LOGIT_EDITS = 1024 per row -- uploads them once (ops.pack_logit_edits; equal rows share one list), and every loop calls
ops.logit_edit_rows (asd_logit_edit_rows, in place) once per logits tensor: stage 0 on the step's [B, V] logits before the
draw and the top-N pass; a verifying stage on every proposal's draft logits (offset = the draft slot k; the copy kept for
the residual is the edited one) and on the target's [B, K+1, V] output before anything is sliced from or scored on it.  The
edit sees seq_len as it is before the step's commit, so row j of a step knows which generated token it decides.  Draft and
target receive the SAME edit, so the draft -> verify -> residual chain stays lossless against the edited target distribution.
Consequences: the returned log-probs and the top-N tables are those of the EDITED distribution; a banned token is never
listed; a banned token is never proposed, accepted or drawn.  The rows route, seeds, the stop and finish routes, greedy decoding
and `logprobs = N` are untouched and compose with the edit.  A call whose merged lists are all empty (no keyword, an empty
dict or list, min_tokens 0, biases of 0) makes exactly the ops calls it made before.  ValueError before any launch: a bool,
non-integer or out-of-vocabulary id, a bias that is no number, NaN or outside [-100, 100], a negative or non-integer
min_tokens, a sequence of the wrong length, more than 1024 entries in one row after merging, a row whose banned ids (for ever
or at its first token) would leave no token.  NOT BUILT: `min_tokens` > 0 on a row whose stop list holds a MULTI-token
sequence raises ValueError (the match would have to be suppressed in the commit kernels, which stay as they are); and
serving/hierarchy.py's loop.  (Allow-lists are a dense mask, not a sparse edit: the next section; the stateful penalties keep
per-token state: PENALTIES below; multi-token `bad_words` depend on the row's history: BAD WORDS below; automata: GUIDED DECODING.)

ALLOW-LISTS.  `generate(allowed_token_ids=)` (or StageConfig.allowed_token_ids; None takes the configuration's value) is
vLLM's `SamplingParams.allowed_token_ids`: a sequence of token ids for every prompt, or one sequence (or None: no list) per
prompt.  Every logit OUTSIDE a row's list becomes -inf ahead of every sampler; the order is mask -> edit -> temperature ->
top-k -> top-p -> min-p.  An allow-list of 4 tokens bans 152 060, 148 times what the sparse edit holds per row, so this is its
own operation: the host builds one bitmask per DISTINCT list ([R, ceil(V / 32)] int32, bit v & 31 of word v >> 5 set = kept; the
form grammar back ends produce), uploads it once (ops.pack_token_masks; R <= B, a row without a list gets mask_row -1 and is
never touched), and every loop calls ops.logit_mask_rows (asd_logit_mask_rows, in place, a pure write stream) once per logits
tensor, immediately in front of the edit's call at each of its three sites: stage 0's [B, V] logits, every proposal's draft
logits, the target's [B, K+1, V] output before anything is sliced from or scored on it.  Draft and target receive the SAME
mask, so -- the argument of LOGIT EDITS, word for word -- the draft -> verify -> residual chain stays lossless against the
restricted target distribution.  The mask and the sparse edit commute (a masked element stays -inf under a bias, a ban inside
the list is -inf either way); the order is fixed only so that the call pattern is.  Consequences: only listed tokens are
proposed, accepted, drawn or listed; the returned log-probs and top-N tables are those of the RESTRICTED distribution; with
`logprobs` = N and fewer than N allowed tokens the unfillable slots hold id -1 and -inf; a stop id outside a row's list can
never end that row (the caller's choice, as in vLLM).  A call without a list (None everywhere) makes exactly the ops calls it
made before.  ValueError before any launch: a bool, non-integer or out-of-vocabulary id, a mix of ids and lists, a sequence of
the wrong length, an EMPTY list (it allows nothing, and the samplers forbid a row without a finite logit), and a row whose
list minus its banned ids -- permanent bans and the stop ids under min_tokens alike -- is empty.  NOT BUILT: folding the mask into
the samplers, and serving/hierarchy.py's loop.  (Per-position masks -- a grammar's mask differs at each of the K + 1 positions --
are GUIDED DECODING below.)

PENALTIES.  `generate(repetition_penalty=, presence_penalty=, frequency_penalty=)` (or the StageConfig fields of those names; None
takes the configuration's value, which defaults to 1.0 / 0.0 / 0.0) are vLLM's `apply_penalties`, each one value for the call or
one per prompt: repetition_penalty in (0, 2], presence_penalty and frequency_penalty in [-2, 2] (vLLM's and OpenAI's ranges).  They
run behind the allow-list and the sparse edit and ahead of the temperature -- mask -> edit -> penalties -> temperature -> top-k
-> top-p -> min-p, vLLM V1's order (`logit_bias` first, penalties second).  For row b at a position whose history is H -- the
row's real prompt tokens (the left-padding is not history), its committed generated tokens, and the step's proposals in front of
that position -- token v is SEEN when it occurs anywhere in H and c is the number of its occurrences among the generated tokens
and proposals in H (the prompt is not counted).  In f32, in this order, with one rounding to the logits' dtype at the end:
y = x; if seen and rep != 1: y = x / rep where x > 0, else x * rep; if c > 0: y = y - freq * c, then y = y - pres.  -inf stays
-inf (a masked or banned token stays so); a result that would round to +inf (f16 with rep < 1) is stored as the dtype's largest
finite value; an element the penalties do not change is not stored at all.  STATE, allocated once per call and only when some
row has a non-neutral value: `seen`, one bit per (row, token) in the allow-list's bit layout, whose prompt bits are built on the
host from the unpadded prompt ids and uploaded once (ops.pack_penalties); `counts`, int32 [B, V]; the rows' three values; and at
a verifying stage a [B, draft_len] buffer of the step's proposals, whose column k the loop fills after proposal k.  Every loop
calls ops.penalty_rows (asd_penalty_rows, in place) once per logits tensor, immediately behind the edit's call at each of its
three sites: stage 0's [B, V] logits (no proposals); every proposal's draft logits (proposal k sees the proposals 0 .. k - 1 of
the step, which are not committed yet); the target's [B, K+1, V] output before anything is sliced from or scored on it (row j
sees the proposals 0 .. j - 1 -- the history the draft's row j had).  Draft and target so receive the SAME penalty from the
SAME history at every position, and -- the argument of LOGIT EDITS, word for word -- the draft -> verify -> residual chain
stays lossless against the penalised target distribution.  ops.penalty_commit (asd_penalty_commit) follows the step's commit
(and the top-N commit): the step's committed tokens enter `seen` and `counts` on the device.  Rejected proposals were never
written there, so nothing is rolled back; the commit kernels leave n_commit = 0 for a finished row, so its state is frozen.
Consequences: the returned log-probs and top-N tables are those of the PENALISED distribution; greedy decoding takes the
arg-max of the penalised row; the rows route, seeds, the stop and finish routes, edits, masks and `logprobs = N` are untouched
and compose with it.  A call whose rows are all neutral (no keyword, 1.0 / 0.0 / 0.0, sequences of them) makes exactly the ops
calls it made before.  ValueError before any launch and before the prompts are encoded: a bool, a NaN, a value that is no
number or lies outside its range, a sequence of the wrong length or one that holds None.  COST: the kernel scans a row's seen
bits (19 KB at V = 152064) and works per distinct seen token, not per vocabulary entry (profiles/penalties_step.json).  NOT
BUILT: vLLM's `repetition_penalty` over the OUTPUT only (here, as in vLLM, the prompt counts as seen), removing finished rows
from the state, and serving/hierarchy.py's loop.

BAD WORDS.  `generate(bad_words=, bad_words_per_prompt=)` is vLLM's `SamplingParams.bad_words`, on token ids.  `bad_words` (or
StageConfig.bad_words; None takes the configuration's value) is one list for every prompt, `bad_words_per_prompt` holds
len(prompts) lists; an entry is a str -- encoded by the stage's tokenizer and folded into the vocabulary exactly as a stop
string is -- or a sequence of 1..8 integer ids in [0, V).  A row's list is the common list followed by its own, duplicates
dropped (not refused), at most MAX_BAD_WORDS = 256 words afterwards.  `banned_token_ids` is the one-token case, fixed for the
whole call; for a word w_0 .. w_{m-1} WHICH logit is banned depends on what the row has just produced.  Take a logits position
of row b whose history is H: the row's committed GENERATED tokens, tokens[b][P : seq_len[b]] with seq_len as it stands before
the step's commit, and behind them the step's proposals that the position sees.  The prompt and the left-padding are not history
(vLLM also matches over the output only).  Element w_{m-1} becomes -inf when len(H) >= m - 1 and the last m - 1 tokens of H
equal w_0 .. w_{m-2}; a word of one token always bans its token; nothing else is written.  So no row's generated tokens hold
one of its words as a contiguous run.  The words are uploaded once per call (ops.pack_bad_words: two tables in the layout of the
stop sequences; equal rows share one list) and every loop calls ops.bad_words_rows (asd_bad_words_rows, in place) once per
logits tensor at the three sites of the edit: stage 0's [B, V] logits (no proposals); every proposal's draft logits (proposal k
sees the proposals 0 .. k - 1 of the step: K1 = 1, n_prev = k); the target's [B, K+1, V] output before anything is sliced from
or scored on it (n_prev = 0, row j sees the proposals 0 .. j - 1 -- the history the draft's row j had).  The [B, draft_len]
buffer of the step's proposals is ONE buffer of the call, which the penalties read too when both are on.  The order is mask ->
bad words -> edit -> penalties -> temperature, vLLM V1's; the four operations commute on a -inf (a banned element stays -inf
under a bias and under a penalty), and the order is fixed only so that the call pattern is.  Draft and target receive the SAME
ban from the SAME history at every position, so -- the argument of LOGIT EDITS and PENALTIES, word for word -- the draft ->
verify -> residual chain stays lossless against the target distribution with the bad words removed.  A rejected proposal never
reaches `tokens`: nothing is rolled back, and the operation keeps no state -- nothing follows the commit.  Consequences: the
returned log-probs and top-N tables are those of the distribution with the banned tokens removed; greedy decoding takes the
arg-max of what is left; the rows route, seeds, the stop and finish routes, `logprobs = N`, edits, masks and penalties are
untouched and compose with it.  A call whose lists are all empty makes exactly the ops calls it made before.  THE ROW KEEPS A
TOKEN, conservatively, because the match is decided on the device: a row's allow-list minus its banned ids (permanent bans and
the stop ids under min_tokens) minus the LAST ids of all its words must be non-empty; without an allow-list the union of those
ids must be smaller than V.  ValueError before any launch and before the prompts are encoded: a bool, float or out-of-vocabulary
id, an empty word, a word of more than 8 ids, more than 256 distinct words in a row, the wrong number of per-prompt lists, a
str where a list is wanted, a row that would keep no token.  COST: one workgroup per logits row, one lane per word, at most
seven history loads and one store per lane (profiles/bad_words_step.json).  NOT BUILT: vLLM's second variant of every word
with a leading space (SimpleTokenizer has no such variant); and serving/hierarchy.py's loop.  (`no_repeat_ngram_size`, whose
"words" are the n-grams of the row's own history, is the next section: its bans are dynamic, but a position bans at most one
token per n-gram of its history, which the host bounds before the call.)

NO REPEAT N-GRAM.  `generate(no_repeat_ngram_size=)` (or StageConfig.no_repeat_ngram_size; None takes the configuration's value)
is HF generate's `no_repeat_ngram_size` (transformers' NoRepeatNGramLogitsProcessor): an int n in [0, MAX_NGRAM = 8] for every
prompt, or one per prompt; 0 is off.  It is the usual cure for greedy or low-temperature decoding that runs into loops.  A
logits position of row b has the history H = tokens[b][row_start[b] : L] ++ the step's proposals the position sees, with L =
seq_len[b] as it stands before the step's commit: the row's REAL prompt ids (the `real` lists of _encode, so row_start[b] =
P - len(real[b]); the prompt counts as history, as in HF for decoder-only models, the left-padding in front of it does not),
its committed generated tokens, and behind them the step's uncommitted proposals, exactly as for bad words.  For every i in
[0, len(H) - n] with H[i : i+n-1] == H[len(H)-n+1 :] element H[i+n-1] becomes -inf; nothing else is written.  With n = 1 the
compared run is empty and every token of H is banned; with len(H) < n nothing is.  So no n-gram that ends in a row's generated
tokens equals an earlier n-gram of its prompt plus generated tokens.  This is the operation ops.bad_words_rows cannot express:
the "words" are not given by the caller, they are every n-gram of the row's own history, so the kernel scans the history
(asd_no_repeat_ngram_rows: a workgroup per logits row and per slice of 2048 n-gram starts, the last suffix token compared
first).  The rows' n and row_start are uploaded once per call (ops.pack_no_repeat_ngram) and every loop calls
ops.no_repeat_ngram_rows (in place) once per logits tensor at the three sites of bad.apply: stage 0's [B, V] logits (no
proposals); every proposal's draft logits (K1 = 1, n_prev = k); the target's [B, K+1, V] output before anything is sliced from
or scored on it (n_prev = 0).  The proposal buffer is the call's ONE [B, draft_len] buffer, now also allocated when only this
feature is on.  The order is mask -> fsm -> bad words -> n-gram -> edit -> penalties -> temperature; all of them commute on a
-inf, and the place is fixed only so that the call pattern is.  Draft and target receive the SAME ban from the SAME history at
every position, so -- the argument of LOGIT EDITS, word for word -- the draft -> verify -> residual chain stays lossless against
the target distribution with the repeating tokens removed.  The operation keeps no state: a rejected proposal never reaches
`tokens`, nothing follows the commit, nothing is rolled back.  Consequences: the returned log-probs and top-N tables are those of
the restricted distribution; greedy decoding takes the arg-max of what is left; a stop id can be banned like any other token (HF
does the same); everything else is untouched and composes with it.  A call whose every n is 0 makes exactly the ops calls it
made before.  THE ROW KEEPS A TOKEN: the bans are dynamic, but a position bans at most one token per n-gram that starts in its
history, so at most len(H), and no position of row b sees a history longer than bound_b = len(real[b]) + max_tokens_b +
draft_len (0 at stage 0).  With gone_b the set of BAD WORDS' rule (permanent bans, the stop ids under min_tokens, the last ids
of the row's bad words): a row without an allow-list needs |gone_b| + bound_b < V, a row with one |allowed_b - gone_b| >
bound_b.  ValueError before any launch, naming the prompt: a bool, a float, None inside a sequence, the wrong length, a value
outside [0, 8], a row that fails the rule above (raised once the prompts are encoded: the one check that needs their
lengths), and a guided row with n > 0.  COST: profiles/no_repeat_ngram_step.json.  NOT BUILT: n > 0 on a guided row (a state's
allowed set can be one token, which the rule may ban); HF's encoder-decoder variant; and serving/hierarchy.py's loop.

GUIDED DECODING.  `generate(guided_fsm=, guided_choice=, guided_choice_per_prompt=)` (or StageConfig.guided_fsm / guided_choice; a
keyword of None takes the configuration's value) is structured output: a row that must follow a grammar, or be one of a set of
answers (vLLM's `guided_choice`).  The unit is serving/guided.py's `TokenFSM(n_states, start, edges, other=None, accepting=())`, a
deterministic automaton over token ids: edges[s] = {token id: next state} (a next state of -1: the token is forbidden in s),
other[s] = the next state of every token without an edge in s (-1, the default: forbidden), `accepting` = the states in which the
row may end.  `TokenFSM.from_choices(choices)` is the trie of up to 256 choices, each a str (encoded by the stage's tokenizer and
folded into the vocabulary exactly as a stop string is) or a sequence of 1..64 ids, duplicates dropped, a choice's end node
accepting -- an inner node too when one choice is a prefix of another.  `guided_fsm` is one TokenFSM for every prompt or one (or
None) per prompt, `guided_choice` one list of choices for every prompt, `guided_choice_per_prompt` len(prompts) lists (None or
empty: the row is free).  In a speculative step the mask of position j depends on the proposals 0 .. j - 1, which exist only on
the device, so a host-side grammar back end could drive this loop only with a read-back per proposal: the automaton LIVES ON THE
DEVICE.  COMPILATION, per (automaton, row stop set): Z is the row's length-1 stop-list entries -- its stop ids and one-token stop
sequences, which is what grammar back ends do with EOS.  One state END is appended, which allows exactly Z and loops; in an
accepting state every z of Z without an explicit edge leads to END; in a non-accepting state every such z is forbidden, even
under `other`.  Rows with the same automaton and the same Z share one compiled automaton; all of a call's are laid into one
state space (at most MAX_FSM_STATES = 1024 states and 2^20 edges per call) and uploaded once (ops.pack_fsm): CSR edge tables
(state_first, edge_tok ascending, edge_next), state_other, state_bits [S, ceil(V / 32)] in the allow-list's bit layout -- built by
the host from the other tables -- and pos_state [B, ld_state], ld_state = draft_len + 1 at a verifying stage and 1 at stage 0:
column 0 is the state behind the row's committed tokens (the start state at first; -1, never touched, for a free row), column i
the state behind the proposals 0 .. i - 1 of the running step.  THREE OPS.  ops.fsm_mask_rows (asd_fsm_mask_rows, in place, the
allow-list's write stream with a mask index per (row, position) -- one shared kernel body) directly behind the allow-list's call at
each of its three sites: stage 0's [B, V] logits (first = 0); every proposal's draft logits (first = k); the target's [B, K+1, V]
output before anything is sliced from or scored on it (first = 0: row j under column j).  ops.fsm_advance (asd_fsm_advance)
behind every proposal k, once it is drawn and written to the call's proposal buffer -- the ONE [B, draft_len] buffer the bad
words and the penalties read too, allocated when any of the three is on: column k + 1 = delta(column k, proposal k), for every k
including the last, so that column K exists for the bonus row.  ops.fsm_commit (asd_fsm_commit) behind the step's commit, the
top-N commit and penalty_commit: for a row that committed c > 0 tokens, column 0 = delta(column c - 1, the last committed token)
-- ONE transition, because the first c - 1 committed tokens of a step are always its accepted proposals 0 .. c - 2 (stops and
limits cut from the end), so column c - 1 already is the state behind them; a finished row (c = 0) keeps its state.  delta(s, t)
is the edge's next state, else other[s]; where that is -1, or t lies outside the vocabulary -- which cannot happen, every
proposal having been drawn from masked logits -- the state STAYS, so a row never loses its non-empty mask.  The order is mask ->
fsm -> bad words -> n-gram -> edit -> penalties -> temperature; all of them commute on a -inf.  Nothing is read back inside a step.  Draft and
target receive the SAME mask from the SAME history at every position, so -- the argument of LOGIT EDITS, word for word -- the
draft -> verify -> residual chain stays lossless against the grammar-restricted target distribution.  Consequences: the returned
log-probs and top-N tables are those of the RESTRICTED distribution, unfillable top-N slots holding -1 / -inf as with allow-lists;
a guided-choice row ends by "stop" and its generated tokens are exactly one choice followed by one stop id; a row cut by
`max_tokens` ends by "length" holding a prefix of some choice; greedy decoding takes the arg-max of what the state allows; the
rows route, seeds, the stop and finish routes, `logprobs = N`, edits, masks, penalties and bad words are untouched and compose
with it.  A call without a guided row makes exactly the ops calls it made before.  THE ROW KEEPS A TOKEN, conservatively, because
the state lives on the device: for every state reachable from the row's start, the state's allowed set, intersected with the
row's allow-list, minus its permanent bans, minus the last ids of all its bad words, must be non-empty -- which refuses a
non-accepting dead end, and an accepting leaf on a row without a stop id: `guided_choice` needs a stop id on the row.  ValueError
before any launch and before the prompts are encoded: a bool or non-integer id, an id outside the vocabulary, a state out of
range, a str where a list is wanted, an empty choice or one of more than 64 ids, more than 256 choices, the wrong number of
per-prompt entries, a row with both an automaton and choices, more than 1024 states or 2^20 edges in the call, a row that would
not keep a token, and `min_tokens` > 0 on a guided row (below).  COST: 2 * draft_len + 2 extra launches per speculative step
(draft_len + 1 masks, draft_len advances, one commit; 2 per plain step).  Measured at B = 32, K = 8, V = 152064, bf16
(profiles/fsm_step.json), kernel time: the mask 15.7 us on the target's [32, 9, V] output and 4.7 us on one proposal's row, against
16.0 and 4.7 us for asd_logit_mask_rows with an allow-list of the same size in the same run (ratios 0.98 and 1.00, inside the
run-to-run spread: it is the same stream); an advance 2.7 us at a state of 1 edge and 2.9 us at a state of V edges (three search
rounds), a commit 3.1 and 3.4 us; from Python every one of these calls costs the launch cadence, 10 - 11 us.
NOT BUILT: regex- or JSON-schema-to-automaton compilers (a caller hands over the automaton); byte-level grammars; `min_tokens` > 0
on a guided row raises ValueError (its temporary ban of the stop ids can empty an accepting leaf); fusing the advance into the
mask launch; and serving/hierarchy.py's loop.

PROMPT LOG-PROBS.  `generate(prompt_logprobs=N)` (or StageConfig.prompt_logprobs; None takes the configuration's value, and None
there is OFF) is vLLM's `SamplingParams(prompt_logprobs=N)`, OpenAI's `echo` + `logprobs`: the stage's model is scored on the
given text -- the perplexity of a prompt, the log-likelihood of a fixed continuation, "how surprised is this stage by the
request".  N is an int in [0, 8]; 0 is ON and returns the tokens' own log-prob and rank without a table (vLLM's meaning, and the
reason "off" is None and not 0); a bool, a float, a sequence or a value outside the range raises ValueError before the prompts
are encoded.  Both loops run the prefill through forward_ragged, which returns logits for every prompt position; they used to be
dropped.  With the feature on a loop makes ONE ops.prompt_logprobs call (asd_prompt_logprobs: one streaming pass that keeps the
row's log-sum-exp, gathers the logit of the NEXT prompt token, counts the logits that stand ahead of it and, with N >= 1, keeps
asd_top_logprobs' table) directly behind the prefill pass that produced the logits and before the first decode pass (with
graphs enabled the model's output is a buffer that the next replay overwrites): stage 0 on rows [:, :P-1] of its [B, P, V]
result, a verifying stage on the target's whole [B, P-1, V] result, both read where they lie; `target` is the view ids32[:, 1:]
and first[b] = P - (row b's real prompt tokens), so the rows of the left-padding are skipped and cost no pass.  The draft
model's prefill is not scored.  WHAT IS SCORED: the RAW model distribution at temperature 1, ahead of the mask, the automata,
the bad words, the n-gram rule, the edits and the penalties -- vLLM scores prompts on unprocessed logits too, and those
operations describe generated text.  The left-padding is attended (PROMPTS, below), so a short prompt's numbers are conditioned
on the padding in front of it; the longest prompt of a call has none.  Nothing is read back before the loop ends, the generator
is not consumed, and the texts, log-probs and tables of the generated tokens keep their bits; with the feature off a call makes
exactly the ops calls it made before.  RESULTS, with m_i = (row i's real prompt tokens) - 1 and entry j belonging to real prompt
token j + 1 (the first real token has no log-prob, as in vLLM): stats["prompt_token_ids"][i] (int32 [m_i + 1], all real ids),
stats["prompt_logprobs"][i] (float32 [m_i]), stats["prompt_ranks"][i] (int32 [m_i]; 1 = the most likely token, ties by lowest
id: the table's order, so rank <= N means the token stands in slot rank - 1 with the same bits) and, with N >= 1,
stats["prompt_top_token_ids"][i] (int32 [m_i, N]) / stats["prompt_top_logprobs"][i] (float32 [m_i, N]).  Off: none of the keys.
COST: profiles/prompt_logprobs.json.  NOT BUILT: the [B, P, V] prefill logits are materialised as before -- chunking the prefill
over positions is not part of this; one N per request; and serving/hierarchy.py's loop.

TOKEN STATS.  `generate(token_stats=True)` (or StageConfig.token_stats; None takes the configuration's value; anything but None
or a bool raises ValueError before the prompts are encoded) returns, per COMMITTED token, the uncertainty figures the quality
predictor is specified on (RESEARCH_PROTOCOL.md:366-409: the entropy of the last 32 tokens' distributions and the mean of the
per-token maximum log-prob) and vLLM's rank of a sampled token.  A step makes ONE ops.token_stats call (asd_token_stats: the
top-N pass with the committed token's rank counted beside it and a third running sum for the entropy) where the table's call
stands -- behind sampler.draw / sampler.settle, on the tensor the table reads: stage 0's processed [B, V] logits with n_acc = 0
and the drawn token, a verifying stage's processed [B, K+1, V] output as returned with the step's proposals, n_acc and drawn
token -- and one more ops.commit_top_logprobs (N = 2: the pair per row) behind the step's commit, which moves row j to the
step's j-th committed token.  Rows behind n_acc are never committed and are not streamed.  With `logprobs` = N on, that one
call returns the table too (in place of ops.top_logprobs / top_logprobs_rows: the rows are not read again) and the table's
commit is unchanged.  WHAT IS DESCRIBED: the distribution the top-N table describes -- processed (mask -> automaton -> bad
words -> n-gram -> edits -> penalties), temperature-scaled (the call's temperature; 1 when greedy; the row's own on the rows
route) and UNTRUNCATED by top-k / top-p / min-p.  So `token_argmax_ids` / `token_max_logprobs` are table slot 0 with its bits,
rank <= N means the token stands in table slot rank - 1, greedy rows have rank 1, and a sampled token's rank can exceed 1.
Nothing is read back inside a step, the generator is not consumed, and tokens, log-probs and tables keep their bits; with the
feature off a call makes exactly the ops calls it made before.  RESULTS, ragged like logprobs[i]: stats["token_entropy"][i]
(float32 [n_i], nats), stats["token_max_logprobs"][i] (float32 [n_i]), stats["token_argmax_ids"][i] (int32 [n_i]),
stats["token_ranks"][i] (int32 [n_i]) and stats["predictor_features"] (float32 [B, 256]): FeatureExtractor.extract_device on the
[B, cap, 2] device buffer's max log-probs and entropies behind the prompt with n_valid = seq_len - P, the prompt's word count and
the row's token count, formed before anything is read back.  A finished row's entries stay as committed.  Off: none of the keys.
COST (profiles/token_stats.json: B = 32, K1 = 9, V = 152064, bf16, kernel time): every row live, with the table (N = 5) 76.4 us
against 76.6 us for asd_top_logprobs alone (ratio 1.00: the statistics ride on the table's pass) and without it (N = 0) 77.6 us
against 67.3 us for asd_prompt_logprobs at N = 0 (ratio 1.15, more than that pass's run-to-run spread of 0.13); with n_acc
uniform in 0..K 52.9 / 45.1 us; plus one commit launch per step.  NOT BUILT: serving/hierarchy.py's loop; statistics of the
draft model's rows.

ENTROPY CUTS.  `generate(typical_p=, epsilon_cutoff=, eta_cutoff=)` are HF's TypicalLogitsWarper, EpsilonLogitsWarper and
EtaLogitsWarper with min_tokens_to_keep = 1: the truncations that are no threshold on the sorted probabilities, because they
need the row's entropy or its exact probabilities.  Each takes one number for the call or one per prompt; typical_p lies in
[0, 1] and is off at 0 and 1, the other two lie in [0, 1) and are off at 0; None takes the configuration's value:
StageConfig.typical_p / epsilon_cutoff / eta_cutoff are the stage's own draws at stage 0 and the proposals its model makes for
the stage above, target_typical_p / target_epsilon_cutoff / target_eta_cutoff a verifying stage's own distribution -- the rule
of min_p / target_min_p; all default to off.  A row has at most one of the three.  INPUT: p = softmax(x / T) of the row behind
the mask, the automaton, the bad words, the n-gram rule, the edits and the penalties, at the row's temperature (its own on the
rows route) and untruncated; a -inf element carries no mass and stays -inf.  With H = -sum p ln p:
  typical_p = m       d_v = |-ln p_v - H|; d* is the smallest value with sum{p_v : d_v <= d*} >= m; token v is kept iff
                      d_v <= d*.  Every tie at d* is kept; if the mass never reaches m everything is kept; the arg-max MAY be
                      cut, which no other route here can express.
  epsilon_cutoff = e  token v is cut iff p_v < e and x_v < x_max: every token that ties the maximum survives (HF's top-1 clause).
  eta_cutoff = e      the same with min(e, sqrt(e) exp(-H)) in place of e.
A cut token's logit becomes -inf in place; nothing else is written; a row with a NaN element or without a finite one is left as
it is.  It is one more in-place pass of the form of the others (asd_entropy_cut_rows; the rows' {1 / T, mode, value} records are
uploaded once per call and side through ops.pack_entropy_cut), and it runs LAST of them, directly ahead of the draw, propose or
settle call, and so ahead of top.score and stat.score, which read the same tensor: the order is mask -> fsm -> bad words ->
n-gram -> edit -> penalties -> ENTROPY CUT -> temperature -> top-k -> top-p -> min-p.  Top-k, top-p and min-p then act on the
SURVIVORS.  THIS IS NOT HF's ORDER: HF runs Temperature -> TopK -> TopP -> MinP -> Typical -> Epsilon -> Eta; llama.cpp's
default sampler chain places typical ahead of top-p, as this does.  With top-k, top-p and min-p off the kept set is HF's
(tests/test_entropy_cut_ref.py holds the reference to transformers' three classes, and to HF's classes chained in this order).
At a verifying stage the draft rows receive the DRAFT stage's configured cut and the target's [B, K+1, V] output the call's
own, both with the row's temperature; the samplers, the verify, the residual draw and the commit are untouched and only ever
see logits that already carry the cut, so the draft -> verify -> residual chain stays lossless against the cut target
distribution by the argument of LOGIT EDITS.  As with every other pass the returned log-probs, the top-N tables and the token
statistics describe the distribution behind the cut (unfillable table slots hold -1 / -inf, as under an allow-list).  Greedy
decoding ignores all three, as it ignores min-p, and makes no call; a call whose every row is off makes exactly the ops calls it
made before.  ValueError before any launch and before the prompts are encoded: a bool, a NaN, a value outside its range, the
wrong length, two of the three on one row (NOT BUILT: HF applies them in sequence).  COST (profiles/entropy_cut.json: B = 32, K1 = 9,
V = 152064, bf16, kernel time): epsilon mode 63.2 us and typical mode 175.0 us against 62.4 us for asd_token_stats with N = 0 on the
same tensor (ratios 1.01, inside that pass's run-to-run spread of 0.10, and 2.81).  NOT
BUILT beside that: per-request values of the DRAFT side, and serving/hierarchy.py's loop.

PROMPTS.  `SimpleTokenizer` ids (folded into the model's vocabulary); each prompt keeps its LAST P ids, where P is the longest
encoded prompt of the call, capped by `StageConfig.max_prompt_tokens` and at least 2; shorter prompts are LEFT-padded with id 0.
The synthetic models have no attention mask, so the padding is attended like any other token: that is this build's choice, not
the reference's (whose engines mask it).
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from ..distributed import HipOps
from ..kernels import pack_stop_sequences
from ..minimal_adaptive_decoder import SimpleTokenizer
from .stage_args import (MAX_BAD_WORD_LEN, MAX_BAD_WORDS, MAX_LOGIT_EDITS, MAX_NGRAM, MAX_STOP_SEQ_LEN, MAX_STOP_SEQS,  # noqa: F401
                         _check_logprobs, _check_min_p, _check_prompt_logprobs, _check_stop_ids, _check_stop_sequences, _check_token_stats,
                         _is_seq,
                         check_allowed_token_ids, check_bad_words, check_banned_token_ids, check_frequency_penalty, check_guided, check_logit_bias, check_max_tokens, check_min_tokens, check_ngram_rows_keep_a_token, check_no_repeat_ngram_size, check_per_prompt,
                         check_entropy_cuts, check_presence_penalty, check_repetition_penalty, check_rows_keep_a_token, check_seeds, merge_logit_edits)
from .guided import MAX_FSM_EDGES, MAX_FSM_STATES, CompiledFsm, TokenFSM, check_guided_rows_keep_a_token, compile_rows  # noqa: F401
from .synthetic_lm import QWEN25_SHAPES, LMShape, SyntheticLM

# reference stage label -> the Qwen2.5 shape this build runs in its place (configs/models.yaml names the tiers by size)
_DEFAULT_SHAPES = {"8b": "7b", "13b": "14b", "34b": "32b", "70b": "72b"}


@dataclass
class StageConfig:
    # -- the reference's fields (server.py:151-158)
    model_name: str = "synthetic"
    model_size: str = "8b"                   # the stage's name: StageManager.get_stage(model_size)
    tensor_parallel_size: int = 1            # recorded only (multi-rank stages are out of scope)
    gpu_memory_utilization: float = 0.8      # recorded only
    quantized: bool = False                  # recorded only
    cost_per_token: float = 1.0
    # -- build extensions
    shape: Optional[LMShape] = None          # None: QWEN25_SHAPES by model_size
    dtype: torch.dtype = torch.bfloat16
    model_seed: int = 0
    logit_scale: float = 1.0
    max_prompt_tokens: int = 256
    # sampling: the reference's settings for the DRAFT side (temperature comes with the call), off for the TARGET side, as in
    # serving/hierarchy.py HierarchyConfig.  Stage 0 draws with (top_k, top_p); a verifying stage drafts with the stage
    # below's model under ITS OWN (top_k, top_p) and verifies / commits against (target_top_k, target_top_p).
    top_p: float = 0.9
    top_k: int = 0
    target_top_p: float = 1.0
    target_top_k: int = 0
    min_p: float = 0.0                       # min-p of the stage's own draws, behind (top_k, top_p); 0: off (module docstring)
    target_min_p: float = 0.0                # min-p of a verifying stage's own distribution, behind (target_top_k, target_top_p)
    # the entropy cuts (module docstring, ENTROPY CUTS), by the rule of min_p / target_min_p; at most one of the three per side
    typical_p: float = 1.0                   # HF's typical_p of the stage's own draws and of its proposals; 0 and 1: off
    epsilon_cutoff: float = 0.0              # HF's epsilon_cutoff of the same rows; 0: off
    eta_cutoff: float = 0.0                  # HF's eta_cutoff of the same rows; 0: off
    target_typical_p: float = 1.0            # the three of a verifying stage's own distribution
    target_epsilon_cutoff: float = 0.0
    target_eta_cutoff: float = 0.0
    draft_len: int = 8
    seed: int = 0
    sync_every: int = 4
    stop_token_ids: Sequence[int] = ()       # EOS ids: a sequence ends behind the first committed one (module docstring)
    logprobs: int = 0                        # top-N log-probs per committed token, 0..8 (0: off; module docstring)
    stop_sequences: Sequence = ()            # stop strings / token-id sequences of every prompt (module docstring, HOW A ROW ENDS)
    logit_bias: Optional[Dict[int, float]] = None    # {token id: bias in raw logit units} (module docstring, LOGIT EDITS)
    banned_token_ids: Sequence[int] = ()     # token ids that are never proposed, accepted or drawn
    min_tokens: int = 0                      # the stop ids are banned until a row has generated this many tokens
    allowed_token_ids: Optional[Sequence[int]] = None    # the only token ids a row may hold (module docstring, ALLOW-LISTS)
    repetition_penalty: float = 1.0          # in (0, 2]; 1: off (module docstring, PENALTIES)
    presence_penalty: float = 0.0            # in [-2, 2]; 0: off
    frequency_penalty: float = 0.0           # in [-2, 2]; 0: off
    bad_words: Sequence = ()                 # words (strings / sequences of 1..8 token ids) no row may produce (module docstring, BAD WORDS)
    no_repeat_ngram_size: int = 0            # in [0, 8]; 0: off (module docstring, NO REPEAT N-GRAM)
    guided_fsm: Optional[TokenFSM] = None    # the automaton every row follows (module docstring, GUIDED DECODING)
    guided_choice: Optional[Sequence] = None  # the choices (strings / sequences of 1..64 token ids) every row picks one of
    prompt_logprobs: Optional[int] = None    # None: off; 0..8: the prompt tokens' log-probs and ranks, and a top-N table (PROMPT LOG-PROBS)
    token_stats: bool = False                # per committed token: entropy, max log-prob, arg-max and rank; the predictor's features (TOKEN STATS)


_REASONS = {1: "stop", 2: "length"}


class _Plan(NamedTuple):
    """One generate call, checked and defaulted by Stage._plan before anything is launched or encoded: what _CallState and the
    two loops are built from.  Nothing here lives on the device."""
    prompts: Tuple[str, ...]
    limits: Tuple[int, ...]                  # every row's max_tokens
    max_tokens: int                          # the largest of them: the size of the buffers
    greedy: bool
    inv_t: float                             # float32(1 / temperature); 1 when greedy; the first row's on the rows route
    scalars: Optional[Tuple[int, float, float]]     # the stage's own (top_k, top_p, min_p); None: greedy, or the rows route
    rows: Optional[Tuple[list, list, list, list]]   # the rows route: every row's inv_t, top_k, top_p, min_p
    stop: Tuple[int, ...]                    # the stop ids
    row_seqs: List[list]                     # every row's stop list: the stop ids as length-1 sequences, the common ones, its own
    finish_route: bool                       # asd_commit_step_finish: only for what the stop-id route cannot do
    edit_rows: list                          # every row's merged (id, bias, until) entries
    mask_rows: list                          # every row's allow-list: a sorted tuple of ids, or None
    bad_rows: list                           # every row's bad words: distinct tuples of 1..8 ids
    ngram_rows: list                         # every row's no_repeat_ngram_size in [0, 8]; 0: off
    penalties: Optional[Tuple[list, list, list]]    # every row's repetition, presence and frequency penalty; None: all neutral
    fsm: Optional[CompiledFsm]               # the rows' guided automata in one state space (host arrays); None: no row is guided
    seeds: Optional[List[int]]
    n_top: int
    n_prompt: Optional[int] = None           # prompt_logprobs: None off, else the table's N in [0, 8]
    token_stats: bool = False                # the per-token statistics and the predictor's feature batch (TOKEN STATS)
    cut_rows: Optional[list] = None          # every row's (mode, value) of the stage's own entropy cut; None: every row off
    cut_draft_rows: Optional[list] = None    # a verifying stage: every row's (mode, value) of the draft stage's configured cut


class _EditState:
    """What a generate call with logit edits keeps: the merged entries on the device (uploaded once) and the prompt length;
    `apply` is the loops' one call per logits tensor (module docstring, LOGIT EDITS)."""

    def __init__(self, ops, rows, P: int, device):
        self.ops, self.start = ops, int(P)
        self.packed = ops.pack_logit_edits(rows, device)

    def apply(self, logits: torch.Tensor, seq_len: torch.Tensor, offset: int = 0) -> torch.Tensor:
        """logits [B, V] or [B, K+1, V], edited in place; seq_len: the step's lengths before its commit."""
        return self.ops.logit_edit_rows(logits, self.packed, seq_len, self.start, offset)


class _MaskState:
    """What a generate call with an allow-list keeps: the rows' bitmasks on the device (uploaded once; equal lists share one);
    `apply` is the loops' one call per logits tensor, in front of the edit's (module docstring, ALLOW-LISTS)."""

    def __init__(self, ops, rows, V: int, device):
        self.ops = ops
        self.packed = ops.pack_token_masks(rows, int(V), device)

    def apply(self, logits: torch.Tensor) -> torch.Tensor:
        """logits [B, V] or [B, K+1, V], masked in place."""
        return self.ops.logit_mask_rows(logits, self.packed)


class _BadWordState:
    """What a generate call with bad words keeps: the rows' word tables on the device (uploaded once; equal lists share one),
    the prompt length, the size of the token buffer and, at a verifying stage, the call's [B, draft_len] buffer of the step's
    proposals.  `apply` is the loops' one call per logits tensor, behind the mask's and in front of the edit's; nothing follows
    the commit: the operation reads `tokens` and keeps no state (module docstring, BAD WORDS)."""

    def __init__(self, ops, rows, P: int, cap: int, step_tok: Optional[torch.Tensor], device):
        self.ops, self.start, self.cap, self.step_tok = ops, int(P), int(cap), step_tok
        self.packed = ops.pack_bad_words(rows, device)

    def apply(self, logits: torch.Tensor, tokens: torch.Tensor, seq_len: torch.Tensor, n_prev: int = 0) -> torch.Tensor:
        """logits [B, V] or [B, K+1, V], banned in place; seq_len: the step's lengths before its commit; position j sees the
        step's first n_prev + j proposals behind the row's committed tokens."""
        if self.step_tok is None:
            return self.ops.bad_words_rows(logits, self.packed, tokens, seq_len, self.start, self.cap)
        return self.ops.bad_words_rows(logits, self.packed, tokens, seq_len, self.start, self.cap, self.step_tok, n_prev)


class _NgramState:
    """What a generate call with a no_repeat_ngram_size keeps: the rows' n and the index of their first real prompt id on the
    device (uploaded once), the size of the token buffer and, at a verifying stage, the call's [B, draft_len] buffer of the
    step's proposals.  `apply` is the loops' one call per logits tensor, behind the bad words' and in front of the edit's;
    nothing follows the commit: the operation reads `tokens` and keeps no state (module docstring, NO REPEAT N-GRAM)."""

    def __init__(self, ops, ns, prompt_ids, P: int, cap: int, step_tok: Optional[torch.Tensor], device):
        self.ops, self.cap, self.step_tok = ops, int(cap), step_tok
        self.packed = ops.pack_no_repeat_ngram(ns, [len(r) for r in prompt_ids], int(P), device)

    def apply(self, logits: torch.Tensor, tokens: torch.Tensor, seq_len: torch.Tensor, n_prev: int = 0) -> torch.Tensor:
        """logits [B, V] or [B, K+1, V], banned in place; seq_len: the step's lengths before its commit; position j sees the
        step's first n_prev + j proposals behind the row's prompt and committed tokens."""
        if self.step_tok is None:
            return self.ops.no_repeat_ngram_rows(logits, self.packed, tokens, seq_len, self.cap)
        return self.ops.no_repeat_ngram_rows(logits, self.packed, tokens, seq_len, self.cap, self.step_tok, n_prev)


class _CutState:
    """What a generate call with an entropy cut keeps for one side (its own rows, or a verifying stage's draft rows): the
    rows' {1 / temperature, mode, value} records on the device, uploaded once.  `apply` is the loops' one call per logits
    tensor, the last one ahead of the draw, propose or settle call (module docstring, ENTROPY CUTS)."""

    def __init__(self, ops, rows, inv_t: List[float], device):
        self.ops = ops
        self.packed = ops.pack_entropy_cut(inv_t, [m for m, _ in rows], [v for _, v in rows], device)

    def apply(self, logits: torch.Tensor, keep: bool = False) -> Optional[torch.Tensor]:
        """logits [B, V] or [B, K+1, V], cut in place.  keep: the tests' record -- a clone of the tensor as it entered."""
        entered = logits.clone() if keep else None
        self.ops.entropy_cut_rows(logits, self.packed)
        return entered


class _FsmState:
    """What a generate call with a guided row keeps: the call's automata and the rows' state columns on the device (uploaded
    once; rows with the same automaton and stop ids share one), and at a verifying stage the call's [B, draft_len] buffer of the
    step's proposals (shared with _BadWordState, _NgramState and _PenaltyState).  `apply` is the loops' one call per logits tensor, directly
    behind the allow-list's; `advance` follows proposal k; `commit` follows the step's commit (module docstring, GUIDED
    DECODING)."""

    def __init__(self, ops, fsm: CompiledFsm, ld_state: int, step_tok: Optional[torch.Tensor], device):
        self.ops, self.step_tok = ops, step_tok
        self.packed = ops.pack_fsm(fsm, int(ld_state), device)

    def apply(self, logits: torch.Tensor, first: int = 0) -> torch.Tensor:
        """logits [B, V] or [B, K+1, V], masked in place: position j by the state behind the step's first `first` + j proposals."""
        return self.ops.fsm_mask_rows(logits, self.packed, first)

    def advance(self, k: int) -> None:
        """Behind proposal k, which the loop has written to column k of the proposal buffer."""
        self.ops.fsm_advance(self.packed, self.step_tok, k)

    def commit(self, tokens: torch.Tensor, seq_len: torch.Tensor, n_commit: torch.Tensor, cap: int) -> None:
        """Behind the step's commit, which left seq_len and n_commit (0 for a finished row: its state stays)."""
        self.ops.fsm_commit(self.packed, tokens, seq_len, n_commit, cap)


class _PenaltyState:
    """What a generate call with a non-neutral penalty keeps: the rows' seen bits, counts and parameters on the device (the
    prompt's bits uploaded once) and, at a verifying stage, the call's [B, draft_len] buffer of the step's proposals (shared
    with _BadWordState; the loop fills column k after proposal k).  `apply` is the loops' one call per logits tensor, behind
    the edit's; `commit` follows the step's commit (module docstring, PENALTIES)."""

    def __init__(self, ops, penalties, prompt_ids, V: int, step_tok: Optional[torch.Tensor], device):
        self.ops, self.step_tok = ops, step_tok
        self.packed = ops.pack_penalties(*penalties, prompt_ids, int(V), device)

    def apply(self, logits: torch.Tensor, n_prev: int = 0) -> torch.Tensor:
        """logits [B, V] or [B, K+1, V], penalised in place; position j sees the step's first n_prev + j proposals."""
        if self.step_tok is None:
            return self.ops.penalty_rows(logits, self.packed)
        return self.ops.penalty_rows(logits, self.packed, self.step_tok, n_prev)

    def commit(self, tokens: torch.Tensor, seq_len: torch.Tensor, n_commit: torch.Tensor, cap: int) -> None:
        """Behind the step's commit, which left seq_len and n_commit (0 for a finished row: its state stays)."""
        self.ops.penalty_commit(tokens, seq_len, n_commit, self.packed, cap)


# ---------------------------------------------------------------------------------------------- how a call's rows end
# One interface for the three commit kernels: commit(tok, lp_tok, n_acc, drawn, lp_drawn, seq_len, tokens, lps, n_commit, cap)
# is the step's commit, done(seq_len, cap) makes the loop's ONE host read, outcome(...) names every row's end for `stats`.
class _RunToLimit:
    """No stop set: asd_commit_step_lp; every row returns exactly max_tokens tokens.  `stops` is False: stage 0 then never
    calls done() -- it knows every position on the host -- and a verifying stage reads min(seq_len)."""
    stops = False

    def __init__(self, ops):
        self.commit = ops.commit_step_lp

    def done(self, seq_len: torch.Tensor, cap: int) -> bool:
        return int(seq_len.min().item()) >= cap

    def outcome(self, seq_len, tok_h, P: int, limits):
        return list(limits), ["length"] * len(limits), [None] * len(limits)


class _Stops:
    """What the two stopping routes keep beside seq_len: the per-sequence finished flag (1 stop, 2 length) and the counter of
    finished sequences their commit kernels maintain -- the ONE int32 the host reads."""
    stops = True

    def __init__(self, ops, B: int, device):
        self.ops, self.B = ops, B
        self.finished = torch.zeros((B,), dtype=torch.int32, device=device)
        self.n_finished = torch.zeros((1,), dtype=torch.int32, device=device)

    def done(self, seq_len: torch.Tensor, cap: int) -> bool:
        return int(self.n_finished.item()) == self.B

    def outcome(self, seq_len, tok_h, P: int, limits):
        n_tok = [int(n) - P for n in seq_len.cpu().tolist()]
        flags = self.finished.cpu().tolist()
        if any(f not in _REASONS for f in flags) or any(not 1 <= n <= lim for n, lim in zip(n_tok, limits)):
            raise RuntimeError("stage loop ended with an unfinished sequence")
        return n_tok, [_REASONS[f] for f in flags], self._matches(flags, tok_h, n_tok)


class _StopIds(_Stops):
    """A stop set: asd_commit_step_stop, the ids on the device (uploaded once)."""

    def __init__(self, ops, stop_ids: Sequence[int], B: int, device):
        super().__init__(ops, B, device)
        self.stop_ids = torch.tensor(list(stop_ids), dtype=torch.int32, device=device)

    def commit(self, *step) -> None:
        self.ops.commit_step_stop(*step, self.stop_ids, self.finished, self.n_finished)

    def _matches(self, flags, tok_h, n_tok):
        return [(int(tok_h[b, n_tok[b] - 1]),) if f == 1 else None for b, f in enumerate(flags)]


class _StopSequences(_Stops):
    """Unequal limits or multi-token stop sequences: asd_commit_step_finish.  Every row's list of stop sequences (the stop ids
    as length-1 sequences first) and its own length limit on the device, uploaded once, and beside the flag and the counter
    the index of the sequence that ended each row."""

    def __init__(self, ops, row_seqs: List[List[Tuple[int, ...]]], limits: Sequence[int], P: int, device):
        super().__init__(ops, len(row_seqs), device)
        self.rows, self.start = row_seqs, int(P)
        self.seq_tok = self.seq_n = self.row_first = self.row_max_len = None
        if any(row_seqs):
            shared = all(r == row_seqs[0] for r in row_seqs)             # one list for every row: no row_first
            self.seq_tok, self.seq_n, self.row_first = pack_stop_sequences(row_seqs[0] if shared else row_seqs, device, shared)
        if len(set(limits)) > 1:
            self.row_max_len = torch.tensor([P + int(n) for n in limits], dtype=torch.int32, device=device)
        self.matched = torch.full((self.B,), -1, dtype=torch.int32, device=device)

    def commit(self, *step) -> None:
        self.ops.commit_step_finish(*step, self.start, self.seq_tok, self.seq_n, self.row_first, self.row_max_len, self.finished,
                                    self.n_finished, self.matched)

    def _matches(self, flags, tok_h, n_tok):
        which = self.matched.cpu().tolist()
        return [self.rows[b][which[b]] if f == 1 else None for b, f in enumerate(flags)]


class _TopState:
    """What a generate call with logprobs = n > 0 keeps beside the token buffer: the [B, cap, n] tables the commit fills
    (positions count from the start of the row, prompt included, like `tokens`) and the step's two calls."""

    def __init__(self, ops, n: int, inv_t: float, B: int, cap: int, device, rows=None):
        self.ops, self.n, self.inv_t, self.cap = ops, n, inv_t, cap
        self.rows = rows                                 # the rows route: the `own` table (every row's own temperature)
        self.ids = torch.full((B, cap, n), -1, dtype=torch.int32, device=device)
        self.lps = torch.full((B, cap, n), float("-inf"), dtype=torch.float32, device=device)
        self.step = None

    def score(self, logits: torch.Tensor) -> None:
        """logits: the rows the step commits from, [B, V] or [B, K+1, V], read where they are."""
        self.step = self.ops.top_logprobs(logits, self.n, self.inv_t) if self.rows is None else \
            self.ops.top_logprobs_rows(logits, self.n, self.rows)

    def commit(self, seq_len: torch.Tensor, n_commit: torch.Tensor) -> None:
        """Behind the step's commit, which left seq_len and n_commit."""
        self.ops.commit_top_logprobs(self.step[0], self.step[1], seq_len, n_commit, self.ids, self.lps, self.cap)

    def record(self) -> dict:
        return dict(top_id=self.step[0].clone(), top_lp=self.step[1].clone())


class _StatsState:
    """What a generate call with token_stats on keeps beside the token buffer (module docstring, TOKEN STATS): [B, cap, 2] buffers
    -- int32 (rank, arg-max id), filled with (0, -1), and float32 (entropy, max log-prob), filled with NaN -- that the commit
    fills like the top-N tables, and the step's two calls.  With a table on (`top`), the step's ONE ops.token_stats call
    returns the table too and hands it to `top`, whose commit then moves it: the rows are not read a second time."""

    def __init__(self, ops, top: Optional[_TopState], inv_t: float, B: int, cap: int, device, rows=None):
        self.ops, self.top, self.inv_t, self.cap, self.rows = ops, top, inv_t, cap, rows
        self.ids = torch.zeros((B, cap, 2), dtype=torch.int32, device=device)
        self.ids[:, :, 1] = -1
        self.vals = torch.full((B, cap, 2), float("nan"), dtype=torch.float32, device=device)
        self.step = self.given = None

    def score(self, logits: torch.Tensor, tok32, n_acc: torch.Tensor, drawn: torch.Tensor) -> None:
        """logits: the rows the step commits from, [B, V] (tok32 None) or [B, K+1, V], read where they are; n_acc / drawn: what
        the step's draw or verification left, which the commit reads too."""
        out = self.ops.token_stats(logits, tok32, n_acc, drawn, n=0 if self.top is None else self.top.n,
                                   inv_temperature=self.inv_t, rows=self.rows)
        self.step, self.given = out[:2], (n_acc, drawn)
        if self.top is not None:
            self.top.step = out[2:]

    def commit(self, seq_len: torch.Tensor, n_commit: torch.Tensor) -> None:
        """Behind the step's commit: row j goes to the step's j-th committed token (N = 2: the pair per row)."""
        self.ops.commit_top_logprobs(self.step[0], self.step[1], seq_len, n_commit, self.ids, self.vals, self.cap)

    def record(self) -> dict:
        return dict(stat_id=self.step[0].clone(), stat_val=self.step[1].clone(), n_acc=self.given[0].clone(),
                    drawn=self.given[1].clone())

    def features(self, P: int, seq_len: torch.Tensor, prompts: Sequence[str], stage_id: int) -> torch.Tensor:
        """The predictor's [B, 256] batch (FeatureExtractor.extract_device) from the committed figures, on the device."""
        from .components import FeatureExtractor
        n_valid = seq_len.to(torch.int64) - P
        return FeatureExtractor.extract_device(self.vals[:, P:, 1], self.vals[:, P:, 0], [len(p.split()) for p in prompts],
                                               n_valid.to(torch.float64), stage_id, n_valid=n_valid)

    def stats(self, P: int, n_tok, features: torch.Tensor) -> dict:
        ids, vals = self.ids[:, P:].cpu().numpy(), self.vals[:, P:].cpu().numpy()
        cut = lambda a, k: [np.ascontiguousarray(r[:n, k]) for r, n in zip(a, n_tok)]        # noqa: E731
        return {"token_entropy": cut(vals, 0), "token_max_logprobs": cut(vals, 1), "token_argmax_ids": cut(ids, 1),
                "token_ranks": cut(ids, 0), "predictor_features": features.cpu().numpy()}


class _PromptState:
    """What a generate call with prompt_logprobs = n keeps (module docstring, PROMPT LOG-PROBS): the scored tokens -- the view
    ids32[:, 1:], row t scores prompt position t + 1 -- and every row's first scored position on the device, uploaded once.
    `score` is the loops' ONE call, directly behind the prefill pass whose logits it reads; `stats` reads back after the loop."""

    def __init__(self, ops, n: int, ids: torch.Tensor, prompt_ids: List[List[int]]):
        P = ids.shape[1]
        self.ops, self.n, self.P = ops, int(n), P
        self.real = prompt_ids
        self.target = ids.to(torch.int32)[:, 1:]
        self.first = torch.tensor([P - len(r) for r in prompt_ids], dtype=torch.int32).to(ids.device)
        self.out = None

    def score(self, logits: torch.Tensor, keep: bool = False) -> Optional[dict]:
        """logits: the prefill's rows 0 .. P - 2, [B, P - 1, V], read where they lie (a view; possibly a buffer that the next
        pass overwrites, so this runs before it).  keep: the tests' record."""
        self.out = self.ops.prompt_logprobs(logits, self.target, self.first, self.n)
        return dict(logits=logits.clone(), target=self.target.clone(), first=self.first.clone()) if keep else None

    def stats(self) -> dict:
        """Entry j of row i belongs to its real prompt token j + 1; the first real token has no log-prob."""
        lp, rank, top_id, top_lp = (None if t is None else t.cpu().numpy() for t in self.out)
        m = [max(len(r) - 1, 0) for r in self.real]
        tail = lambda a, i: np.ascontiguousarray(a[i, self.P - 1 - m[i]:])             # noqa: E731
        rows = range(len(m))
        out = {"prompt_token_ids": [np.asarray(r, dtype=np.int32) for r in self.real],
               "prompt_logprobs": [tail(lp, i).astype(np.float32, copy=False) for i in rows],
               "prompt_ranks": [tail(rank, i).astype(np.int32, copy=False) for i in rows]}
        if self.n:
            out["prompt_top_token_ids"] = [tail(top_id, i) for i in rows]
            out["prompt_top_logprobs"] = [tail(top_lp, i) for i in rows]
        return out


# ---------------------------------------------------------------------------------------------- what a step draws with
# What differs between greedy and sampled decoding, behind one interface; the loops hold everything else.
#   draw(logits, step)   stage 0's step -> (n_acc, tok, lp) for the commit
#   start(step)          the top of a verifying step: a seeded call's one step_uniforms launch
#   propose(dl, k)       proposal k of a verifying step from the draft's logits -> tok
#   settle(t_out, tok32) the target's [B, K+1, V] output against the K proposals -> (lp_t, n_acc, drawn, lp_drawn)
# `dense`: the step reads (and edits) a contiguous copy of the logits, not the tensor the model left; kept(seq_len): the step's
# record for Stage.step_inputs, taken before the commit and only when the stage keeps them.
def _clones(**kept) -> dict:
    return {k: None if v is None else v.clone() for k, v in kept.items()}


class _Greedy:
    """temperature 0: ops.verify_greedy (K = 0 on [B, V] logits, one call on the target's output) on the tensors WHERE THEY LIE
    -- no uniforms, no generator use, no score / bonus / draft-row copies, no kept draft logits.  A draft token is accepted iff
    it is the target row's arg-max and the token behind the accepted prefix is the arg-max of the next row, so the text is the
    target's own greedy continuation; log-probs are the model's at temperature 1."""
    dense = False

    def __init__(self, ops):
        self.ops = ops

    def start(self, step: int) -> None:
        pass

    def draw(self, logits, step: int):
        self.read = logits, None
        out = self.out = self.ops.verify_greedy(logits, None, 1.0)
        return out[1], out[2], out[3]

    def propose(self, dl, k: int):
        return self.ops.verify_greedy(dl, None, 1.0)[2]

    def settle(self, t_out, tok32):
        self.read = t_out, tok32
        out = self.out = self.ops.verify_greedy(t_out, tok32, 1.0)
        return out[:4]

    def kept(self, seq_len) -> dict:
        names = ("logits", "tok", "lp_t", "n_acc", "drawn", "lp_drawn", "argmax", "lp_argmax")
        return _clones(**dict(zip(names, (*self.read, *self.out))), seq_len=seq_len)


class _Sampled:
    """temperature > 0 with one (top_k, top_p, min_p) for the call.  Owns the uniforms -- torch.rand on the stage's generator:
    stage 0 once per step; a verifying step draft_len times (B,), then (B, draft_len), then (B,), in that order; or, seeded, the
    slots of the step's ONE ops.step_uniforms launch and no torch.rand -- the dispatch over the draft_sample* / verify_accept*
    ops, the residual draw and the dense copies it needs (score, bonus, the K edited draft rows)."""
    dense = True

    def __init__(self, stage: "Stage", plan: _Plan, B: int, device):
        self.ops, self.gen, self.inv_t, self.stage = stage.ops, stage.gen, plan.inv_t, stage.index
        self.K = 0 if stage.draft is None else stage.config.draft_len
        self.seeds = None
        if plan.seeds is not None:               # uploaded once (two's-complement wrap above 2^63 - 1), with the one buffer every
            wrapped = [s - 2 ** 64 if s >= 2 ** 63 else s for s in plan.seeds]           # step's uniforms are written to
            self.seeds = torch.tensor(wrapped, dtype=torch.int64, device=device)
            self.buf = torch.empty(((2 * max(self.K, 1) + 1) * B,), dtype=torch.float32, device=device)
        self.own = plan.scalars
        # the proposals: stage 0's are its own draws; a verifying stage's come from the DRAFT stage's configured truncation
        dcfg = None if stage.draft is None else stage.draft.config
        self.prop = plan.scalars if dcfg is None else (dcfg.top_k, dcfg.top_p, dcfg.min_p)
        self.none_accepted = torch.zeros((B,), dtype=torch.int32, device=device) if dcfg is None else None
        self.rd = self.u = self.r = None         # a seeded call: the step's uniforms (start)

    def _uniforms(self, step: int, k_draft: int, k_accept: int, commit: bool):
        """-> (r_draft [k_draft, B] | None, u [B, k_accept] | None, r_commit [B] | None), valid until the next step."""
        return self.ops.step_uniforms(self.seeds, step, self.stage, k_draft, k_accept, commit=commit, out=self.buf)

    def start(self, step: int) -> None:
        if self.seeds is not None:               # ONE launch for every uniform of the step
            self.rd, self.u, self.r = self._uniforms(step, self.K, self.K, True)
        self.lpd, self.thrs, self.dls = [], [], []

    def draw(self, logits, step: int):
        if self.seeds is not None:               # stage 0's one uniform, behind the edit as it always was
            self.rd = self._uniforms(step, 1, 0, False)[0]
        r = torch.rand((logits.shape[0],), generator=self.gen, device=logits.device) if self.rd is None else self.rd[0]
        tok, lp, thr = self._draft_op(logits, r)         # (tok i32, log q(tok), threshold)
        self.last = (logits, tok, lp, thr, r)
        return self.none_accepted, tok, lp

    def propose(self, dl, k: int):
        r = torch.rand((dl.shape[0],), generator=self.gen, device=dl.device) if self.rd is None else self.rd[k]
        tok, lp, thr = self._draft_op(dl, r)
        self.lpd.append(lp)
        self.thrs.append(thr)
        self.dls.append(dl)                      # kept (edited) for the residual distribution at a rejection
        return tok

    def settle(self, t_out, tok32):
        B, Kd = tok32.shape
        lp_d = torch.stack(self.lpd, 1).contiguous()
        d_thr = torch.stack(self.thrs, 1).contiguous()
        score = t_out[:, :Kd].contiguous()
        bonus = t_out[:, Kd].contiguous()
        u = torch.rand((B, Kd), generator=self.gen, device=t_out.device) if self.seeds is None else self.u
        lp_t, n_acc, t_thr = self._verify_op(score, tok32, lp_d, u)
        r = torch.rand((B,), generator=self.gen, device=t_out.device) if self.seeds is None else self.r
        d_rows = torch.stack(self.dls, 1).to(score.dtype).contiguous()
        drawn, lp_drawn = self._residual_op(score, d_rows, n_acc, r, bonus, d_thr, t_thr)
        self.last = (score, bonus, tok32, lp_d, u, lp_t, n_acc, drawn, lp_drawn, t_thr)
        return lp_t, n_acc, drawn, lp_drawn

    def kept(self, seq_len) -> dict:
        seeded = self.rd is not None             # only a seeded call records the uniforms it was handed
        if self.K:
            names = ("logits", "bonus", "tok", "lp_d", "u", "lp_t", "n_acc", "drawn", "lp_drawn", "t_thr")
            last = dict(zip(names, self.last), seq_len=seq_len)
            if seeded:
                last.update(r_draft=self.rd, r_commit=self.r)
        else:
            last = dict(zip(("logits", "drawn", "lp_drawn", "thr"), self.last))
            if seeded:
                last.update(r_draft=self.last[-1][None])
        return _clones(**last)

    # ---- the ops of the call's one (top_k, top_p, min_p); positional and keyword arguments exactly as the ops' twins and
    # recorders expect them (the uniforms by position, `min_p` only where min-p is on)
    def _draft_op(self, logits, r):
        top_k, top_p, min_p = self.prop
        if min_p > 0.0:
            return self.ops.draft_sample_min_p(logits, r, self.inv_t, top_k=top_k, top_p=top_p, min_p=min_p)
        if top_k > 0:
            return self.ops.draft_sample_top_k(logits, r, self.inv_t, top_k=top_k, top_p=top_p)
        return self.ops.draft_sample(logits, r, self.inv_t, top_p)

    def _verify_op(self, score, tok32, lp_d, u):
        """-> (lp_t, n_acc, t_threshold or None) against the target's Temperature -> (TopK ->) (TopP) (-> MinP) distribution."""
        top_k, top_p, min_p = self.own
        if min_p > 0.0:
            out = self.ops.verify_accept_min_p(score, tok32, lp_d, u, self.inv_t, top_k=top_k, top_p=top_p, min_p=min_p)
        elif top_k > 0:
            out = self.ops.verify_accept_top_k(score, tok32, lp_d, u, self.inv_t, top_k=top_k, top_p=top_p)
        elif 0.0 < top_p < 1.0:
            out = self.ops.verify_accept_top_p(score, tok32, lp_d, u, self.inv_t, top_p=top_p)
        else:                                    # (nothing truncates: no threshold)
            out = (*self.ops.verify_accept(score, tok32, lp_d, u, self.inv_t), None)
        return out[0], out[2], out[4]

    def _residual_op(self, score, d_rows, n_acc, r, bonus, d_thr, t_thr):
        top_k, top_p, min_p = self.own
        mp = dict(min_p=min_p) if min_p > 0.0 else {}    # (with min-p off the call is the one made before min-p existed)
        return self.ops.residual_sample_lp(score, d_rows, n_acc, r, bonus, self.inv_t, d_threshold=d_thr, t_threshold=t_thr,
                                           top_k=top_k, top_p=top_p, **mp)


class _SampledRows(_Sampled):
    """The rows route (module docstring, PER-REQUEST SAMPLING): _Sampled with every row under its own values, through the
    packed tables, uploaded once.  `table`: each row's temperature with its own top-k / top-p / min-p; `draft` (verifying
    stages): each row's temperature with the draft stage's configured truncation -- what the proposals are drawn with."""

    def __init__(self, stage: "Stage", plan: _Plan, B: int, device):
        super().__init__(stage, plan, B, device)
        inv_t, top_k, top_p, min_p = plan.rows
        V, pack = stage.shape.vocab, stage.ops.pack_sampling_rows
        # (a table is packed for the dtype of the logits it is used on: `draft` for the draft stage's)
        self.table = self.draft = pack(inv_t, top_k, top_p, min_p, V, stage.config.dtype, device)
        if stage.draft is not None:
            dcfg = stage.draft.config
            self.draft = pack(inv_t, [int(dcfg.top_k)] * B, [float(dcfg.top_p)] * B, [float(dcfg.min_p)] * B, V, dcfg.dtype, device)

    def _draft_op(self, logits, r):
        return self.ops.draft_sample_rows(logits, r, self.draft)

    def _verify_op(self, score, tok32, lp_d, u):
        lp_t, _, n_acc, _, t_thr, _ = self.ops.verify_accept_rows(score, tok32, lp_d, u, self.table)
        return lp_t, n_acc, t_thr

    def _residual_op(self, score, d_rows, n_acc, r, bonus, d_thr, t_thr):
        return self.ops.residual_sample_lp_rows(score, d_rows, n_acc, r, bonus, self.table, d_threshold=d_thr, t_threshold=t_thr)


class _CallState:
    """The device side of one generate call, built in this one place from the plan and the encoded prompts and handed to the
    loop: how rows end (`end`), the allow-list (`mask`, None without a list), the logit edit (`edit`, None without an entry), the
    guided automata (`fsm`, None when no row is guided), the bad words (`bad`, None when no row has one), the n-gram rule
    (`ngram`, None when every row's n is 0), the penalties (`pen`, None when every row is neutral), the sampler and the top-N
    tables (`top`, None when off), the per-token statistics (`stats`, None when off) and the prompt's scores (`prompt`, None when off).  `step_tok`: the [B, draft_len] buffer of the step's proposals, ONE per call, which `fsm`,
    `bad`, `ngram` and `pen` all read at a verifying stage (None at stage 0, and when all four are off).  Uploads happen here, once; a part
    that is off costs no launch.  `prompt_ids`: every row's prompt ids without the padding."""

    def __init__(self, stage: "Stage", plan: _Plan, ids: torch.Tensor, prompt_ids: List[List[int]]):
        (B, P), dev, ops = ids.shape, ids.device, stage.ops
        self.end = _StopSequences(ops, plan.row_seqs, plan.limits, P, dev) if plan.finish_route else \
            _StopIds(ops, plan.stop, B, dev) if plan.stop else _RunToLimit(ops)
        self.mask = _MaskState(ops, plan.mask_rows, stage.shape.vocab, dev) if any(r is not None for r in plan.mask_rows) else None
        self.edit = _EditState(ops, plan.edit_rows, P, dev) if any(plan.edit_rows) else None
        history = any(plan.bad_rows) or any(plan.ngram_rows) or bool(plan.penalties) or plan.fsm is not None
        self.step_tok = torch.zeros((B, stage.config.draft_len), dtype=torch.int32, device=dev) \
            if history and stage.draft is not None else None
        self.fsm = _FsmState(ops, plan.fsm, 1 if stage.draft is None else stage.config.draft_len + 1, self.step_tok, dev) \
            if plan.fsm is not None else None
        self.bad = _BadWordState(ops, plan.bad_rows, P, P + plan.max_tokens, self.step_tok, dev) if any(plan.bad_rows) else None
        self.ngram = _NgramState(ops, plan.ngram_rows, prompt_ids, P, P + plan.max_tokens, self.step_tok, dev) \
            if any(plan.ngram_rows) else None
        self.pen = _PenaltyState(ops, plan.penalties, prompt_ids, stage.shape.vocab, self.step_tok, dev) if plan.penalties else None
        # greedy: no draws, no truncation, no table, a seed is ignored; else rows or scalars, decided here and nowhere else
        self.sampler = _Greedy(ops) if plan.greedy else (_SampledRows if plan.rows else _Sampled)(stage, plan, B, dev)
        self.top = _TopState(ops, plan.n_top, plan.inv_t, B, P + plan.max_tokens, dev,
                             self.sampler.table if plan.rows else None) if plan.n_top else None
        self.stats = _StatsState(ops, self.top, plan.inv_t, B, P + plan.max_tokens, dev,
                                 self.sampler.table if plan.rows else None) if plan.token_stats else None
        self.prompt = _PromptState(ops, plan.n_prompt, ids, prompt_ids) if plan.n_prompt is not None else None
        # the entropy cuts: `cut` on the stage's own rows, `cut_draft` on a verifying stage's draft rows; both with the rows' temperatures
        inv_t = list(plan.rows[0]) if plan.rows else [plan.inv_t] * B
        self.cut = _CutState(ops, plan.cut_rows, inv_t, dev) if plan.cut_rows else None
        self.cut_draft = _CutState(ops, plan.cut_draft_rows, inv_t, dev) if plan.cut_draft_rows else None


def _shape_of(cfg: StageConfig) -> LMShape:
    if cfg.shape is not None:
        return cfg.shape
    key = _DEFAULT_SHAPES.get(cfg.model_size, cfg.model_size)
    if key not in QWEN25_SHAPES:
        raise ValueError(f"no model shape for stage {cfg.model_size!r}: set StageConfig.shape")
    return QWEN25_SHAPES[key]


class Stage:
    def __init__(self, config: StageConfig, index: int, draft: Optional["Stage"], ops, device):
        self.config = config
        self.index = index
        self.name = config.model_size
        self.model_size = config.model_size
        self.model_name = config.model_name
        self.cost_per_token = float(config.cost_per_token)
        self.draft = draft                               # the stage below (its model drafts for this one); None for stage 0
        self.ops = ops
        self.device = torch.device(device)
        self.shape = _shape_of(config)
        if draft is not None and draft.shape.vocab != self.shape.vocab:
            raise ValueError("a stage and the stage below it must share the vocabulary")
        if not 1 <= config.draft_len <= 64:
            raise ValueError("draft_len must be in [1, 64]")
        _check_min_p(config.min_p, "min_p")
        _check_min_p(config.target_min_p, "target_min_p")
        check_entropy_cuts(config.typical_p, config.epsilon_cutoff, config.eta_cutoff, 1)
        check_entropy_cuts(config.target_typical_p, config.target_epsilon_cutoff, config.target_eta_cutoff, 1)
        self.model = SyntheticLM(self.shape, dtype=config.dtype, device=self.device, seed=config.model_seed,
                                 logit_scale=config.logit_scale)
        self.tokenizer = SimpleTokenizer()
        self.gen = torch.Generator(device=self.device).manual_seed(int(config.seed))
        self.keep_inputs = False                         # tests: keep every step's inputs and draws in `step_inputs`
        self.step_inputs: List[dict] = []
        self.prompt_inputs: Optional[dict] = None        # tests: the prefill logits, targets and first rows a call scored
        self.last_steps = 0

    def get_model_info(self) -> Dict[str, object]:
        c = self.config
        return {"name": self.model_name, "size": self.model_size, "stage": self.index, "shape": self.shape.name,
                "parameters": self.shape.param_count(), "vocab": self.shape.vocab, "cost_per_token": self.cost_per_token,
                "draft": None if self.draft is None else self.draft.model_size, "draft_len": c.draft_len,
                "tensor_parallel_size": c.tensor_parallel_size, "quantized": c.quantized, "device": str(self.device)}

    # ------------------------------------------------------------------------------------------ prompts / text
    def encode_prompts(self, prompts: Sequence[str]) -> torch.Tensor:
        """[B, P] int64 on the stage's device: the last P ids of every prompt, left-padded with id 0 (module docstring)."""
        return self._encode(prompts)[0]

    def _encode(self, prompts: Sequence[str]) -> Tuple[torch.Tensor, List[List[int]]]:
        """-> (encode_prompts' tensor, every row's kept ids WITHOUT the padding: the lists the tensor was padded from)."""
        V = self.shape.vocab
        rows = [[i % V for i in self.tokenizer.encode(p, return_tensors=None)] for p in prompts]
        P = max(2, min(max((len(r) for r in rows), default=0), int(self.config.max_prompt_tokens)))
        real = [r[-P:] for r in rows]
        rows = [[0] * (P - len(r)) + r for r in real]
        return torch.tensor(rows, dtype=torch.int64).reshape(len(rows), P).to(self.device), real

    @staticmethod
    def decode_tokens(ids: Sequence[int]) -> str:
        return " ".join(f"t{int(i)}" for i in ids)

    # ------------------------------------------------------------------------------------------ generate
    @torch.no_grad()
    def generate(self, prompts: List[str], max_tokens=512, temperature=0.7, return_logprobs: bool = True,
                 top_p=None, stop_token_ids: Optional[Sequence[int]] = None,
                 logprobs: Optional[int] = None,
                 min_p=None,
                 seed=None, stop_sequences=None,
                 stop_sequences_per_prompt=None, top_k=None, logit_bias=None, banned_token_ids=None,
                 min_tokens=None, allowed_token_ids=None, repetition_penalty=None, presence_penalty=None,
                 frequency_penalty=None, bad_words=None,
                 bad_words_per_prompt=None, guided_fsm=None, guided_choice=None,
                 guided_choice_per_prompt=None,
                 no_repeat_ngram_size=None,
                 prompt_logprobs: Optional[int] = None,
                 token_stats: Optional[bool] = None,
                 typical_p=None, epsilon_cutoff=None,
                 eta_cutoff=None) -> Tuple[List[str], Optional[List[np.ndarray]], Dict[str, object]]:
        """-> (texts, logprobs, {"generation_time_ms": ...}).  texts[i]: the committed token ids as space-joined token strings
        ("t123 t7 ..."; len(text.split()) is the token count, as the reference counts it); logprobs[i]: float32 [n_i], log-prob
        of every committed token under THIS stage's (truncated, renormalised) distribution.  `top_p` overrides the nucleus of that
        distribution for the call: StageConfig.top_p at stage 0, StageConfig.target_top_p at a verifying stage.
        `stop_token_ids`: None = StageConfig.stop_token_ids, an empty sequence = no stop set.  n_i = max_tokens without a stop set;
        with one, the tokens up to and including the first stop id (module docstring).  stats["n_tokens"][i] = n_i and
        stats["finish_reasons"][i] = "stop" | "length".
        `logprobs`: None = StageConfig.logprobs; N in 1..8 adds stats["top_token_ids"][i] (int32 [n_i, N]) and
        stats["top_logprobs"][i] (float32 [n_i, N]): per committed token the N most likely tokens of the UNTRUNCATED
        temperature-scaled distribution it came from, most likely first (ties: lowest id), ragged like logprobs[i]; 0 = off.
        With top-k / top-p active the token's own (renormalised) log-prob is not less than its table entry, and the token is
        always inside the nucleus (module docstring).  Anything outside 0..8 raises ValueError.
        `min_p` overrides min-p for the call by the rule of `top_p`: StageConfig.min_p at stage 0, StageConfig.target_min_p at a
        verifying stage; None = the configuration's, 0 = off, outside [0, 1] raises ValueError (module docstring, MIN-P).
        `seed`: None = the stage's own generator (StageConfig.seed), as before; an int in [0, 2^64) for every prompt, or a
        sequence of len(prompts) such ints, makes row i's uniforms a function of (seed_i, this stage's index, the step) alone
        -- not of the row index, the batch size, the other requests, earlier calls, StageConfig.seed or draft_len -- through one
        ops.step_uniforms call per step and no torch.rand.  The same call repeated, and a permuted batch of equal-length prompts
        with the seeds permuted alike, return bit-equal texts and log-probs; another batch size may not (left-padding and the
        model kernels' tilings change the logits).  Greedy decoding ignores it.  Anything else raises ValueError (module
        docstring, SEEDS).
        `max_tokens`: an int, or one int >= 1 per prompt (row i then returns at most max_tokens[i] tokens).  `stop_sequences`:
        None = StageConfig.stop_sequences; strings or sequences of 1..8 token ids that end EVERY prompt's row;
        `stop_sequences_per_prompt`: len(prompts) such lists (possibly empty), each for its own row.  A row ends behind the first
        committed token at which one of its sequences is complete in the GENERATED tokens; the matched tokens are kept.
        stats["stop_matches"][i] is the tuple of token ids that ended row i ((id,) for a stop id), or None for "length".
        A row's list -- stop ids, common sequences, its own -- holds at most 16 distinct entries (module docstring, HOW A ROW
        ENDS).
        `temperature`, `top_p`, `min_p` and `top_k` (None = the configuration's: StageConfig.top_k at stage 0, target_top_k at a
        verifying stage) each take one value or one per prompt; unequal values select the rows route, where row i is sampled
        with its own four values; a temperature sequence may not mix 0 with positive values (module docstring, PER-REQUEST
        SAMPLING).
        `logit_bias` ({token id: bias in [-100, 100]}, raw logit units, added before the temperature), `banned_token_ids` (ids
        whose logit becomes -inf; a ban wins over a bias) and `min_tokens` (the row's stop ids and one-token stop sequences are
        banned until it has generated that many tokens): None = the configuration's; one value for every prompt or one per
        prompt.  Draft and target logits receive the same edit, so log-probs and top-N tables are those of the edited
        distribution and a banned token is never proposed, accepted, drawn or listed (module docstring, LOGIT EDITS).
        `allowed_token_ids` (vLLM's): None = StageConfig.allowed_token_ids; a sequence of ids for every prompt, or one sequence
        (or None: no list) per prompt.  Every logit outside a row's list becomes -inf, on the draft's and the target's logits
        alike and ahead of the edits above, so only listed tokens are proposed, accepted, drawn or listed and the log-probs are
        those of the restricted distribution; with `logprobs` = N above the list's size the unfillable slots hold id -1 and
        -inf.  An empty list, and a list that the bans or min_tokens' stop ids empty, raise ValueError; a stop id outside a
        row's list can never end that row (module docstring, ALLOW-LISTS).
        `repetition_penalty` (in (0, 2]; 1 = off), `presence_penalty` and `frequency_penalty` (in [-2, 2]; 0 = off) are vLLM's:
        None = the StageConfig field of that name; one value for every prompt or one per prompt.  A token that occurs in the
        row's prompt or among its generated tokens has its logit divided (when positive) or multiplied (otherwise) by the
        repetition penalty; a token that occurs c > 0 times among the generated tokens loses frequency_penalty * c +
        presence_penalty.  The history at a position includes the step's own proposals in front of it, draft and target logits
        receive the same penalty, and log-probs and top-N tables are those of the penalised distribution, behind the mask and
        the edits above and ahead of the temperature (module docstring, PENALTIES).
        `bad_words` (vLLM's, on token ids): None = StageConfig.bad_words; strings (encoded like a stop string) or sequences of
        1..8 token ids that NO prompt's row may produce; `bad_words_per_prompt`: len(prompts) such lists (possibly empty), each
        for its own row, behind the common list.  A word of one token is banned for ever; the last token of a longer word is
        banned at every position whose history -- the row's generated tokens, the prompt excluded, and the step's own proposals
        in front of the position -- ends in the word's other tokens, so no row's generated tokens hold a word as a contiguous
        run.  Draft and target logits receive the same ban, behind the mask and ahead of the edits and the penalties, and
        log-probs and top-N tables are those of the distribution with the banned tokens removed.  Duplicates are dropped; a
        row keeps at most 256 words; a row whose allow-list (or vocabulary) the bans and the words' last ids would empty
        raises ValueError (module docstring, BAD WORDS).
        `guided_fsm` (None = StageConfig.guided_fsm): one serving.guided.TokenFSM for every prompt, or one TokenFSM (or None:
        the row is free) per prompt; `guided_choice` (None = StageConfig.guided_choice): one list of choices -- strings, encoded
        like a stop string, or sequences of 1..64 token ids, at most 256 -- for every prompt; `guided_choice_per_prompt`:
        len(prompts) such lists, None or an empty list leaving the row free.  A guided row produces only tokens its automaton
        allows in the state its generated tokens have led to; in an accepting state it may produce one of its stop ids (which
        ends it), elsewhere its stop ids are forbidden.  A guided-choice row therefore returns exactly one choice followed by
        one stop id with reason "stop", or a prefix of a choice with reason "length"; it needs a stop id.  Draft and target
        logits receive the same mask at every position, directly behind the allow-list's, and log-probs and top-N tables are
        those of the restricted distribution.  A row with both an automaton and choices, `min_tokens` > 0 on a guided row,
        more than 1024 states in a call, and a reachable state that the row's other restrictions leave without a token raise
        ValueError (module docstring, GUIDED DECODING).
        `no_repeat_ngram_size` (HF generate's): None = StageConfig.no_repeat_ngram_size; an int in [0, 8] for every prompt or
        one per prompt, 0: off.  With n > 0 no n-gram that ends in a row's generated tokens equals an earlier n-gram of its
        prompt (the real ids, not the padding) plus generated tokens: at every position the tokens that followed an earlier
        occurrence of the last n - 1 tokens of the history -- prompt, generated tokens, and the step's own proposals in front
        of the position -- are banned; n = 1 bans every token of the history.  Draft and target logits receive the same ban,
        behind the bad words and ahead of the edits and the penalties, and log-probs and top-N tables are those of the
        distribution with the repeating tokens removed.  A row whose vocabulary (or allow-list) its bans and prompt length +
        max_tokens + draft_len repeats could empty, and a guided row with n > 0, raise ValueError (module docstring, NO REPEAT
        N-GRAM).
        `prompt_logprobs` (vLLM's; OpenAI's echo + logprobs): None = StageConfig.prompt_logprobs, and None there is off; an int
        N in [0, 8] scores the prompt under THIS stage's model, raw and at temperature 1.  With m_i = (row i's real prompt
        tokens) - 1, entry j belongs to real prompt token j + 1 (the first has no log-prob): stats["prompt_token_ids"][i] (int32
        [m_i + 1], all real ids), stats["prompt_logprobs"][i] (float32 [m_i]: log p(token | the tokens before it)),
        stats["prompt_ranks"][i] (int32 [m_i]: 1 = the most likely token; ties by lowest id) and, with N >= 1,
        stats["prompt_top_token_ids"][i] (int32 [m_i, N]) / stats["prompt_top_logprobs"][i] (float32 [m_i, N]), most likely
        first.  N = 0 is ON and returns no table.  Off: none of the keys.  The generated tokens, their log-probs and tables
        keep their bits; a bool, a float, a sequence or a value outside [0, 8] raises ValueError (module docstring, PROMPT
        LOG-PROBS).
        `token_stats`: None = StageConfig.token_stats; True adds, ragged like logprobs[i], stats["token_entropy"][i] (float32
        [n_i]: the entropy in nats of the distribution committed token j came from), stats["token_max_logprobs"][i] (float32
        [n_i]) and stats["token_argmax_ids"][i] (int32 [n_i]): that distribution's most likely token and its log-prob -- the
        top-N table's slot 0 --, stats["token_ranks"][i] (int32 [n_i]: the committed token's rank there, 1 = the most likely,
        ties by lowest id; rank <= N means the token stands in table slot rank - 1; greedy rows have rank 1) and
        stats["predictor_features"] (float32 [B, 256]: FeatureExtractor.extract_device on the two float arrays, formed on the
        device).  The distribution is the one the top-N table describes: processed, temperature-scaled, UNTRUNCATED.  Off: none
        of the five keys and no extra call.  Tokens, log-probs and tables keep their bits; anything but None or a bool raises
        ValueError (module docstring, TOKEN STATS).
        `typical_p`, `epsilon_cutoff`, `eta_cutoff` (HF's warpers of those names, min_tokens_to_keep = 1): None = the
        configuration's (StageConfig.typical_p / epsilon_cutoff / eta_cutoff at stage 0, the target_* fields at a verifying
        stage: the rule of `min_p`); one number for every prompt or one per prompt.  typical_p lies in [0, 1] (0 and 1: off),
        the other two in [0, 1) (0: off); a row has at most one of the three.  They act on p = softmax(x / T) of the row behind
        every other processor, at the row's temperature and untruncated, with its entropy H: typical_p = m keeps the tokens
        whose |-ln p_v - H| is smallest until their mass reaches m (ties kept; the most likely token may be cut);
        epsilon_cutoff = e cuts p_v < e; eta_cutoff = e cuts p_v < min(e, sqrt(e) exp(-H)); the last two keep every token
        that ties the maximum.  The cut runs LAST of the processors and AHEAD of top-k, top-p and min-p, which act on the
        survivors -- llama.cpp's order, not HF's (Temperature -> TopK -> TopP -> MinP -> Typical -> Epsilon -> Eta); with
        those three off the kept set is HF's.  Log-probs, top-N tables and token statistics describe the distribution behind
        the cut.  Greedy decoding ignores all three.  A bool, a NaN, a value outside its range, the wrong length and two of
        them on one row raise ValueError (module docstring, ENTROPY CUTS)."""
        t0 = time.perf_counter()
        self.step_inputs = []
        self.prompt_inputs = None
        plan = self._plan(prompts, max_tokens, temperature, top_p, stop_token_ids, logprobs, min_p, seed, stop_sequences,
                          stop_sequences_per_prompt, top_k, logit_bias, banned_token_ids, min_tokens, allowed_token_ids,
                          repetition_penalty, presence_penalty, frequency_penalty, bad_words, bad_words_per_prompt, guided_fsm,
                          guided_choice, guided_choice_per_prompt, no_repeat_ngram_size, prompt_logprobs, token_stats,
                          typical_p, epsilon_cutoff, eta_cutoff)
        if not plan.prompts or plan.max_tokens <= 0:
            return ["" for _ in plan.prompts], ([np.zeros(0, np.float32) for _ in plan.prompts] if return_logprobs else None), \
                {"generation_time_ms": 0.0}
        ids, prompt_ids = self._encode(plan.prompts)
        P = ids.shape[1]
        if any(plan.ngram_rows):                 # (the one check that needs the prompts' lengths: host lists, nothing launched yet)
            check_ngram_rows_keep_a_token(plan.ngram_rows, [len(r) for r in prompt_ids], plan.limits,
                                          0 if self.draft is None else self.config.draft_len, plan.mask_rows, plan.edit_rows,
                                          plan.bad_rows, self.shape.vocab)
        state = _CallState(self, plan, ids, prompt_ids)
        decode = self._decode_plain if self.draft is None else self._decode_speculative
        tokens, lps, seq_len = decode(ids, plan.max_tokens, state)
        self.ops.check_status()
        feats = None if state.stats is None else state.stats.features(P, seq_len, plan.prompts, self.index)   # before any read-back
        tok_h = tokens[:, P:].cpu().numpy()
        lp_h = lps[:, P:].cpu().numpy().astype(np.float32, copy=False)
        n_tok, reasons, matches = state.end.outcome(seq_len, tok_h, P, plan.limits)
        texts = [self.decode_tokens(row[:n]) for row, n in zip(tok_h, n_tok)]
        stats = {"generation_time_ms": (time.perf_counter() - t0) * 1000.0, "steps": float(self.last_steps),
                 "n_tokens": n_tok, "finish_reasons": reasons, "stop_matches": matches}
        if state.top is not None:
            id_h, tlp_h = state.top.ids[:, P:].cpu().numpy(), state.top.lps[:, P:].cpu().numpy()
            stats["top_token_ids"] = [np.ascontiguousarray(r[:n]) for r, n in zip(id_h, n_tok)]
            stats["top_logprobs"] = [np.ascontiguousarray(r[:n]) for r, n in zip(tlp_h, n_tok)]
        if state.stats is not None:
            stats.update(state.stats.stats(P, n_tok, feats))
        if state.prompt is not None:
            stats.update(state.prompt.stats())
        return texts, ([np.ascontiguousarray(r[:n]) for r, n in zip(lp_h, n_tok)] if return_logprobs else None), stats

    def _plan(self, prompts, max_tokens, temperature, top_p, stop_token_ids, logprobs, min_p, seed, stop_sequences,
              stop_sequences_per_prompt, top_k, logit_bias, banned_token_ids, min_tokens, allowed_token_ids,
              repetition_penalty, presence_penalty, frequency_penalty, bad_words, bad_words_per_prompt, guided_fsm=None,
              guided_choice=None, guided_choice_per_prompt=None, no_repeat_ngram_size=None, prompt_logprobs=None,
              token_stats=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None) -> _Plan:
        """generate's arguments -> the call's _Plan: every check (ValueError before any launch and before encode_prompts), every
        `None = the configuration's` default -- a stage's own side is (top_k, top_p, min_p) at stage 0 and (target_top_k,
        target_top_p, target_min_p) at a verifying stage -- and the choice of route."""
        cfg, V, prompts = self.config, self.shape.vocab, tuple(prompts)
        n = len(prompts)
        given = lambda v, default: default if v is None else v                       # noqa: E731
        stop = _check_stop_ids(given(stop_token_ids, cfg.stop_token_ids), V)
        n_top = _check_logprobs(given(logprobs, cfg.logprobs))
        n_prompt = _check_prompt_logprobs(given(prompt_logprobs, cfg.prompt_logprobs))
        token_stats = bool(given(_check_token_stats(token_stats), _check_token_stats(cfg.token_stats)))
        own_top_k, own_top_p, own_min_p = (cfg.top_k, cfg.top_p, cfg.min_p) if self.draft is None else \
            (cfg.target_top_k, cfg.target_top_p, cfg.target_min_p)
        min_p = check_per_prompt(given(min_p, own_min_p), n, "min_p")
        top_p = given(check_per_prompt(top_p, n, "top_p"), float(own_top_p))
        top_k = given(check_per_prompt(top_k, n, "top_k"), int(own_top_k))
        if _is_seq(temperature):
            temperature = check_per_prompt(temperature, n, "temperature")
            if isinstance(temperature, list) and any(t == 0.0 for t in temperature):
                raise ValueError("greedy (temperature 0) and sampled rows cannot share one generate call: split the batch")
        elif isinstance(temperature, bool):
            raise ValueError(f"temperature must be a number, got {temperature!r}")
        seeds = check_seeds(seed, n)
        max_tokens = check_max_tokens(max_tokens, n)
        common = _check_stop_sequences(given(stop_sequences, cfg.stop_sequences), V, self.tokenizer)
        own = [[] for _ in prompts]
        if stop_sequences_per_prompt is not None:
            if isinstance(stop_sequences_per_prompt, (str, bytes)) or len(stop_sequences_per_prompt) != n:
                raise ValueError(f"stop_sequences_per_prompt must hold one list per prompt ({n})")
            own = [_check_stop_sequences(e, V, self.tokenizer) for e in stop_sequences_per_prompt]
        row_seqs = [[(i,) for i in stop] + common + o for o in own]
        for r in row_seqs:
            if len(r) > MAX_STOP_SEQS:
                raise ValueError(f"a prompt's stop list (stop ids included) holds at most {MAX_STOP_SEQS} entries, got {len(r)}")
            if len(set(r)) != len(r):
                raise ValueError("the stop sequences of a prompt must be distinct")
        edit_rows = merge_logit_edits(check_logit_bias(given(logit_bias, cfg.logit_bias), n, V),
                                      check_banned_token_ids(given(banned_token_ids, cfg.banned_token_ids), n, V),
                                      min_tokens := check_min_tokens(given(min_tokens, cfg.min_tokens), n), row_seqs, V)
        mask_rows = check_allowed_token_ids(given(allowed_token_ids, cfg.allowed_token_ids), n, V)
        bad_rows = check_bad_words(given(bad_words, cfg.bad_words), bad_words_per_prompt, n, V, self.tokenizer)
        check_rows_keep_a_token(mask_rows, edit_rows, bad_rows, V)
        fsm_rows = check_guided(given(guided_fsm, cfg.guided_fsm), given(guided_choice, cfg.guided_choice), guided_choice_per_prompt,
                                n, V, self.tokenizer)
        ngram_rows = check_no_repeat_ngram_size(given(no_repeat_ngram_size, cfg.no_repeat_ngram_size), n)
        for b, (f, g) in enumerate(zip(fsm_rows, ngram_rows)):
            if f is not None and g > 0:          # (a state's allowed set can be one token, which the n-gram rule may ban)
                raise ValueError(f"prompt {b}: no_repeat_ngram_size > 0 is not built for a guided row")
        fsm = None
        if any(f is not None for f in fsm_rows):
            for b, (f, m) in enumerate(zip(fsm_rows, min_tokens)):
                if f is not None and m > 0:      # (its temporary ban of the stop ids can empty an accepting leaf)
                    raise ValueError(f"prompt {b}: min_tokens > 0 is not built for a guided row")
            # Z: the row's length-1 stop-list entries -- its stop ids and one-token stop sequences (what grammar back ends do with EOS)
            fsm = compile_rows(fsm_rows, [[s[0] for s in r if len(s) == 1] for r in row_seqs], V)
            check_guided_rows_keep_a_token(fsm, fsm_rows, mask_rows, edit_rows, bad_rows)
        penalties = (check_repetition_penalty(given(repetition_penalty, cfg.repetition_penalty), n),
                     check_presence_penalty(given(presence_penalty, cfg.presence_penalty), n),
                     check_frequency_penalty(given(frequency_penalty, cfg.frequency_penalty), n))
        if all(r == 1.0 and p == 0.0 and f == 0.0 for r, p, f in zip(*penalties)):
            penalties = None                             # every row neutral: no state, no call
        own_cuts = (cfg.typical_p, cfg.epsilon_cutoff, cfg.eta_cutoff) if self.draft is None else \
            (cfg.target_typical_p, cfg.target_epsilon_cutoff, cfg.target_eta_cutoff)
        cut_rows = check_entropy_cuts(*(given(v, d) for v, d in zip((typical_p, epsilon_cutoff, eta_cutoff), own_cuts)), n)
        dcfg = None if self.draft is None else self.draft.config
        cut_draft_rows = [] if dcfg is None else check_entropy_cuts(dcfg.typical_p, dcfg.epsilon_cutoff, dcfg.eta_cutoff, n)
        limits = max_tokens if isinstance(max_tokens, list) else [max_tokens] * n
        limit = max(limits, default=0)
        live = n > 0 and limit > 0               # (a call that returns at once never looked at a scalar temperature: it still does not)
        if live and not isinstance(temperature, list) and not temperature >= 0.0:     # (NaN included)
            raise ValueError("temperature must be >= 0 (0: greedy decoding)")
        greedy = not live or (not isinstance(temperature, list) and temperature == 0.0)
        scalars = rows = None
        if not greedy and any(isinstance(v, list) for v in (temperature, top_p, top_k, min_p)):
            # the rows route (module docstring, PER-REQUEST SAMPLING): every row's four values
            temps, top_k, top_p, min_p = (v if isinstance(v, list) else [v] * n for v in (temperature, top_k, top_p, min_p))
            rows = ([float(np.float32(1.0 / t)) for t in temps], top_k, top_p, min_p)
            temperature = temps[0]
        elif not greedy:
            scalars = (top_k, top_p, min_p)
        return _Plan(prompts=prompts, limits=tuple(limits), max_tokens=int(limit), greedy=greedy,
                     inv_t=1.0 if greedy else float(np.float32(1.0 / temperature)), scalars=scalars, rows=rows,
                     stop=stop, row_seqs=row_seqs, finish_route=len(set(limits)) > 1 or bool(common) or any(own),
                     edit_rows=edit_rows, mask_rows=mask_rows, bad_rows=bad_rows, ngram_rows=ngram_rows,
                     penalties=penalties, fsm=fsm, seeds=seeds, n_top=n_top, n_prompt=n_prompt,
                     token_stats=token_stats,
                     cut_rows=cut_rows if not greedy and any(m for m, _ in cut_rows) else None,        # greedy ignores the cuts
                     cut_draft_rows=cut_draft_rows if not greedy and any(m for m, _ in cut_draft_rows) else None)

    def _buffers(self, ids: torch.Tensor, cap: int):
        B, P = ids.shape
        dev = ids.device
        tokens = torch.zeros((B, cap), dtype=torch.int32, device=dev)
        tokens[:, :P] = ids.to(torch.int32)
        lps = torch.zeros((B, cap), dtype=torch.float32, device=dev)
        seq_len = torch.full((B,), P, dtype=torch.int32, device=dev)
        n_commit = torch.zeros((B,), dtype=torch.int32, device=dev)
        return tokens, lps, seq_len, n_commit

    def _decode_plain(self, ids: torch.Tensor, max_tokens: int, st: _CallState):
        """Stage 0.  Without a stop set every sequence appends exactly one token per step, so all positions are known on the
        host and nothing is read back; with one (`st.end.stops`), a sequence is fed its last committed token at seq_len - 1,
        which is the same for a running sequence and stays put for a finished one."""
        B, P = ids.shape
        dev = ids.device
        cap = P + max_tokens
        end, mask, bad, edit, pen, top, sampler = st.end, st.mask, st.bad, st.edit, st.pen, st.top, st.sampler
        fsm, ngram, stat, cut = st.fsm, st.ngram, st.stats, st.cut
        tokens, lps, seq_len, n_commit = self._buffers(ids, cap)
        m = self.model
        m.reset()
        m.alloc_ragged(B, cap + 1)
        logits = m.forward_ragged(ids, torch.zeros((B,), dtype=torch.int64, device=dev), P)
        if st.prompt is not None:                # rows 0 .. P - 2 score prompt tokens 1 .. P - 1: raw, ahead of every edit below
            self.prompt_inputs = st.prompt.score(logits[:, :P - 1], self.keep_inputs)
        logits = logits[:, -1]
        for step in range(max_tokens):
            if sampler.dense:
                logits = logits.contiguous()
            if mask is not None:
                mask.apply(logits)                                       # the allow-list first, then the sparse edit (they commute)
            if fsm is not None:
                fsm.apply(logits)                                        # mask -> fsm: the state behind the committed tokens
            if bad is not None:
                bad.apply(logits, tokens, seq_len)                       # mask -> bad words -> n-gram -> edit -> penalties
            if ngram is not None:
                ngram.apply(logits, tokens, seq_len)                     # the history: the prompt's real ids and the committed tokens
            if edit is not None:
                edit.apply(logits, seq_len)                              # ahead of the draw and the top-N pass
            if pen is not None:
                pen.apply(logits)                                        # the penalties last: mask -> edit -> penalties
            cut_in = cut.apply(logits, self.keep_inputs) if cut is not None else None   # the entropy cut: behind every processor
            n_acc, tok, lp = sampler.draw(logits, step)
            kept = sampler.kept(seq_len) if self.keep_inputs else None
            if kept is not None and cut is not None:
                kept["cut_in"] = cut_in
            if stat is not None:
                stat.score(logits, None, n_acc, tok)                     # one pass: the statistics, and the table when it is on
            elif top is not None:
                top.score(logits)
            end.commit(None, None, n_acc, tok, lp, seq_len, tokens, lps, n_commit, cap)
            if top is not None:
                top.commit(seq_len, n_commit)
            if stat is not None:
                stat.commit(seq_len, n_commit)
            if pen is not None:
                pen.commit(tokens, seq_len, n_commit, cap)               # the committed tokens enter the history
            if fsm is not None:
                fsm.commit(tokens, seq_len, n_commit, cap)               # ... and move the automaton
            if kept is not None:                                        # tests: the record, with the top-N rows behind it
                if top is not None:
                    kept = dict(kept, **top.record(), n_commit=n_commit.clone())
                self.step_inputs.append(kept if stat is None else dict(kept, **stat.record(), n_commit=n_commit.clone()))
            self.last_steps = step + 1
            if end.stops and (step + 1) % self.config.sync_every == 0 and end.done(seq_len, cap):
                break
            if step + 1 < max_tokens:
                if end.stops:
                    pos = seq_len.to(torch.int64) - 1
                    last = tokens.gather(1, pos[:, None]).to(torch.int64)
                else:
                    pos = torch.full((B,), P + step, dtype=torch.int64, device=dev)
                    last = tok.to(torch.int64)[:, None]
                logits = m.forward_ragged(last, pos, P + step + 1)[:, -1]
        return tokens, lps, seq_len

    def _decode_speculative(self, ids: torch.Tensor, max_tokens: int, st: _CallState):
        """Stage s > 0: speculative_generate_ragged's step on `ops`, with the log-probs committed beside the tokens.

        Invariant at the top of a step, L = seq_len[b]: tokens[b, :L] are committed; the target's KV is valid for positions
        < L - 1 and the draft's for positions < L - 2, so the target is fed [t_{L-1}, d_0 .. d_{K-1}] at position L - 1 (row i
        scores d_i, row K is the bonus row) and the draft first re-feeds the last two committed tokens."""
        cfg = self.config
        draft, target = self.draft.model, self.model
        B, P = ids.shape
        dev = ids.device
        Kd = cfg.draft_len
        cap = P + max_tokens
        end, mask, bad, edit, pen, top, sampler = st.end, st.mask, st.bad, st.edit, st.pen, st.top, st.sampler
        fsm, ngram, stat, cut, cut_draft = st.fsm, st.ngram, st.stats, st.cut, st.cut_draft
        step_tok = st.step_tok                                          # the step's proposals, for `fsm`, `bad`, `ngram` and `pen`; None: all off
        tokens, lps, seq_len, n_commit = self._buffers(ids, cap)
        for m in (draft, target):
            m.reset()
            m.alloc_ragged(B, cap + Kd + 2)
        zero = torch.zeros((B,), dtype=torch.int64, device=dev)
        prefill = target.forward_ragged(ids[:, :P - 1], zero, P)        # prefill: everything but the last prompt token
        if st.prompt is not None:                # the target's [B, P - 1, V] rows, before the next pass; the draft's are not scored
            self.prompt_inputs = st.prompt.score(prefill, self.keep_inputs)
        del prefill
        if P > 2:
            draft.forward_ragged(ids[:, :P - 2], zero, P)
        rows = torch.arange(B, device=dev)
        steps = 0
        while True:
            L = seq_len.to(torch.int64)
            window = min(P + steps * (Kd + 1) + Kd + 1, cap + Kd + 2)   # host-side bound on every position touched this step
            last2 = torch.stack([tokens[rows, L - 2], tokens[rows, L - 1]], 1).to(torch.int64)
            dl = draft.forward_ragged(last2, L - 2, window)[:, -1]
            sampler.start(steps)
            toks, cut_in_draft = [], []
            for k in range(Kd):
                if sampler.dense:
                    dl = dl.contiguous()
                if mask is not None:
                    mask.apply(dl)
                if fsm is not None:
                    fsm.apply(dl, k)                                    # the state behind the proposals 0 .. k - 1
                if bad is not None:
                    bad.apply(dl, tokens, seq_len, k)                   # the history: the committed tokens, then proposals 0 .. k - 1
                if ngram is not None:
                    ngram.apply(dl, tokens, seq_len, k)                 # ... with the prompt's real ids in front
                if edit is not None:
                    edit.apply(dl, seq_len, k)                          # proposal k decides generated token L - P + k
                if pen is not None:
                    pen.apply(dl, k)                                    # ... and sees the proposals 0 .. k - 1 of this step
                if cut_draft is not None:
                    cut_in_draft.append(cut_draft.apply(dl, self.keep_inputs))   # the DRAFT stage's configured cut, last
                toks.append(sampler.propose(dl, k))
                if step_tok is not None:
                    step_tok[:, k] = toks[-1]
                if fsm is not None:
                    fsm.advance(k)                                      # column k + 1; the last one is the bonus row's
                if k + 1 < Kd:
                    dl = draft.forward_ragged(toks[-1].to(torch.int64)[:, None], L + k, window)[:, -1]
            tok32 = torch.stack(toks, 1).to(torch.int32).contiguous()
            t_out = target.forward_ragged(torch.cat([last2[:, 1:], tok32.to(torch.int64)], 1), L - 1, window)   # [B, K+1, V]
            if mask is not None:
                mask.apply(t_out)                                       # the whole [B, K+1, V] output, before any slice
            if fsm is not None:
                fsm.apply(t_out)                                        # row j under the state the draft's proposal j had
            if bad is not None:
                bad.apply(t_out, tokens, seq_len)                       # row j sees the proposals 0 .. j - 1, as the draft's did
            if ngram is not None:
                ngram.apply(t_out, tokens, seq_len)                     # the same history per row as the draft's proposal j had
            if edit is not None:
                edit.apply(t_out, seq_len)                              # the same edit on the target's K + 1 rows, before any slice
            if pen is not None:
                pen.apply(t_out)                                        # row j sees the proposals 0 .. j - 1, as the draft's did
            cut_in = cut.apply(t_out, self.keep_inputs) if cut is not None else None    # the call's own cut on the K + 1 rows
            lp_t, n_acc, drawn, lp_drawn = sampler.settle(t_out, tok32)
            kept = sampler.kept(seq_len) if self.keep_inputs else None
            if kept is not None and cut is not None:
                kept["cut_in"] = cut_in
            if kept is not None and cut_draft is not None:              # the draft rows as they entered and as they left the cut
                kept["cut_in_draft"] = torch.stack(cut_in_draft, 1)
                kept["cut_out_draft"] = torch.stack(sampler.dls, 1)
            if stat is not None:
                stat.score(t_out, tok32, n_acc, drawn)                  # one pass: the statistics, and the table when it is on
            elif top is not None:
                top.score(t_out)                                        # the [B, K+1, V] output as returned, not a copy
            end.commit(tok32, lp_t, n_acc, drawn, lp_drawn, seq_len, tokens, lps, n_commit, cap)
            if top is not None:
                top.commit(seq_len, n_commit)
            if stat is not None:
                stat.commit(seq_len, n_commit)
            if pen is not None:
                pen.commit(tokens, seq_len, n_commit, cap)               # the committed tokens enter the history
            if fsm is not None:
                fsm.commit(tokens, seq_len, n_commit, cap)               # ... and move the automaton
            if kept is not None:                                        # tests: the record, with the top-N rows behind it
                if top is not None:
                    kept = dict(kept, **top.record(), n_commit=n_commit.clone())
                self.step_inputs.append(kept if stat is None else dict(kept, **stat.record(), n_commit=n_commit.clone()))
            steps += 1
            if steps % cfg.sync_every == 0 and end.done(seq_len, cap):
                break
            if steps > max_tokens + cfg.sync_every:      # cannot happen: every step appends >= 1 token per unfinished row
                raise RuntimeError("stage loop did not terminate")
        self.last_steps = steps
        return tokens, lps, seq_len


class StageManager:
    """The reference's StageManager(stage_configs, gpu_allocation) (server.py:163): stages in the order of `stage_configs`,
    stage i drafting for stage i + 1.  `ops`: the arithmetic behind every step (default distributed.HipOps -> libasd_hip.so on
    the current GPU); a CPU ops object makes every stage run on CPU tensors, as in serving/hierarchy.py.  `gpu_allocation`
    ({size: [gpu ids]}) is accepted and reported by get_model_info(); multi-rank stages are not built, all stages share the
    ops' device."""

    def __init__(self, stage_configs: Sequence[StageConfig], gpu_allocation: Optional[Dict[str, List[int]]] = None, ops=None):
        self.ops = ops if ops is not None else HipOps()
        self.gpu_allocation = dict(gpu_allocation or {})
        self.device = torch.device("cuda", torch.cuda.current_device()) if isinstance(self.ops, HipOps) else torch.device("cpu")
        self.stages: Dict[str, Stage] = {}
        below: Optional[Stage] = None
        for i, cfg in enumerate(stage_configs):
            if cfg.model_size in self.stages:
                raise ValueError(f"duplicate stage {cfg.model_size!r}")
            below = self.stages[cfg.model_size] = Stage(cfg, i, below, self.ops, self.device)
        self.names = tuple(self.stages)

    def get_stage(self, name: str) -> Stage:
        return self.stages[name]

    def warmup_all(self, max_tokens: int = 2) -> None:
        for s in self.stages.values():
            s.generate(["warm up"], max_tokens=max_tokens)

    def get_model_info(self) -> Dict[str, Dict[str, object]]:
        return {n: dict(s.get_model_info(), gpus=self.gpu_allocation.get(n)) for n, s in self.stages.items()}
