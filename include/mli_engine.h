/*
 * mli_engine.h -- C ABI over the host engine loops (continuous batching + paged KV allocator) of
 * libmli_hip.so.  It binds what the reference exposes as C++ only:
 *   start_inference_engine / start_paged_attention_inference_engine /
 *   start_paged_attention_cublas_inference_engine       (reference include/inferencer.h:18-32)
 * together with the objects their callers build first (ItemStorage, ProcessingStorage,
 * MemoryBlockManager, PagedAttentionsManager, *InferenceModel; reference tests/paged_for_profile.cpp:10-62).
 * One engine drives one GPU.  bench.py and the tests use it through ctypes; a C++ host links the classes
 * directly (min_llm_inference_amd/host/include).
 */
#ifndef MLI_ENGINE_H
#define MLI_ENGINE_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mli_engine mli_engine;

/* MLI_ENGINE_PAGED_BF16 is an EXTENSION (the reference is fp32 only): the paged GEMM engine over bf16 pages and
 * bf16 Wk/Wq/Wv (the fp32 host weights are rounded to nearest-even at creation); emb_dim % 8 == 0; a page is
 * 16 * 3 * emb_dim bf16 elements. */
/* MLI_ENGINE_PAGED_FP8 is an EXTENSION, opt-in: OCP e4m3 pages (x, K and V: one byte per element under
 * the same layout rule, a page is 16 * 3 * emb_dim bytes), bf16 Wk/Wq/Wv, fp32 everywhere else; emb_dim % 16 == 0; lean
 * compositions only. */
enum { MLI_ENGINE_CONTIGUOUS = 0, MLI_ENGINE_PAGED = 1, MLI_ENGINE_PAGED_GEMM = 2, MLI_ENGINE_PAGED_BF16 = 3,
       MLI_ENGINE_PAGED_FP8 = 4 };

typedef struct {
    int kind;             /* MLI_ENGINE_* */
    int n_batch;          /* slots in the continuous batch */
    int n_sequence;       /* max tokens per item (multiple of 16 for the paged kinds) */
    int emb_dim;          /* multiple of 4 */
    int n_vocab;
    int n_blocks;         /* paged: pages in the pool (each 16 * 3 * emb_dim floats) */
    int n_forward_rounds; /* paged: decode rounds per iteration, 1..16 */
    int device;           /* GPU ordinal this engine runs on */
    int reference_length_reset_quirk; /* 1 = reproduce src/paged_item_storage.cpp:110-118 (measurement only) */
} mli_engine_config;

typedef struct {
    long long total_tokens; /* tokens appended by process_decoder_result (ThroughputCounter) */
    double seconds;         /* wall time since the first insert, host work and copies included */
    long long iterations;   /* engine iterations executed */
    int finished;           /* items finished */
    int waiting;            /* items still queued */
    int in_flight;          /* items occupying a slot */
} mli_engine_stats;

/* Weights are HOST pointers (row-major fp32): emb_table [n_vocab, emb_dim], pos_table [n_sequence, emb_dim],
 * wk/wq/wv [emb_dim, emb_dim]; they are copied to the device.  Returns 0 or a negative error
 * (mli_engine_last_error() has the message). */
int mli_engine_create(const mli_engine_config* config, const float* emb_table, const float* pos_table,
                      const float* wk, const float* wq, const float* wv, mli_engine** out);
void mli_engine_destroy(mli_engine* engine);

/* Give the engine its own non-blocking HIP stream (default: the calling thread's stream, i.e. the legacy default
 * stream, as the reference).  Engines with private streams can be driven from different threads of one process
 * and overlap on one GPU: while one waits for its decoder result and does its host bookkeeping, the other's
 * kernels run.  Each engine has its own ThroughputCounter, scratch and page pool; an engine is driven by one
 * thread at a time. */
int mli_engine_use_private_stream(mli_engine* engine);

/* EXTENSION: the pipelined loop of the paged kinds -- the host works one step behind the GPU (page
 * growth and admission for step k+1 while step k's result is still in flight; per-slot device updates instead of
 * whole-tensor uploads), min_llm_inference_amd/host/include/pipelined_engine.h.  Per-item token streams are identical
 * to the sequential loop's.  It is what mli_engine_run uses BY DEFAULT wherever it applies: a paged kind,
 * n_forward_rounds <= 8, no reference_length_reset_quirk, an engine that has not been stepped.  enabled = 0 selects
 * the reference's sequential loop order, enabled = 1 insists on the pipelined loop (mli_engine_run then fails where it
 * does not apply, and mli_engine_step is refused).  Call before the first run. */
int mli_engine_set_pipelined(mli_engine* engine, int enabled);

/* Queue one item (ItemStorage::add_new_item). */
int mli_engine_add_item(mli_engine* engine, int id, const int* tokens, int n_tokens);

/* EXTENSION: queue an item that is decoded by sampling (temperature > 0) or greedily (temperature == 0): the contract of
 * mli_sample_tokens (mli_kernels.h), drawn at each new token's position with this item's seed, so an item's tokens do
 * not depend on its slot, the batch, the loop, n_forward_rounds, preemption or step graphs.  -1 with a message for
 * temperature < 0 or not finite, top_k < 0, top_p outside (0, 1], an id already queued by this entry point, or an
 * engine created with reference_length_reset_quirk.  The engine chooses its head once, at the first step or run:
 * sampled if a queued item has temperature > 0 (plain mli_engine_add_item items then decode with temperature 0),
 * otherwise the greedy head, after which an item with temperature > 0 is refused. */
int mli_engine_add_item_sampled(mli_engine* engine, int id, const int* tokens, int n_tokens, float temperature,
                                int top_k, float top_p, unsigned long long seed);

/* Run to completion (the reference's start_*_engine). */
int mli_engine_run(mli_engine* engine, mli_engine_stats* stats);

/* One iteration: forward -> process_decoder_result -> page bookkeeping -> insert_new_items.  The first call
 * also performs the initial insert.  *done is set to 1 once every item has finished. */
int mli_engine_step(mli_engine* engine, int* done);

int mli_engine_get_stats(mli_engine* engine, mli_engine_stats* stats);

/* Device pointer to the int32 decoder output of the last iteration, [n_batch, n_forward_rounds]
 * (what a multi-GPU host all-gathers), and its element count. */
int mli_engine_decoder_result(mli_engine* engine, void** device_ptr, int* count);

/* The stream this engine's kernels run on (hipStream_t as void*; NULL = the legacy default stream): what a multi-GPU host
 * enqueues the token all-gather on (include/mli_shard.h). */
int mli_engine_stream(mli_engine* engine, void** stream);

/* Finished item `index` (0 <= index < stats.finished), in completion order: id and tokens (prompt + generated). */
int mli_engine_get_finished(mli_engine* engine, int index, int* id, int* tokens, int capacity, int* n_tokens);

/* EXTENSION: per-token log-probabilities and top-n alternatives (mli_kernels.h: mli_sample_tokens_logprobs, DESIGN.md
 * 3.6c).  For every token it generates, the engine records the natural-log probability of that token under the RAW model
 * distribution at its position -- independent of the item's temperature, top_k, top_p and seed, so greedy and sampled
 * items report on one scale -- and the n_top (0 .. 8) candidates of largest logit with theirs, ordered by (logit
 * descending, index ascending).  Before the first step or run; all five kinds.  -1 with a message for a null engine, a
 * started engine, an engine created with reference_length_reset_quirk, n_top outside 0 .. 8, or an engine an id was already
 * queued on twice.  An engine the call was never made on behaves exactly as before.
 * What it changes: the engine decodes with the sampled head family (materialised logits) even when every item is greedy
 * -- plain mli_engine_add_item items decode with temperature 0, as in any sampled engine --, the token streams are those
 * of the same engine without logprobs, and item ids must be unique from then on (mli_engine_add_item and
 * mli_engine_add_item_sampled refuse a duplicate).  The figures cross to the host with the tokens, at the same
 * synchronisation point of either loop, and are kept per item id where the token is appended: a token dropped in flight by
 * a preemption takes its figures with it, a re-admitted item keeps those of the tokens it had generated; n_forward_rounds
 * and step graphs need nothing more. */
int mli_engine_set_logprobs(mli_engine* engine, int n_top);

/* The figures of finished item `index` (the index of mli_engine_get_finished): entry i belongs to token n_prompt + i of
 * that item's tokens, and *n_generated == n_tokens - *n_prompt always.  Up to `capacity` entries of token_logprobs and up
 * to `top_capacity` entries of top_ids / top_logprobs ([n_generated, n_top] row-major) are written; any of the three may
 * be NULL.  -1 on an engine without logprobs. */
int mli_engine_get_finished_logprobs(mli_engine* engine, int index, int* n_prompt, float* token_logprobs, int capacity,
                                     int* n_generated, int* top_ids, float* top_logprobs, int top_capacity);

/* EXTENSION: PROMPT log-probabilities (mli_kernels.h: mli_paged_prompt_logprobs).  Beside the figures of the
 * tokens it generates, the engine reports for every prompt token but the first the natural-log probability the model gives
 * it after the tokens before it, and the n_top alternatives at that position -- the figures mli_engine_set_logprobs defines,
 * for a token that was GIVEN: scoring and perplexity, ranking of continuations, "echo".  The new rows' prompts are scored in
 * the forward that prefills them, directly behind the prefill and on the same stream, in passes of at most n_batch positions
 * (a longer prompt continues in the next pass).  An item is scored at its first admission only: a preempted and re-admitted
 * item keeps its figures and is not scored again, and "prompt" means the tokens it was queued with.  Tokens and
 * generated-token figures are bit-identical to the same engine without the switch, in both loops, with several rounds, step
 * graphs and sampling; a forward with new rows waits for its figures to reach the host, every other forward is untouched.
 * Call before the first step or run and after mli_engine_set_logprobs, which supplies n_top.  -1 with a message for a null
 * or started engine, an engine without logprobs, MLI_ENGINE_CONTIGUOUS and MLI_ENGINE_PAGED_FP8, an engine with page release
 * (its prefill skips dead pages, so the prompt's K / V are not all there; mli_engine_set_page_release afterwards is refused
 * likewise), or a shape the prompt scan does not take (rows of more than two 16-byte lane loads: emb_dim > 512 fp32 / 1024
 * bf16). */
int mli_engine_set_prompt_logprobs(mli_engine* engine, int enabled);

/* The prompt figures of finished item `index` (the index of mli_engine_get_finished): entry i belongs to prompt token i + 1,
 * and *n_scored == n_prompt - 1 always (a one-token prompt has none).  Up to `capacity` entries of token_logprobs and up to
 * `top_capacity` entries of top_ids / top_logprobs ([n_scored, n_top] row-major) are written; any of the three may be NULL.
 * -1 on an engine without prompt log-probabilities. */
int mli_engine_get_finished_prompt_logprobs(mli_engine* engine, int index, float* token_logprobs, int capacity, int* n_scored,
                                            int* top_ids, float* top_logprobs, int top_capacity);

/* The DEFAULT of engines created afterwards (every engine keeps its own value, see mli_engine_configure; two engines in one
 * process never change each other's composition): 1 (default) = the models' layers run the lean compositions (prefill with the encoder as the fill GEMM's
 * prologue, attention without materialised scores / probabilities, decoder head with the argmax as the logits GEMM's
 * epilogue), 0 = the reference's launch sequence (encoder, fill, latest, scan + combine, logits, argmax).  Tokens are
 * identical either way; the switch exists to measure one against the other. */
void mli_engine_set_lean_layers(int enabled);

/* The DEFAULT of engines created afterwards: 1 = the models replay their pure decode forwards (no newly inserted rows) from a hipGraph recorded on
 * the first such forward -- one host call per forward instead of one per launch (host/include/step_graph.h).  Only
 * engines with a private stream can record (the legacy default stream cannot be captured); others keep launching
 * eagerly.  Default 0: a replay costs the GPU a few microseconds more than the same launches issued from C++. */
void mli_engine_set_step_graphs(int enabled);

/* This engine's own switches, before its first step / run: lean_layers and step_graphs as above; -1 leaves a value as
 * it is.  (The fp8 engine has the lean compositions only.) */
int mli_engine_configure(mli_engine* engine, int lean_layers, int step_graphs);

/* EXTENSION: multi-head attention (mli_kernels.h: mli_paged_attention_lean_heads).  n_heads heads of
 * head_dim = emb_dim / n_heads, head h owning columns [h * head_dim, (h + 1) * head_dim) of q, K and V; one softmax per
 * head over q_h . K_h / sqrtf(head_dim).  Before the first step or run; kinds MLI_ENGINE_PAGED, MLI_ENGINE_PAGED_GEMM and
 * MLI_ENGINE_PAGED_BF16.  -1 with a message for another kind, an unsupported (emb_dim, n_heads) -- head_dim 32, 64, 128 or
 * 256, emb_dim <= 512 (fp32) / 1024 (bf16) --, an engine configured with lean_layers = 0 (mli_engine_configure(e, 0, ...)
 * afterwards is refused likewise) or a call after the first step.  n_heads = 1 is accepted everywhere and changes
 * nothing.  Loops, step graphs, preemption, sampling and n_forward_rounds work as with one head. */
int mli_engine_set_heads(mli_engine* engine, int n_heads);

/* EXTENSION: grouped-query attention (mli_kernels.h: mli_paged_attention_lean_gqa).  n_kv_heads K/V heads serve the
 * engine's n_heads query heads: query head h attends K/V head h / (n_heads / n_kv_heads), which owns columns
 * [(h / g) * head_dim, (h / g + 1) * head_dim) of K and V.  Only the first n_kv_heads * head_dim output columns of the
 * engine's wk / wv matter; pages, pool, projection, prefill and the heads do not change.  Before the first step or run.
 * n_kv_heads must divide the engine's CURRENT n_heads (set the heads first); n_kv_heads == n_heads is accepted by every
 * engine kind and changes nothing (on an engine that holds a grouping it takes the grouping away: every head has its own
 * K/V head again, and nothing stays stored).  Anything else needs MLI_ENGINE_PAGED, MLI_ENGINE_PAGED_GEMM or
 * MLI_ENGINE_PAGED_BF16 with lean layers (mli_engine_configure(e, 0, ...) afterwards is refused likewise) and is STORED:
 * a later mli_engine_set_heads keeps the stored n_kv_heads, and is refused for a value n_kv_heads does not divide (for
 * n_heads == n_kv_heads every head has its own K/V head until the heads change again).  -1 with a message that names
 * n_kv_heads for n_kv_heads < 1, a non-divisor, another kind, lean_layers = 0 or a call after the first step.  Composes
 * in any order with window, sinks, page release, sampling, n_forward_rounds, step graphs and both loops: none of them
 * looks at K / V columns. */
int mli_engine_set_kv_heads(mli_engine* engine, int n_kv_heads);

/* EXTENSION: ALiBi (mli_kernels.h: mli_paged_attention_lean_alibi).  Every decode scan of the engine adds
 * slopes[h] * (s - (L - 1)) to query head h's scaled score of the row's slot s (L: the row's length, s absolute in the row).
 * slopes_host: n floats in HOST memory, n == the engine's CURRENT n_heads (set the heads first), every one finite; a null
 * pointer stands for the standard slopes of n_heads heads (mli_alibi_slopes; n is then ignored).  The engine keeps a device
 * copy.  Pages, pool, projection, prefill and the decoder head never see the bias.  Before the first step or run;
 * MLI_ENGINE_PAGED, MLI_ENGINE_PAGED_GEMM or MLI_ENGINE_PAGED_BF16 with lean layers.  Composes with mli_engine_set_heads (the
 * same count again), _set_kv_heads, _set_window, _set_sinks, _set_page_release, _set_logprobs, sampling, both loops,
 * n_forward_rounds and step graphs; every setter validates the combination, whichever comes last.  -1 with a message for a
 * null engine, n_heads < 2 or n != n_heads, a non-finite slope, MLI_ENGINE_CONTIGUOUS and MLI_ENGINE_PAGED_FP8, a started
 * engine, lean_layers = 0 (mli_engine_configure(e, 0, ...) afterwards is refused likewise, as is mli_engine_set_heads with
 * another count), and an engine with prompt log-probabilities (mli_engine_set_prompt_logprobs afterwards is refused likewise:
 * the prompt scan has no bias, and a prompt would be scored under another model than the one that decodes).  Without the call
 * nothing changes anywhere. */
int mli_engine_set_alibi(mli_engine* engine, const float* slopes_host, int n);

/* EXTENSION: rotary position embeddings (mli_kernels.h: mli_paged_prefill_rope, mli_paged_attention_lean_rope).  Every prefill
 * and every decode projection of the engine rotates K (before its one rounding to the page's element type) and q by the
 * token's absolute slot in its row; the scans, the pool, V, x and the decoder head do not change.  The position table
 * (pos_table of mli_engine_create) is still added: a RoPE model passes zeros.  _set_rope builds the standard table
 * (mli_rope_table) of theta for the engine's CURRENT n_heads (set the heads first; head_dim = emb_dim / n_heads, emb_dim for
 * MLI_ENGINE_PAGED_FP8); _set_rope_table takes any table -- n_floats == n_sequence * head_dim floats of HOST memory,
 * [n_sequence][head_dim / 2] (cos, sin), every one finite (the scaled variants are just another table; all (1, 0) gives the
 * tokens of the engine without the call).  The engine keeps a device copy at a fixed address, so a captured step graph replays
 * it.  Before the first step or run; MLI_ENGINE_PAGED, _PAGED_GEMM, _PAGED_BF16 and _PAGED_FP8 with lean layers.  Composes with
 * heads, K/V heads, window, sinks, page release (positions are never renumbered), ALiBi, sampling, logprobs, both loops,
 * n_forward_rounds and step graphs; a preempted item is prefilled again at the same slots.  -1 with a message for a null
 * engine (or table), MLI_ENGINE_CONTIGUOUS, a started engine, lean_layers = 0 (mli_engine_configure(e, 0, ...) afterwards is
 * refused likewise), an odd or fractional head_dim, a wrong n_floats, a non-finite entry or theta not finite or <= 0, an
 * engine with prompt log-probabilities (mli_engine_set_prompt_logprobs afterwards is refused likewise: the prompt scan's q is
 * not rotated), and mli_engine_set_heads with another count after a table was set.  Without the calls nothing changes
 * anywhere. */
int mli_engine_set_rope(mli_engine* engine, double theta);
int mli_engine_set_rope_table(mli_engine* engine, const float* table_host, size_t n_floats);

/* EXTENSION: attention logit soft-capping (mli_kernels.h: mli_paged_attention_lean_softcap).  Every decode scan of the engine
 * -- and, with mli_engine_set_prompt_logprobs, every prompt scan -- replaces query head h's scaled score x of an attended slot
 * by cap * tanh(x / cap): the engine scores its prompts under the model it decodes with.  cap: finite and > 0; 0 turns the cap
 * off again.  Pages, pool, projection, prefill and the decoder head never see it.  Before the first step or run;
 * MLI_ENGINE_PAGED, MLI_ENGINE_PAGED_GEMM or MLI_ENGINE_PAGED_BF16 with lean layers and two heads at least (set the heads
 * first).  Composes with mli_engine_set_kv_heads, _set_window, _set_sinks, _set_page_release, _set_rope[_table],
 * _set_logprobs, _set_prompt_logprobs, sampling, both loops, n_forward_rounds and step graphs; every setter validates the
 * combination, whichever comes last.  -1 with a message for a null engine, a negative or non-finite cap, n_heads < 2
 * (mli_engine_set_heads(e, 1) afterwards is refused likewise), MLI_ENGINE_CONTIGUOUS and MLI_ENGINE_PAGED_FP8, a started
 * engine, lean_layers = 0 (mli_engine_configure(e, 0, ...) afterwards is refused likewise), and an engine with ALiBi
 * (mli_engine_set_alibi afterwards is refused likewise: no order of bias and cap is defined).  Without the call nothing changes
 * anywhere. */
int mli_engine_set_softcap(mli_engine* engine, float cap);

/* EXTENSION: learned attention-sink logits (mli_kernels.h: mli_paged_attention_lean_sink_logits has the formula and the
 * anchors).  Every decode scan of the engine -- and, with mli_engine_set_prompt_logprobs, every prompt scan -- counts
 * logits_host[h] as one more logit of query head h's softmax without a value row: the engine scores its prompts under the model
 * it decodes with.  n must equal the engine's current n_heads (set the heads first; two at least); every value finite or -inf
 * (-inf: no sink for that head; all -inf gives the tokens and log-probabilities of the engine without the call, bit for bit).
 * logits_host null turns the switch off again.  The engine keeps a device copy at a fixed address, so step graphs replay it.
 * Pages, pool, projection, prefill and the decoder head never see the logits.  Before the first step or run;
 * MLI_ENGINE_PAGED, MLI_ENGINE_PAGED_GEMM or MLI_ENGINE_PAGED_BF16 with lean layers.  Composes with mli_engine_set_kv_heads,
 * _set_window, _set_sinks (sink TOKENS, another switch), _set_page_release, _set_rope[_table], _set_logprobs,
 * _set_prompt_logprobs, sampling, both loops, n_forward_rounds, step graphs and preemption; every setter validates the
 * combination, whichever comes last.  -1 with a message naming the reason for a null or started engine, MLI_ENGINE_CONTIGUOUS
 * and MLI_ENGINE_PAGED_FP8, n_heads < 2 (mli_engine_set_heads to another count afterwards is refused likewise), n != n_heads,
 * NaN or +inf, lean_layers = 0 (mli_engine_configure(e, 0, ...) afterwards is refused likewise), and an engine with ALiBi or
 * with a soft cap (mli_engine_set_alibi and mli_engine_set_softcap afterwards are refused likewise: no model defines the
 * combination).  Without the call nothing changes anywhere. */
int mli_engine_set_sink_logits(mli_engine* engine, const float* logits_host, int n);

/* EXTENSION: sliding-window attention (mli_kernels.h: mli_paged_attention_lean_window).  Every row attends its newest
 * `window` tokens only.  The window changes which slots the scan reads and nothing else: admission, page growth,
 * preemption, re-prefill, n_forward_rounds (the window follows the device-side length), step graphs, sampling and the
 * pipelined loop work as without one, and no page is returned to the pool early unless mli_engine_set_page_release.  Before
 * the first step or run; kinds
 * MLI_ENGINE_PAGED, MLI_ENGINE_PAGED_GEMM, MLI_ENGINE_PAGED_BF16 and MLI_ENGINE_PAGED_FP8; combines with
 * mli_engine_set_heads in either order (each call validates the combination).  -1 with a message for another kind,
 * window < 1, a call after the engine has started, an engine configured with lean_layers = 0
 * (mli_engine_configure(e, 0, ...) afterwards is refused likewise) or a shape the windowed scan does not take.
 * window >= n_sequence is accepted everywhere and changes nothing. */
int mli_engine_set_window(mli_engine* engine, int window);

/* EXTENSION: attention sinks beside the window (mli_kernels.h: mli_paged_attention_lean_sinks).  Every row attends its
 * first n_sink tokens as well as its newest `window`.  Like the window, sinks change which slots the scan reads and
 * nothing else: admission, growth, preemption, re-prefill, n_forward_rounds, step graphs, sampling and the pipelined loop
 * work as without them, and no page is returned to the pool early unless mli_engine_set_page_release.  Before the first
 * step or run; the four paged kinds;
 * combines with mli_engine_set_heads and mli_engine_set_window in any order (each call validates the combination).
 * Without an effective window (none set, or window >= n_sequence) it is accepted and changes nothing until one is set.
 * -1 with a message for MLI_ENGINE_CONTIGUOUS, n_sink < 0, a call after the engine has started, or an engine configured
 * with lean_layers = 0. */
int mli_engine_set_sinks(mli_engine* engine, int n_sink);

/* EXTENSION: early page release beside the window.  A row under a window of W tokens with K sinks never again reads the
 * pages between its sink pages and its window's first page (index ceil(K / 16) <= i < max(0, n - W) / 16 at n tokens).
 * With release on, those pages go back to the pool while the row decodes, a new or re-admitted item takes and prefills
 * its live pages only (mli_kernels.h: mli_paged_prefill_window), and a row never holds more than
 *   ceil(K / 16) + ceil((W + a) / 16) + 1 pages,   a = n_forward_rounds (sequential loop) or 2 n_forward_rounds (pipelined),
 * whatever n_sequence: the same pool serves more rows with fewer preemptions, and a pool smaller than n_sequence / 16
 * pages decodes a row to n_sequence.  Tokens are those of the engine without release.  Before the first step or run; the
 * four paged kinds; combines with mli_engine_set_window, mli_engine_set_sinks and mli_engine_set_heads in any order (the
 * switch is read at the first step or run).  Without an effective window (none set, window >= n_sequence, or n_sink +
 * window >= n_sequence) it is accepted and changes nothing.  -1 with a message for MLI_ENGINE_CONTIGUOUS, a call after the
 * engine has started, or an engine with reference_length_reset_quirk (the quirk moves device lengths backwards; release
 * rests on lengths that only grow). */
int mli_engine_set_page_release(mli_engine* engine, int enabled);

/* EXTENSION: occupancy of the page pool, for every paged kind with or without release: pages the pool has, pages out of it
 * now and at most so far, pages returned early by mli_engine_set_page_release, and rows pushed back to the queue because
 * the pool ran dry.  -1 for MLI_ENGINE_CONTIGUOUS. */
typedef struct {
    int pool_pages, in_use, peak_in_use;
    long long released_early, preemptions;
} mli_engine_page_stats;
int mli_engine_get_page_stats(mli_engine* engine, mli_engine_page_stats* stats);

const char* mli_engine_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MLI_ENGINE_H */
