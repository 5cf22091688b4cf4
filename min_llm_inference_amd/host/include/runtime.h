// Per-thread execution context: which GPU this thread drives and which stream kernels go to.
// The reference is single-GPU and launches everything on the legacy default stream; that stays the
// default here (compute_stream() == nullptr).  A multi-GPU host creates one engine per GPU, each on its
// own thread or process, and calls use_device() first.
#pragma once

#include <cstddef>

namespace mli {
namespace runtime {

void use_device(int ordinal);          // hipSetDevice for the calling thread
int current_device();
void set_compute_stream(void* stream); // hipStream_t as void*; nullptr = legacy default stream
void* compute_stream();
void* create_stream();                  // a non-blocking stream for one engine (several engines per GPU overlap)
void destroy_stream(void* stream) noexcept;
void synchronize();                    // hipStreamSynchronize(compute stream) / device sync for the default stream

// Device scratch of the split-sequence attention kernels (mli_attention_workspace_bytes): one buffer per device,
// grown on demand, owned by the host library because the C ABI never allocates.
struct Scratch {
    void* ptr;
    size_t bytes;
};
// n_heads > 1 (EXTENSION, multi-head scan): sized by mli_attention_heads_workspace_bytes, which covers the single-head need
Scratch attention_scratch(int n_batch, int n_sequence, int emb_dim, int n_heads = 1);
void release_attention_scratch(void* stream) noexcept;  // frees the buffers tied to a stream that is going away

// The three switches below are PER THREAD, like the device and the compute stream: they apply to what the calling thread
// runs afterwards (an engine is driven by one thread at a time; engines created through the C ABI carry their own values,
// mli_engine.h).
//
// What the layers run (default true): the LEAN compositions -- attention without materialising scores /
// probabilities in the layer's qkt_output scratch, decoder head with the argmax as the logits GEMM's epilogue instead of
// materialising emb_score.  Outputs a caller of forward() can observe (attention_result, tokens, lengths, pages) are
// bit-identical either way; false reproduces the reference's launch sequence, scratch contents included.
void set_lean_layers(bool enabled);
bool lean_layers();

// The one lean dispatch of the paged attention layers (fp32, bf16 and fp8 pages: elem = MLI_ELEM_*).
// lean_paged_wanted: does the layer run the lean composition?  Multi-head and sliding-window attention (0 < window <
// n_sequence) exist there only: with lean layers off they throw.
// lean_paged_attention: sizes the scratch and calls the one entry point that serves (n_heads, window, n_sink), chosen by
// lean_scan_kind (scan_plan.hpp) -- window <= 0 or >= n_sequence: none; n_sink counts beside a window only (attention
// sinks: the first n_sink tokens stay attended).  One head without a window returns the entry point's status
// (MLI_ERR_BAD_ARG where the rows are too wide for the single-pass kernel: the caller may take its materialising
// composition); every other form throws on failure.  n_kv_heads (EXTENSION, grouped-query attention): 0 or n_heads = every
// query head has its own K/V head, the calls above; anything else is mli_paged_attention_lean_gqa.  alibi_slopes (EXTENSION,
// n_heads floats in device memory; null: none): mli_paged_attention_lean_alibi, whatever the other options are.  rope_table
// (EXTENSION, [n_sequence][head_dim / 2] (cos, sin) in device memory; null: none): mli_paged_attention_lean_rope, whatever the
// other options are, slopes included; every failure throws.  softcap (EXTENSION, logit soft-capping; 0: none):
// mli_paged_attention_lean_softcap, with or without a rotary table; slopes beside it throw.  sink_logits (EXTENSION, n_heads
// floats in device memory; null: none): mli_paged_attention_lean_sink_logits, with or without a rotary table; slopes or a cap
// beside them throw.
bool lean_paged_wanted(int n_heads, int window, int n_sequence);
int lean_paged_attention(int elem, int n_heads, int window, int n_sink, void* const* page_table, const int* lengths,
                         const void* wk, const void* wq, const void* wv, const int* new_batch_idx, float* q_output,
                         float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_new_items,
                         int n_kv_heads = 0, const float* alibi_slopes = nullptr, const float* rope_table = nullptr,
                         float softcap = 0.f, const float* sink_logits = nullptr);

// Which loop start_paged_attention_*_inference_engine runs (default false): the pipelined loop
// (pipelined_engine.h: the host one step behind the GPU, same tokens per item) wherever it applies -- up to
// PAGE_BLOCK_SIZE / 2 forward rounds, no length-reset quirk --, or, with true, always the reference's sequential order
// forward -> process_decoder_result -> allocate_or_free_memory_blocks_if_needed -> insert_new_items.
void set_sequential_engine_loop(bool enabled);
bool sequential_engine_loop();

// hipGraph replay of decode forwards (step_graph.h); default false.
void set_step_graphs(bool enabled);
bool step_graphs();

// roctx ranges around engine phases (the reference wraps them in NVTX ranges, src/inferencer.cpp:55-82)
void range_push(const char* name);
void range_pop();

}  // namespace runtime
}  // namespace mli
