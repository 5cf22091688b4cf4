// extern "C" engine sessions (include/mli_engine.h): the reference's engine loops in resumable form, so a
// host in another language -- or bench.py -- can step them and interleave the multi-GPU token gather.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <memory>
#include <numeric>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "bf16_extension.h"
#include "constants.h"
#include "fp8_extension.h"
#include "inference_model.h"
#include "inferencer.h"
#include "kernels/decoder.h"
#include "mli_engine.h"
#include "mli_kernels.h"
#include "pipelined_engine.h"
#include "prompt_plan.hpp"  // cut_prompt_passes
#include "runtime.h"
#include "scan_plan.hpp"   // heads_shape_supported, window_shape_supported, prompt_scan_shape_ok
#include "throughput_counter.h"

namespace {

thread_local std::string g_last_error;
// what an engine created from now on starts with (mli_engine_set_lean_layers / mli_engine_set_step_graphs); every engine
// keeps its own copy, installed for the calling thread while one of its entry points runs
std::atomic<bool> g_default_lean_layers{true};
std::atomic<bool> g_default_step_graphs{false};

TensorFloat upload(const float* host, std::vector<size_t> shape) {
    TensorFloat staging(shape, DeviceType::HOST);
    std::memcpy(staging.data(), host, staging.get_total_size() * sizeof(float));
    TensorFloat device(shape, DeviceType::DEVICE);
    device.copy_from(staging);
    return device;
}

}  // namespace

struct mli_engine {
    mli_engine_config cfg;
    TensorFloat emb_table, pos_table;
    ItemStorage item_storage;
    ProcessingStorage processing_storage;
    std::unique_ptr<InferenceModel> naive_model;  // the contiguous kind's model, or
    std::unique_ptr<PagedInferenceModel> paged;   // the model of one of the four paged kinds
    std::unique_ptr<MemoryBlockManager> pool;
    std::unique_ptr<PagedAttentionsManager> pages;
    TensorInt inp_device, inp_host, lengths_device, lengths_host, new_idx_device, new_idx_host;
    TensorInt result_device, result_host;
    bool started = false;
    int n_new_items = 0;
    long long iterations = 0;
    ThroughputCounter counter;  // this engine's own (the reference has one per process)
    int pipelined = -1;         // mli_engine_set_pipelined: 1 / 0 = run() uses the pipelined / the sequential loop,
                                // -1 (default) = pipelined wherever it applies (see use_pipelined())
    // the pipelined loop serves the paged kinds with up to PAGE_BLOCK_SIZE / 2 rounds, without the reference's quirk,
    // and only an engine that is run to completion from the start (mli_engine_step drives the sequential loop)
    bool pipelined_applies() const {
        return paged_kind() && 2 * cfg.n_forward_rounds <= PAGE_BLOCK_SIZE &&
               !cfg.reference_length_reset_quirk && !started;
    }
    bool use_pipelined() const { return pipelined == 1 || (pipelined == -1 && pipelined_applies()); }
    void* stream = nullptr;     // private compute stream (mli_engine_use_private_stream), else the thread's
    bool lean_layers = g_default_lean_layers.load();   // this engine's composition and replay switches (runtime.h)
    bool step_graphs = g_default_step_graphs.load();
    // What mli_engine_set_heads / _kv_heads / _window / _sinks have accepted is kept in one place, the paged model's own
    // option set (layers.h): n_heads, n_kv_heads (0: as many as n_heads), window (0: none), n_sink (counts beside a window
    // only).  Every one of those setters refuses the contiguous kind, which therefore reads the defaults.
    PagedAttentionOptions no_options;
    PagedAttentionOptions& options() { return paged ? paged->options() : no_options; }
    bool release_pages = false; // mli_engine_set_page_release: takes effect at the first step or run, beside an effective window

    bool paged_kind() const { return cfg.kind != MLI_ENGINE_CONTIGUOUS; }   // mli_engine_create admits the five kinds only
    bool heads_kind() const { return paged_kind() && cfg.kind != MLI_ENGINE_PAGED_FP8; }  // the fp8 scan has one head
    int elem() const {   // MLI_ELEM_* of the kind's pages
        return cfg.kind == MLI_ENGINE_PAGED_FP8 ? MLI_ELEM_FP8 : cfg.kind == MLI_ENGINE_PAGED_BF16 ? MLI_ELEM_BF16 : MLI_ELEM_F32;
    }
    DecoderHeadSetters& model_head() {
        if (paged) return *paged;
        return *naive_model;
    }

    // at the first step or run: the manager and the model's prefill follow the switch together, or not at all
    void apply_page_release() {
        if (!paged) return;
        pages->set_page_release(release_pages ? options().window : 0, options().n_sink);
        paged->set_page_release(pages->page_release());
    }

    // EXTENSION: sampled decoding (mli_engine_add_item_sampled).  The parameters live here, keyed by item
    // id, so a preempted item keeps its stream; the decoder head reads them from per-slot device arrays, filled when an
    // item takes a slot.  The head is chosen once, at the first step or run: sampled if a queued item has T > 0.
    struct Sampling {
        float temperature = 0.f;
        int top_k = 0;
        float top_p = 1.f;
        unsigned long long seed = 0;
    };
    struct SlotArrays {  // [n_batch] each
        TensorFloat temperature, top_p;
        TensorInt top_k;
        Tensor<int64_t> seed;
        SlotArrays(size_t B, DeviceType d)
            : temperature({B}, d, TensorDataType::SYNC_ALLOCATE), top_p({B}, d, TensorDataType::SYNC_ALLOCATE),
              top_k({B}, d, TensorDataType::SYNC_ALLOCATE), seed({B}, d, TensorDataType::SYNC_ALLOCATE) {}
    };
    std::unordered_map<int, Sampling> sampling;
    int head = -1;  // -1 = not chosen yet, 0 = greedy (the existing heads), 1 = sampled
    std::unique_ptr<SlotArrays> slots_device, slots_host;
    SlotSampling slot_sampling{};

    Sampling sampling_of(int id) const {
        auto it = sampling.find(id);
        return it == sampling.end() ? Sampling{} : it->second;
    }

    // EXTENSION: per-token log-probabilities (mli_engine_set_logprobs).  The decoder layer owns the device
    // buffers; the figures cross to the host with decoder_result and are appended, keyed by item id, where the token is
    // appended to the item -- so a token dropped by a preemption takes its figures with it and a re-admitted item keeps
    // those of the tokens it already generated.
    struct Logprobs : ResultFigures {
        struct Record {
            int n_prompt = 0;
            std::vector<float> token_logprob, top_logprobs;
            std::vector<int> top_ids;
        };
        int n_top, n_rounds, width;
        TensorFloat token_device, top_device, token_host, top_host;  // shallow copies of the layer's / pinned mirrors
        TensorInt ids_device, ids_host;
        std::unordered_map<int, Record> records;

        explicit Logprobs(const DecoderLogprobs& d)
            : n_top(d.n_top), n_rounds(d.n_rounds), width(d.n_top > 0 ? d.n_top : 1), token_device(*d.token_logprob),
              top_device(*d.top_logprobs), token_host(d.token_logprob->shape(), DeviceType::HOST, TensorDataType::SYNC_ALLOCATE),
              top_host(d.top_logprobs->shape(), DeviceType::HOST, TensorDataType::SYNC_ALLOCATE), ids_device(*d.top_ids),
              ids_host(d.top_ids->shape(), DeviceType::HOST, TensorDataType::SYNC_ALLOCATE) {}

        void fetch(bool in_flight) override {
            if (in_flight) {
                token_host.copy_range_from_async(token_device, 0, token_host.get_total_size());
                if (n_top > 0) {
                    ids_host.copy_range_from_async(ids_device, 0, ids_host.get_total_size());
                    top_host.copy_range_from_async(top_device, 0, top_host.get_total_size());
                }
                return;
            }
            token_host.copy_from(token_device);
            if (n_top > 0) {
                ids_host.copy_from(ids_device);
                top_host.copy_from(top_device);
            }
        }

        void token(const IdTokensPair& item, int slot, int round) override {
            auto it = records.find(item.first);
            if (it == records.end()) {
                it = records.emplace(item.first, Record{}).first;
                it->second.n_prompt = (int)item.second.size() - 1;  // its first generated token has just been appended
            }
            Record& r = it->second;
            const size_t at = (size_t)slot * n_rounds + round;
            r.token_logprob.push_back(token_host.data()[at]);
            if (n_top > 0) {
                r.top_ids.insert(r.top_ids.end(), ids_host.data() + at * width, ids_host.data() + (at + 1) * width);
                r.top_logprobs.insert(r.top_logprobs.end(), top_host.data() + at * width, top_host.data() + (at + 1) * width);
            }
        }
    };
    // EXTENSION: prompt log-probabilities (mli_engine_set_prompt_logprobs).  The rows admitted for a forward are
    // noted here (admitted()); the model's layer calls score() directly behind their prefill, on the forward's stream.  The
    // prompts are cut into passes of at most n_batch positions (prompt_plan.hpp), each pass is one mli_paged_prompt_logprobs
    // call, and its figures cross to the host at once with a blocking copy -- a forward with new rows waits for its scoring,
    // every other forward is untouched -- and are kept per item id.  An id is noted once: a re-admitted item is not scored
    // again, and "prompt" is the tokens it was queued with.
    struct PromptLogprobs : PromptScoring {
        struct Record {
            std::vector<float> token_logprob, top_logprobs;
            std::vector<int> top_ids;
        };
        int n_top, width, limit;
        TensorInt seg_device, seg_host, ids_device, ids_host;       // segments: [4][limit]
        TensorFloat token_device, token_host, top_device, top_host, scratch;
        size_t scratch_bytes;
        std::vector<mli::PromptRow> pending;
        std::unordered_map<int, int> pending_id;                    // batch row -> item id
        std::unordered_map<int, Record> records;

        static std::vector<size_t> shape(size_t n) { return {n}; }
        PromptLogprobs(int n_top_, int n_batch, int emb_dim, int n_vocab)
            : n_top(n_top_), width(n_top_ > 0 ? n_top_ : 1), limit(n_batch),
              seg_device(shape(4 * (size_t)n_batch), DeviceType::DEVICE, TensorDataType::SYNC_ALLOCATE),
              seg_host(shape(4 * (size_t)n_batch), DeviceType::HOST, TensorDataType::SYNC_ALLOCATE),
              ids_device(shape((size_t)n_batch * width), DeviceType::DEVICE, TensorDataType::SYNC_ALLOCATE),
              ids_host(shape((size_t)n_batch * width), DeviceType::HOST, TensorDataType::SYNC_ALLOCATE),
              token_device(shape((size_t)n_batch), DeviceType::DEVICE, TensorDataType::SYNC_ALLOCATE),
              token_host(shape((size_t)n_batch), DeviceType::HOST, TensorDataType::SYNC_ALLOCATE),
              top_device(shape((size_t)n_batch * width), DeviceType::DEVICE, TensorDataType::SYNC_ALLOCATE),
              top_host(shape((size_t)n_batch * width), DeviceType::HOST, TensorDataType::SYNC_ALLOCATE),
              scratch(shape((mli_prompt_logprobs_scratch_bytes(n_batch, emb_dim, n_vocab) + 3) / 4), DeviceType::DEVICE,
                      TensorDataType::SYNC_ALLOCATE),
              scratch_bytes(mli_prompt_logprobs_scratch_bytes(n_batch, emb_dim, n_vocab)) {}

        // the item in batch row `row` has just been admitted with n_tokens tokens
        void admitted(int row, int id, int n_tokens) {
            if (!records.emplace(id, Record{}).second) return;      // scored at its first admission only
            pending.push_back(mli::PromptRow{row, n_tokens});
            pending_id[row] = id;
        }

        void score(int elem, const void* wq, const PagedAttentionOptions& o, void* const* page_table, const int* inp,
                   const float* emb_table, int n_batch, int n_sequence, int emb_dim, int n_vocab) override {
            if (pending.empty()) return;
            const int n_kv_heads = o.n_kv_heads != 0 ? o.n_kv_heads : o.n_heads;
            for (const mli::PromptPass& pass : mli::cut_prompt_passes(pending, limit)) {
                const int n_seg = (int)pass.segments.size();
                int* seg = seg_host.data();
                for (int i = 0; i < n_seg; ++i) {
                    seg[i] = pass.segments[i].row;
                    seg[limit + i] = pass.segments[i].first;
                    seg[2 * limit + i] = pass.segments[i].count;
                    seg[3 * limit + i] = pass.segments[i].offset;
                }
                seg_device.copy_from(seg_host);
                const int* d = seg_device.data();
                // (an engine with a cap scores its prompts under the model it decodes with: the capped prompt scan)
                const int rc = o.sink_logits
                    ? mli_paged_prompt_logprobs_sink_logits(   // (likewise with learned sink logits)
                          page_table, inp, wq, emb_table, d, d + limit, d + 2 * limit, d + 3 * limit, token_device.data(),
                          n_top > 0 ? ids_device.data() : nullptr, n_top > 0 ? top_device.data() : nullptr, n_seg, pass.max_count,
                          pass.n_positions, n_batch, n_sequence, emb_dim, n_vocab, o.n_heads, n_kv_heads, o.window, o.n_sink,
                          o.sink_logits->data(), elem, n_top, scratch.data(), scratch_bytes, mli::runtime::compute_stream())
                    : o.softcap != 0.f
                    ? mli_paged_prompt_logprobs_softcap(
                          page_table, inp, wq, emb_table, d, d + limit, d + 2 * limit, d + 3 * limit, token_device.data(),
                          n_top > 0 ? ids_device.data() : nullptr, n_top > 0 ? top_device.data() : nullptr, n_seg, pass.max_count,
                          pass.n_positions, n_batch, n_sequence, emb_dim, n_vocab, o.n_heads, n_kv_heads, o.window, o.n_sink,
                          o.softcap, elem, n_top, scratch.data(), scratch_bytes, mli::runtime::compute_stream())
                    : mli_paged_prompt_logprobs(
                    page_table, inp, wq, emb_table, d, d + limit, d + 2 * limit, d + 3 * limit, token_device.data(),
                    n_top > 0 ? ids_device.data() : nullptr, n_top > 0 ? top_device.data() : nullptr, n_seg, pass.max_count,
                    pass.n_positions, n_batch, n_sequence, emb_dim, n_vocab, o.n_heads, n_kv_heads, o.window, o.n_sink, elem,
                    n_top, scratch.data(), scratch_bytes, mli::runtime::compute_stream());
                if (rc != 0) throw std::runtime_error("mli_paged_prompt_logprobs failed: " + std::to_string(rc));
                token_host.copy_from(token_device);                  // blocking: the pass has run
                if (n_top > 0) {
                    ids_host.copy_from(ids_device);
                    top_host.copy_from(top_device);
                }
                for (const mli::PromptSegment& g : pass.segments) {
                    Record& r = records.at(pending_id.at(g.row));
                    r.token_logprob.insert(r.token_logprob.end(), token_host.data() + g.offset, token_host.data() + g.offset + g.count);
                    if (n_top > 0) {
                        const size_t a = (size_t)g.offset * width, b = (size_t)(g.offset + g.count) * width;
                        r.top_ids.insert(r.top_ids.end(), ids_host.data() + a, ids_host.data() + b);
                        r.top_logprobs.insert(r.top_logprobs.end(), top_host.data() + a, top_host.data() + b);
                    }
                }
            }
            pending.clear();
            pending_id.clear();
        }
    };
    bool prompt_logprobs_wanted = false;             // mli_engine_set_prompt_logprobs
    std::unique_ptr<PromptLogprobs> prompt_logprobs; // from the first step or run of an engine with the switch set

    // the rows admitted for the next forward (both loops): their prompts are scored in that forward
    void note_admitted(const std::vector<int>& slots) {
        if (!prompt_logprobs) return;
        for (int b : slots) {
            const IdTokensPair& item = processing_storage.get_token(b);
            prompt_logprobs->admitted(b, item.first, (int)item.second.size());
        }
    }
    bool prompt_shape_ok() {
        const PagedAttentionOptions& o = options();
        return mli::prompt_scan_shape_ok(cfg.n_batch, cfg.n_sequence, cfg.emb_dim, o.n_heads,
                                         o.n_kv_heads != 0 ? o.n_kv_heads : o.n_heads, elem());
    }

    int logprobs_n_top = -1;              // mli_engine_set_logprobs: -1 = never called
    std::unique_ptr<Logprobs> logprobs;   // from the first step or run of an engine with logprobs
    std::unordered_set<int> item_ids;     // every id queued so far
    bool duplicate_ids = false;

    void note_item_id(int id) {
        if (!item_ids.insert(id).second) {
            if (logprobs_n_top >= 0) throw std::invalid_argument("an engine with logprobs keys them by item id: duplicate id " + std::to_string(id));
            duplicate_ids = true;
        }
    }

    void choose_head() {
        if (head >= 0) return;
        head = 0;
        for (const auto& kv : sampling)
            if (kv.second.temperature > 0.f) head = 1;
        if (logprobs_n_top >= 0) head = 1;  // the figures come from materialised logits, for greedy items too
        if (!head) return;
        const size_t B = cfg.n_batch;
        slots_device = std::make_unique<SlotArrays>(B, DeviceType::DEVICE);
        slots_host = std::make_unique<SlotArrays>(B, DeviceType::HOST);
        for (size_t b = 0; b < B; ++b) set_slot_host((int)b, Sampling{});
        upload_slots();
        slot_sampling = {slots_device->temperature.data(), slots_device->top_k.data(), slots_device->top_p.data(),
                         slots_device->seed.data()};
        model_head().set_sampling(&slot_sampling);
        if (logprobs_n_top < 0) return;
        model_head().set_logprobs(logprobs_n_top);
        logprobs = std::make_unique<Logprobs>(model_head().logprobs());
        if (!prompt_logprobs_wanted) return;
        // (the setters that came after mli_engine_set_prompt_logprobs may have changed what it validated)
        if (!paged || release_pages || !prompt_shape_ok())
            throw std::runtime_error("prompt log-probabilities (mli_engine_set_prompt_logprobs): not with page release, and "
                                     "the prompt scan does not take this (n_batch, n_sequence, emb_dim, n_heads, n_kv_heads)");
        prompt_logprobs = std::make_unique<PromptLogprobs>(logprobs_n_top, cfg.n_batch, cfg.emb_dim, cfg.n_vocab);
        paged->set_prompt_logprobs(prompt_logprobs.get());
    }

    void set_slot_host(int b, const Sampling& s) {
        slots_host->temperature.data()[b] = s.temperature;
        slots_host->top_k.data()[b] = s.top_k;
        slots_host->top_p.data()[b] = s.top_p;
        slots_host->seed.data()[b] = (int64_t)s.seed;
    }

    void upload_slots() {
        slots_device->temperature.copy_from(slots_host->temperature);
        slots_device->top_k.copy_from(slots_host->top_k);
        slots_device->top_p.copy_from(slots_host->top_p);
        slots_device->seed.copy_from(slots_host->seed);
    }

    // sequential loop: after the whole-tensor insert, every slot's parameters in the same stream-ordered way
    void refresh_slots_sequential() {
        if (head != 1) return;
        for (int b = 0; b < cfg.n_batch; ++b)
            set_slot_host(b, processing_storage.batch_id_processing(b) ? sampling_of(processing_storage.get_token(b).first)
                                                                       : Sampling{});
        upload_slots();
    }

    // pipelined loop: the admitted slots only, by scatter (the other slots' items are in flight)
    void scatter_admitted(const std::vector<int>& slots) {
        if (head != 1 || slots.empty()) return;
        std::vector<long long> idx(slots.begin(), slots.end());
        std::vector<float> t, p;
        std::vector<int> k;
        std::vector<int64_t> s;
        for (int b : slots) {
            const Sampling v = sampling_of(processing_storage.get_token(b).first);
            t.push_back(v.temperature);
            k.push_back(v.top_k);
            p.push_back(v.top_p);
            s.push_back((int64_t)v.seed);
        }
        slots_device->temperature.scatter_from_host(idx.data(), t.data(), idx.size());
        slots_device->top_k.scatter_from_host(idx.data(), k.data(), idx.size());
        slots_device->top_p.scatter_from_host(idx.data(), p.data(), idx.size());
        slots_device->seed.scatter_from_host(idx.data(), s.data(), idx.size());
    }

    ~mli_engine() {
        if (stream) {
            mli::runtime::release_attention_scratch(stream);
            mli::runtime::destroy_stream(stream);
        }
    }

    // every entry point runs under this: device, stream and counter of THIS engine for the calling thread
    struct Scope {
        void* saved;
        bool saved_lean, saved_graphs, saved_sequential;
        explicit Scope(mli_engine* e)
            : saved(mli::runtime::compute_stream()), saved_lean(mli::runtime::lean_layers()),
              saved_graphs(mli::runtime::step_graphs()), saved_sequential(mli::runtime::sequential_engine_loop()) {
            mli::runtime::use_device(e->cfg.device);
            if (e->stream) mli::runtime::set_compute_stream(e->stream);
            mli::runtime::set_lean_layers(e->lean_layers);
            mli::runtime::set_step_graphs(e->step_graphs);
            set_thread_throughput_counter(&e->counter);
        }
        ~Scope() {
            mli::runtime::set_compute_stream(saved);
            mli::runtime::set_lean_layers(saved_lean);
            mli::runtime::set_step_graphs(saved_graphs);
            mli::runtime::set_sequential_engine_loop(saved_sequential);
            set_thread_throughput_counter(nullptr);
        }
    };

    mli_engine(const mli_engine_config& c, const float* emb, const float* pos, const float* wk, const float* wq,
               const float* wv)
        : cfg(c),
          emb_table(upload(emb, {(size_t)c.n_vocab, (size_t)c.emb_dim})),
          pos_table(upload(pos, {(size_t)c.n_sequence, (size_t)c.emb_dim})),
          inp_device({(size_t)c.n_batch, (size_t)c.n_sequence}, DeviceType::DEVICE),
          inp_host({(size_t)c.n_batch, (size_t)c.n_sequence}, DeviceType::HOST),
          lengths_device({(size_t)c.n_batch}, DeviceType::DEVICE), lengths_host({(size_t)c.n_batch}, DeviceType::HOST),
          new_idx_device({(size_t)c.n_batch}, DeviceType::DEVICE), new_idx_host({(size_t)c.n_batch}, DeviceType::HOST),
          result_device(result_shape(c), DeviceType::DEVICE), result_host(result_shape(c), DeviceType::HOST) {
        const size_t B = c.n_batch, S = c.n_sequence, D = c.emb_dim, V = c.n_vocab;
        const int R = c.n_forward_rounds;
        if (paged_kind()) {   // a block holds 16 x 3 x emb_dim elements of the kind's page element type
            pool = std::make_unique<MemoryBlockManager>(c.n_blocks, elem() == MLI_ELEM_FP8    ? fp8_page_block_floats(D)
                                                                    : elem() == MLI_ELEM_BF16 ? bf16_page_block_floats(D)
                                                                                              : (size_t)PAGE_BLOCK_SIZE * 3 * D);
            pages = std::make_unique<PagedAttentionsManager>(B, S, D);
        }
        if (elem() != MLI_ELEM_F32) {   // bf16 weights
            TensorBf16 dk = make_device_bf16(wk, {D, D}), dq = make_device_bf16(wq, {D, D}), dv = make_device_bf16(wv, {D, D});
            if (c.kind == MLI_ENGINE_PAGED_BF16)
                paged = std::make_unique<PagedAttentionBf16InferenceModel>(
                    PagedAttentionBf16Layer(std::move(dk), std::move(dq), std::move(dv), B, D, S), B, S, D, V, R);
            else
                paged = std::make_unique<PagedAttentionFp8InferenceModel>(
                    PagedAttentionFp8Layer(std::move(dk), std::move(dq), std::move(dv), B, D, S), B, S, D, V, R);
        } else {
            TensorFloat dk = upload(wk, {D, D}), dq = upload(wq, {D, D}), dv = upload(wv, {D, D});
            if (c.kind == MLI_ENGINE_CONTIGUOUS)
                naive_model = std::make_unique<InferenceModel>(
                    SelfAttentionLayer(std::move(dk), std::move(dq), std::move(dv), B, D, S), EncoderLayer(),
                    DecoderLayer(B, V), B, S, D);
            else if (c.kind == MLI_ENGINE_PAGED)
                paged = std::make_unique<PagedAttentionInferenceModel>(
                    PagedAttentionLayer(std::move(dk), std::move(dq), std::move(dv), B, D, S), PagedEncoderLayer(),
                    PagedDecoderLayer(B, V), B, S, D, R);
            else
                paged = std::make_unique<PagedAttentionCublasInferenceModel>(
                    PagedAttentionCublasLayer(std::move(dk), std::move(dq), std::move(dv), B, D, S), PagedEncoderLayer(),
                    PagedCublasDecoderLayer(B, V), B, S, D, R);
        }
        init_loop_tensors(B, S);
    }

    void init_loop_tensors(size_t B, size_t S) {
        std::memset(lengths_host.data(), 0, B * sizeof(int));
        std::memset(inp_host.data(), 0, B * S * sizeof(int));
        inp_device.copy_from(inp_host);
        lengths_device.copy_from(lengths_host);
    }

    static std::vector<size_t> result_shape(const mli_engine_config& c) {
        if (c.kind == MLI_ENGINE_CONTIGUOUS) return {(size_t)c.n_batch};
        return {(size_t)c.n_batch, (size_t)c.n_forward_rounds};
    }

    // one forward of whichever model the engine has
    void forward(const TensorInt& inp, TensorInt& lengths, const TensorInt& new_idx, TensorInt& result, int n_new) {
        if (paged)
            paged->forward(inp, lengths, new_idx, result, n_new, emb_table, pos_table, pages->get_page_table_device());
        else
            naive_model->forward(inp, lengths, new_idx, result, n_new, emb_table, pos_table);
    }

    void insert(const std::vector<int>& free_slots) {
        if (paged_kind()) {
            const std::vector<int> slots = insert_new_items(inp_device, inp_host, lengths_device, lengths_host, new_idx_device,
                                                            new_idx_host, item_storage, processing_storage, *pool, *pages,
                                                            cfg.n_forward_rounds);
            n_new_items = (int)slots.size();
            note_admitted(slots);
        } else {
            n_new_items = insert_new_items(free_slots, inp_device, inp_host, lengths_device, lengths_host,
                                           new_idx_device, new_idx_host, item_storage, processing_storage);
        }
    }

    void start() {
        if (pages) pages->set_length_reset_quirk(cfg.reference_length_reset_quirk != 0);
        apply_page_release();
        get_global_throughput_counter().reset();
        get_global_throughput_counter().start_record();
        std::vector<int> all(cfg.n_batch);
        std::iota(all.begin(), all.end(), 0);
        choose_head();
        insert(all);
        refresh_slots_sequential();
        started = true;
    }

    bool done() { return is_done(item_storage, processing_storage); }

    void run_pipelined() {
        if (started) throw std::runtime_error("pipelined run on an engine that has already been stepped");
        if (!paged_kind() || 2 * cfg.n_forward_rounds > PAGE_BLOCK_SIZE)
            throw std::runtime_error("the pipelined loop serves the paged kinds with n_forward_rounds <= PAGE_BLOCK_SIZE / 2");
        pages->set_length_reset_quirk(cfg.reference_length_reset_quirk != 0);
        apply_page_release();
        get_global_throughput_counter().reset();
        choose_head();
        started = true;
        iterations = run_paged_engine_pipelined(
            item_storage, processing_storage, *pool, *pages, cfg.n_batch, cfg.n_sequence,
            [&](const TensorInt& inp, TensorInt& lengths, const TensorInt& new_idx, TensorInt& result, int n_new) {
                forward(inp, lengths, new_idx, result, n_new);
            }, cfg.n_forward_rounds, [&](const std::vector<int>& slots) {
                scatter_admitted(slots);
                note_admitted(slots);
            }, logprobs.get());
    }

    double t_forward = 0, t_result = 0, t_pages = 0, t_insert = 0;  // host seconds per phase (MLI_ENGINE_TIMING=1)
    static double now() {
        return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }

    void step() {
        if (!started) start();
        if (done()) return;
        const double t0 = now();
        forward(inp_device, lengths_device, new_idx_device, result_device, n_new_items);
        const double t1 = now();
        std::vector<int> free_slots =
            process_decoder_result(result_device, result_host, item_storage, processing_storage, cfg.n_sequence,
                                   logprobs.get());
        const double t2 = now();
        if (paged_kind())
            allocate_or_free_memory_blocks_if_needed(*pages, *pool, processing_storage, item_storage, free_slots,
                                                     cfg.n_forward_rounds);
        const double t3 = now();
        insert(free_slots);
        refresh_slots_sequential();
        if (paged_kind() && processing_storage.size() == 0 && item_storage.new_count() > 0)
            throw std::runtime_error("paged engine: the page pool is too small for the next queued item");
        const double t4 = now();
        t_forward += t1 - t0; t_result += t2 - t1; t_pages += t3 - t2; t_insert += t4 - t3;
        ++iterations;
    }

    void fill(mli_engine_stats* s) {
        s->total_tokens = get_global_throughput_counter().total_tokens();
        s->seconds = get_global_throughput_counter().seconds();
        s->iterations = iterations;
        s->finished = item_storage.finish_count();
        s->waiting = item_storage.new_count();
        s->in_flight = processing_storage.size();
    }
};

#define MLI_GUARD(body)                                  \
    try {                                                \
        body;                                            \
        return 0;                                        \
    } catch (const std::exception& e) {                  \
        g_last_error = e.what();                         \
        return -1;                                       \
    } catch (...) {                                      \
        g_last_error = "unknown C++ exception";          \
        return -1;                                       \
    }

extern "C" {

void mli_engine_set_lean_layers(int enabled) { g_default_lean_layers.store(enabled != 0); }

void mli_engine_set_step_graphs(int enabled) { g_default_step_graphs.store(enabled != 0); }

int mli_engine_configure(mli_engine* e, int lean_layers, int step_graphs) {
    MLI_GUARD({
        if (e->started) throw std::runtime_error("mli_engine_configure after the engine has started");
        PagedAttentionOptions& o = e->options();
        if (o.sink_logits && lean_layers == 0)   // (named first: an engine with sink logits has two heads at least)
            throw std::runtime_error("attention-sink logits (mli_engine_set_sink_logits) have the lean compositions only");
        if (o.softcap != 0.f && lean_layers == 0)   // (named first: an engine with a cap has two heads at least)
            throw std::runtime_error("logit soft-capping (mli_engine_set_softcap) has the lean compositions only");
        if (o.n_heads > 1 && lean_layers == 0)   // refused before anything is changed
            throw std::runtime_error("multi-head attention (mli_engine_set_heads) has the lean compositions only");
        if (o.n_kv_heads != 0 && lean_layers == 0)
            throw std::runtime_error("grouped-query attention (mli_engine_set_kv_heads: n_kv_heads < n_heads) has the lean "
                                     "compositions only");
        if (o.window > 0 && o.window < e->cfg.n_sequence && lean_layers == 0)
            throw std::runtime_error("sliding-window attention (mli_engine_set_window) has the lean compositions only");
        if (o.alibi_slopes && lean_layers == 0)
            throw std::runtime_error("ALiBi (mli_engine_set_alibi) has the lean compositions only");
        if (o.rope_table && lean_layers == 0)
            throw std::runtime_error("RoPE (mli_engine_set_rope) has the lean compositions only");
        if (lean_layers >= 0) e->lean_layers = lean_layers != 0;
        if (step_graphs >= 0) e->step_graphs = step_graphs != 0;
        if (e->cfg.kind == MLI_ENGINE_PAGED_FP8 && !e->lean_layers)
            throw std::runtime_error("the fp8 engine has the lean compositions only");
    })
}

int mli_engine_set_heads(mli_engine* e, int n_heads) {
    MLI_GUARD({
        if (!e) throw std::runtime_error("null argument");
        PagedAttentionOptions& o = e->options();
        if (n_heads < 1) throw std::runtime_error("mli_engine_set_heads: n_heads must be >= 1");
        if (n_heads != o.n_heads) {
            if (e->started) throw std::runtime_error("mli_engine_set_heads after the engine has started");
            if (!e->heads_kind())
                throw std::runtime_error("mli_engine_set_heads: multi-head attention serves the fp32 and bf16 paged engines");
            if (n_heads > 1 && !e->lean_layers)
                throw std::runtime_error("mli_engine_set_heads: multi-head attention has the lean compositions only");
            const int elem = e->elem();
            if (n_heads > 1 && !mli::heads_shape_supported(e->cfg.n_batch, e->cfg.n_sequence, e->cfg.emb_dim, n_heads, elem))
                throw std::runtime_error("mli_engine_set_heads: unsupported (emb_dim, n_heads): head_dim must be 32, 64, 128 or "
                                         "256 and emb_dim at most 512 (fp32) / 1024 (bf16)");
            if (o.window > 0 && o.window < e->cfg.n_sequence &&
                !mli::window_shape_supported(e->cfg.n_batch, e->cfg.n_sequence, e->cfg.emb_dim, n_heads, elem))
                throw std::runtime_error("mli_engine_set_heads: the windowed scan (mli_engine_set_window) does not take this shape");
            if (o.n_kv_heads != 0 && n_heads % o.n_kv_heads != 0)
                throw std::runtime_error("mli_engine_set_heads: the stored n_kv_heads (mli_engine_set_kv_heads) does not divide "
                                         "n_heads");
            if (o.alibi_slopes)
                throw std::runtime_error("mli_engine_set_heads: the stored ALiBi slopes (mli_engine_set_alibi) are those of " +
                                         std::to_string(o.n_heads) + " heads");
            if (o.rope_table)
                throw std::runtime_error("mli_engine_set_heads: the stored rotary table (mli_engine_set_rope) is that of " +
                                         std::to_string(o.n_heads) + " heads");
            if (o.sink_logits)
                throw std::runtime_error("mli_engine_set_heads: the stored sink logits (mli_engine_set_sink_logits) are those of " +
                                         std::to_string(o.n_heads) + " heads");
            if (o.softcap != 0.f && n_heads < 2)
                throw std::runtime_error("mli_engine_set_heads: the stored cap (mli_engine_set_softcap) needs two heads at least");
            o.n_heads = n_heads;
        }
    })
}

// What is stored is a grouping: n_kv_heads < n_heads.  n_kv_heads == n_heads stores "as many as n_heads" (0), the state of an
// engine the call was never made on.  The shapes are the multi-head scan's, validated by set_heads / set_window.
int mli_engine_set_kv_heads(mli_engine* e, int n_kv_heads) {
    MLI_GUARD({
        if (!e) throw std::runtime_error("null argument");
        PagedAttentionOptions& o = e->options();
        if (n_kv_heads < 1) throw std::runtime_error("mli_engine_set_kv_heads: n_kv_heads must be >= 1");
        if (n_kv_heads > o.n_heads || o.n_heads % n_kv_heads != 0)
            throw std::runtime_error("mli_engine_set_kv_heads: n_kv_heads must divide the engine's n_heads (mli_engine_set_heads)");
        const int then = n_kv_heads == o.n_heads ? 0 : n_kv_heads;
        if (then != o.n_kv_heads) {
            if (e->started) throw std::runtime_error("mli_engine_set_kv_heads: n_kv_heads cannot change after the engine has started");
            if (then != 0) {
                // (n_heads > 1 here, so set_heads has accepted the kind, the lean layers and the shape; checked again all the same)
                if (!e->heads_kind())
                    throw std::runtime_error("mli_engine_set_kv_heads: n_kv_heads < n_heads serves the fp32 and bf16 paged engines");
                if (!e->lean_layers)
                    throw std::runtime_error("mli_engine_set_kv_heads: n_kv_heads < n_heads has the lean compositions only");
                if (!mli::gqa_shape_supported(e->cfg.n_batch, e->cfg.n_sequence, e->cfg.emb_dim, o.n_heads, n_kv_heads, e->elem()))
                    throw std::runtime_error("mli_engine_set_kv_heads: the scan does not take this (n_batch, n_sequence, emb_dim, "
                                             "n_heads, n_kv_heads)");
            }
            o.n_kv_heads = then;
        }
    })
}

// The slopes are stored with the option set (the layer owns the device copy).  The shapes are the multi-head scan's, which
// set_heads / set_kv_heads / set_window have validated; they are checked again here.
int mli_engine_set_alibi(mli_engine* e, const float* slopes_host, int n) {
    MLI_GUARD({
        if (!e) throw std::runtime_error("null argument");
        if (e->started) throw std::runtime_error("mli_engine_set_alibi after the engine has started");
        if (!e->heads_kind())
            throw std::runtime_error("mli_engine_set_alibi: ALiBi serves the fp32 and bf16 paged engines");
        PagedAttentionOptions& o = e->options();
        if (o.n_heads < 2)
            throw std::runtime_error("mli_engine_set_alibi: n_heads must be >= 2 (mli_engine_set_heads comes first; the "
                                     "single-head scans have no bias)");
        if (slopes_host != nullptr && n != o.n_heads)
            throw std::runtime_error("mli_engine_set_alibi: n must be the engine's n_heads (" + std::to_string(o.n_heads) + ")");
        if (!e->lean_layers) throw std::runtime_error("mli_engine_set_alibi: ALiBi has the lean compositions only");
        if (o.softcap != 0.f)
            throw std::runtime_error("mli_engine_set_alibi: not with logit soft-capping (mli_engine_set_softcap: no order of bias "
                                     "and cap is defined)");
        if (o.sink_logits)
            throw std::runtime_error("mli_engine_set_alibi: not with attention-sink logits (mli_engine_set_sink_logits: no model "
                                     "defines a sink logit beside a position bias)");
        if (e->prompt_logprobs_wanted)
            throw std::runtime_error("mli_engine_set_alibi: not with prompt log-probabilities (the prompt scan has no bias: the "
                                     "prompt would be scored under another model than the one that decodes)");
        std::vector<float> slopes((size_t)o.n_heads);
        if (slopes_host != nullptr) std::copy(slopes_host, slopes_host + o.n_heads, slopes.begin());
        else if (mli_alibi_slopes(o.n_heads, slopes.data()) != 0) throw std::runtime_error("mli_engine_set_alibi: mli_alibi_slopes");
        for (float s : slopes)
            if (!std::isfinite(s)) throw std::runtime_error("mli_engine_set_alibi: every slope must be finite");
        const int n_kv_heads = o.n_kv_heads != 0 ? o.n_kv_heads : o.n_heads;
        if (!mli::gqa_shape_supported(e->cfg.n_batch, e->cfg.n_sequence, e->cfg.emb_dim, o.n_heads, n_kv_heads, e->elem()))
            throw std::runtime_error("mli_engine_set_alibi: the scan does not take this (n_batch, n_sequence, emb_dim, n_heads, "
                                     "n_kv_heads)");
        mli::runtime::use_device(e->cfg.device);
        e->paged->set_alibi_slopes(slopes);
    })
}

// The cap is a field of the option set; the decode scan and the prompt scan of the engine read it there.  The shapes are the
// multi-head scan's, which set_heads / set_kv_heads / set_window have validated; they are checked again here.
int mli_engine_set_softcap(mli_engine* e, float cap) {
    MLI_GUARD({
        if (!e) throw std::runtime_error("null argument");
        if (e->started) throw std::runtime_error("mli_engine_set_softcap after the engine has started");
        if (!e->heads_kind())
            throw std::runtime_error("mli_engine_set_softcap: logit soft-capping serves the fp32 and bf16 paged engines");
        if (!std::isfinite(cap) || cap < 0.f)
            throw std::runtime_error("mli_engine_set_softcap: the cap must be finite and >= 0 (0: none)");
        PagedAttentionOptions& o = e->options();
        if (cap != 0.f) {
            if (o.n_heads < 2)
                throw std::runtime_error("mli_engine_set_softcap: n_heads must be >= 2 (mli_engine_set_heads comes first; the "
                                         "single-head scans have no cap)");
            if (!e->lean_layers)
                throw std::runtime_error("mli_engine_set_softcap: logit soft-capping has the lean compositions only");
            if (o.alibi_slopes)
                throw std::runtime_error("mli_engine_set_softcap: not with ALiBi (mli_engine_set_alibi: no order of bias and cap "
                                         "is defined)");
            if (o.sink_logits)
                throw std::runtime_error("mli_engine_set_softcap: not with attention-sink logits (mli_engine_set_sink_logits: no "
                                         "model defines a sink logit beside a cap)");
            const int n_kv_heads = o.n_kv_heads != 0 ? o.n_kv_heads : o.n_heads;
            if (!mli::gqa_shape_supported(e->cfg.n_batch, e->cfg.n_sequence, e->cfg.emb_dim, o.n_heads, n_kv_heads, e->elem()))
                throw std::runtime_error("mli_engine_set_softcap: the scan does not take this (n_batch, n_sequence, emb_dim, "
                                         "n_heads, n_kv_heads)");
        }
        e->paged->set_softcap(cap);
    })
}

// The logits are stored with the option set (the layer owns the device copy, whose address a captured step graph replays); the
// decode scan and the prompt scan of the engine read them there.  logits_host null: the switch is turned off again.
int mli_engine_set_sink_logits(mli_engine* e, const float* logits_host, int n) {
    MLI_GUARD({
        if (!e) throw std::runtime_error("null argument");
        if (e->started) throw std::runtime_error("mli_engine_set_sink_logits after the engine has started");
        if (!e->heads_kind())
            throw std::runtime_error("mli_engine_set_sink_logits: attention-sink logits serve the fp32 and bf16 paged engines");
        PagedAttentionOptions& o = e->options();
        if (logits_host != nullptr) {
            if (o.n_heads < 2)
                throw std::runtime_error("mli_engine_set_sink_logits: n_heads must be >= 2 (mli_engine_set_heads comes first; the "
                                         "single-head scans have no sink logit)");
            if (n != o.n_heads)
                throw std::runtime_error("mli_engine_set_sink_logits: n must be the engine's n_heads (" + std::to_string(o.n_heads) +
                                         ")");
            for (int h = 0; h < n; ++h)
                if (std::isnan(logits_host[h]) || logits_host[h] == INFINITY)
                    throw std::runtime_error("mli_engine_set_sink_logits: every logit must be finite or -inf (NaN and +inf are "
                                             "refused)");
            if (!e->lean_layers)
                throw std::runtime_error("mli_engine_set_sink_logits: attention-sink logits have the lean compositions only");
            if (o.alibi_slopes)
                throw std::runtime_error("mli_engine_set_sink_logits: not with ALiBi (mli_engine_set_alibi: no model defines a sink "
                                         "logit beside a position bias)");
            if (o.softcap != 0.f)
                throw std::runtime_error("mli_engine_set_sink_logits: not with logit soft-capping (mli_engine_set_softcap: no model "
                                         "defines a sink logit beside a cap)");
            const int n_kv_heads = o.n_kv_heads != 0 ? o.n_kv_heads : o.n_heads;
            if (!mli::gqa_shape_supported(e->cfg.n_batch, e->cfg.n_sequence, e->cfg.emb_dim, o.n_heads, n_kv_heads, e->elem()))
                throw std::runtime_error("mli_engine_set_sink_logits: the scan does not take this (n_batch, n_sequence, emb_dim, "
                                         "n_heads, n_kv_heads)");
            mli::runtime::use_device(e->cfg.device);
        }
        e->paged->set_sink_logits(logits_host, logits_host != nullptr ? n : 0);
    })
}

// The table is stored with the option set (the layer owns the device copy); table_host null: the standard table of theta.
static void engine_set_rope(mli_engine* e, const char* who, double theta, const float* table_host, size_t n_floats) {
    const std::string name(who);
    if (!e) throw std::runtime_error("null argument");
    if (e->started) throw std::runtime_error(name + " after the engine has started");
    if (!e->paged_kind()) throw std::runtime_error(name + ": RoPE serves the paged engines");
    if (!e->lean_layers) throw std::runtime_error(name + ": RoPE has the lean compositions only");
    if (e->prompt_logprobs_wanted)
        throw std::runtime_error(name + ": not with prompt log-probabilities (the prompt scan's q is not rotated: the prompt "
                                 "would be scored under another model than the one that decodes)");
    PagedAttentionOptions& o = e->options();
    const int H = o.n_heads > 0 ? o.n_heads : 1;
    if (e->cfg.emb_dim % H != 0 || (e->cfg.emb_dim / H) % 2 != 0)
        throw std::runtime_error(name + ": head_dim = emb_dim / n_heads must be an even integer");
    const size_t want = (size_t)e->cfg.n_sequence * (size_t)(e->cfg.emb_dim / H);
    std::vector<float> table(want);
    if (table_host != nullptr) {
        if (n_floats != want)
            throw std::runtime_error(name + ": n_floats must be n_sequence * head_dim (" + std::to_string(want) + ")");
        std::copy(table_host, table_host + want, table.begin());
    } else if (mli_rope_table(e->cfg.n_sequence, e->cfg.emb_dim / H, theta, table.data()) != 0) {
        throw std::runtime_error(name + ": theta must be finite and > 0");
    }
    for (float t : table)
        if (!std::isfinite(t)) throw std::runtime_error(name + ": every entry must be finite");
    mli::runtime::use_device(e->cfg.device);
    e->paged->set_rope_table(table);
}

int mli_engine_set_rope(mli_engine* e, double theta) {
    MLI_GUARD({ engine_set_rope(e, "mli_engine_set_rope", theta, nullptr, 0); })
}

int mli_engine_set_rope_table(mli_engine* e, const float* table_host, size_t n_floats) {
    MLI_GUARD({
        if (e && !table_host) throw std::runtime_error("null argument");
        engine_set_rope(e, "mli_engine_set_rope_table", 0.0, table_host, n_floats);
    })
}

int mli_engine_set_window(mli_engine* e, int window) {
    MLI_GUARD({
        if (!e) throw std::runtime_error("null argument");
        PagedAttentionOptions& o = e->options();
        if (window < 1) throw std::runtime_error("mli_engine_set_window: window must be >= 1");
        // what counts is the window the scan would see: n_sequence or more is none, accepted everywhere, changing nothing
        const int S = e->cfg.n_sequence;
        const int now = o.window > 0 && o.window < S ? o.window : S;
        const int then = window < S ? window : S;
        if (then != now) {
            if (!e->paged_kind())
                throw std::runtime_error("mli_engine_set_window: sliding-window attention serves the paged engines");
            if (e->started) throw std::runtime_error("mli_engine_set_window after the engine has started");
            if (then < S) {
                if (!e->lean_layers)
                    throw std::runtime_error("mli_engine_set_window: sliding-window attention has the lean compositions only");
                if (!mli::window_shape_supported(e->cfg.n_batch, S, e->cfg.emb_dim, o.n_heads, e->elem()))
                    throw std::runtime_error("mli_engine_set_window: the windowed scan does not take this (n_batch, n_sequence, "
                                             "emb_dim, n_heads)");
            }
            o.window = then;
        }
    })
}

// Sinks ride on the window: the shapes are the windowed scan's (validated by set_window / set_heads, with or without sinks),
// and without an effective window the layers ignore the value.
int mli_engine_set_sinks(mli_engine* e, int n_sink) {
    MLI_GUARD({
        if (!e) throw std::runtime_error("null argument");
        PagedAttentionOptions& o = e->options();
        if (n_sink < 0) throw std::runtime_error("mli_engine_set_sinks: n_sink must be >= 0");
        if (!e->paged_kind())
            throw std::runtime_error("mli_engine_set_sinks: attention sinks serve the paged engines");
        if (n_sink != o.n_sink) {
            if (e->started) throw std::runtime_error("mli_engine_set_sinks after the engine has started");
            if (!e->lean_layers)
                throw std::runtime_error("mli_engine_set_sinks: attention sinks have the lean compositions only");
            o.n_sink = n_sink;
        }
    })
}

// Release rides on the window as the sinks do: the switch is kept and read at the first step or run, so it combines with
// set_window / set_sinks / set_heads in any order, and without an effective window nothing changes.
int mli_engine_set_page_release(mli_engine* e, int enabled) {
    MLI_GUARD({
        if (!e) throw std::runtime_error("null argument");
        if (!e->paged_kind())
            throw std::runtime_error("mli_engine_set_page_release: early page release serves the paged engines");
        if (e->started) throw std::runtime_error("mli_engine_set_page_release after the engine has started");
        if (e->cfg.reference_length_reset_quirk)
            throw std::runtime_error("mli_engine_set_page_release: not with reference_length_reset_quirk (it moves device "
                                     "lengths backwards; release rests on lengths that only grow)");
        if (enabled && e->prompt_logprobs_wanted)
            throw std::runtime_error("mli_engine_set_page_release: not with prompt log-probabilities (a prefill that skips dead "
                                     "pages leaves the prompt's K / V incomplete)");
        e->release_pages = enabled != 0;
    })
}

int mli_engine_get_page_stats(mli_engine* e, mli_engine_page_stats* out) {
    MLI_GUARD({
        if (!e || !out) throw std::runtime_error("null argument");
        if (!e->pool || !e->pages) throw std::runtime_error("mli_engine_get_page_stats: the contiguous engine has no page pool");
        out->pool_pages = e->pool->pool_pages();
        out->in_use = e->pool->pages_in_use();
        out->peak_in_use = e->pool->peak_pages_in_use();
        out->released_early = e->pages->pages_released_early();
        out->preemptions = e->pages->preemptions();
    })
}

const char* mli_engine_last_error(void) { return g_last_error.c_str(); }

int mli_engine_create(const mli_engine_config* c, const float* emb_table, const float* pos_table, const float* wk,
                      const float* wq, const float* wv, mli_engine** out) {
    if (!c || !out || !emb_table || !pos_table || !wk || !wq || !wv) { g_last_error = "null argument"; return -1; }
    if (c->kind < 0 || c->kind > MLI_ENGINE_PAGED_FP8 || (c->kind == MLI_ENGINE_PAGED_BF16 && c->emb_dim % 8) ||
        (c->kind == MLI_ENGINE_PAGED_FP8 && (c->emb_dim % 16 || c->emb_dim > 2048)) || c->n_batch <= 0 || c->n_sequence <= 0 || c->emb_dim <= 0 || c->emb_dim % 4 ||
        c->n_vocab <= EOF_TOKEN_ID ||
        (c->kind != MLI_ENGINE_CONTIGUOUS && (c->n_sequence % PAGE_BLOCK_SIZE || c->n_blocks <= 0 ||
                                              c->n_forward_rounds < 1 || c->n_forward_rounds > PAGE_BLOCK_SIZE)) ||
        (c->kind == MLI_ENGINE_CONTIGUOUS && c->n_sequence % 4)) {
        g_last_error = "invalid engine configuration";
        return -1;
    }
    MLI_GUARD({
        mli::runtime::use_device(c->device);
        *out = new mli_engine(*c, emb_table, pos_table, wk, wq, wv);
    })
}

void mli_engine_destroy(mli_engine* e) {
    if (e && std::getenv("MLI_ENGINE_TIMING") && e->iterations && e->t_forward > 0)
        std::fprintf(stderr, "[mli engine] %lld iterations; host us/iteration: launch forward %.1f, wait + process "
                     "decoder result %.1f, page bookkeeping %.1f, insert + uploads %.1f\n", e->iterations,
                     1e6 * e->t_forward / e->iterations, 1e6 * e->t_result / e->iterations,
                     1e6 * e->t_pages / e->iterations, 1e6 * e->t_insert / e->iterations);
    delete e;
}

int mli_engine_add_item(mli_engine* e, int id, const int* tokens, int n_tokens) {
    if (!e || !tokens || n_tokens <= 0 || n_tokens + 1 > e->cfg.n_sequence) { g_last_error = "bad item"; return -1; }
    MLI_GUARD({
        e->note_item_id(id);
        e->item_storage.add_new_item(std::make_pair(id, std::vector<int>(tokens, tokens + n_tokens)));
    })
}

int mli_engine_add_item_sampled(mli_engine* e, int id, const int* tokens, int n_tokens, float temperature, int top_k,
                                float top_p, unsigned long long seed) {
    if (!e || !tokens || n_tokens <= 0 || n_tokens + 1 > e->cfg.n_sequence) { g_last_error = "bad item"; return -1; }
    MLI_GUARD({
        if (!(temperature >= 0.f) || !std::isfinite(temperature))
            throw std::invalid_argument("sampled item: temperature must be finite and >= 0");
        if (top_k < 0) throw std::invalid_argument("sampled item: top_k must be >= 0");
        if (!(top_p > 0.f && top_p <= 1.f)) throw std::invalid_argument("sampled item: top_p must lie in (0, 1]");
        if (e->cfg.reference_length_reset_quirk)
            throw std::invalid_argument("sampled items and the reference's length-reset quirk exclude each other (its "
                                        "length resets replay positions)");
        if (e->sampling.count(id)) throw std::invalid_argument("sampled item: duplicate id " + std::to_string(id));
        if (e->head == 0 && temperature > 0.f)
            throw std::runtime_error("this engine chose the greedy head at its first step: a sampled item (temperature "
                                     "> 0) must be queued before the first step or run");
        e->note_item_id(id);
        e->item_storage.add_new_item(std::make_pair(id, std::vector<int>(tokens, tokens + n_tokens)));
        mli_engine::Sampling params;
        params.temperature = temperature;
        params.top_k = top_k;
        params.top_p = top_p;
        params.seed = seed;
        e->sampling[id] = params;
    })
}

int mli_engine_set_logprobs(mli_engine* e, int n_top) {
    MLI_GUARD({
        if (!e) throw std::runtime_error("null argument");
        if (n_top < 0 || n_top > MLI_MAX_TOP_LOGPROBS)
            throw std::invalid_argument("mli_engine_set_logprobs: n_top must lie in 0 .. " + std::to_string(MLI_MAX_TOP_LOGPROBS));
        if (e->started) throw std::runtime_error("mli_engine_set_logprobs after the engine has started");
        if (e->cfg.reference_length_reset_quirk)
            throw std::invalid_argument("mli_engine_set_logprobs: not with reference_length_reset_quirk (the sampled head, "
                                        "which reports the figures, and the quirk exclude each other)");
        if (e->duplicate_ids)
            throw std::invalid_argument("mli_engine_set_logprobs: the figures are keyed by item id, and an id was queued twice");
        e->logprobs_n_top = n_top;
    })
}

int mli_engine_get_finished_logprobs(mli_engine* e, int index, int* n_prompt, float* token_logprobs, int capacity,
                                     int* n_generated, int* top_ids, float* top_logprobs, int top_capacity) {
    MLI_GUARD({
        if (!e || !n_prompt || !n_generated) throw std::runtime_error("null argument");
        if (e->logprobs_n_top < 0) throw std::runtime_error("mli_engine_get_finished_logprobs: an engine without logprobs "
                                                            "(mli_engine_set_logprobs)");
        const auto& items = e->item_storage.get_finished_items();
        if (index < 0 || index >= (int)items.size()) throw std::out_of_range("finished item index");
        const int id = std::next(items.begin(), index)->first;
        if (!e->logprobs || !e->logprobs->records.count(id)) throw std::runtime_error("no figures for item " + std::to_string(id));
        const auto& r = e->logprobs->records.at(id);
        *n_prompt = r.n_prompt;
        *n_generated = (int)r.token_logprob.size();
        if (token_logprobs && capacity > 0)
            std::memcpy(token_logprobs, r.token_logprob.data(), sizeof(float) * std::min<size_t>(capacity, r.token_logprob.size()));
        const size_t n = top_capacity > 0 ? std::min<size_t>(top_capacity, r.top_ids.size()) : 0;
        if (top_ids && n) std::memcpy(top_ids, r.top_ids.data(), sizeof(int) * n);
        if (top_logprobs && n) std::memcpy(top_logprobs, r.top_logprobs.data(), sizeof(float) * n);
    })
}

int mli_engine_set_prompt_logprobs(mli_engine* e, int enabled) {
    MLI_GUARD({
        if (!e) throw std::runtime_error("null argument");
        if (e->started) throw std::runtime_error("mli_engine_set_prompt_logprobs after the engine has started");
        if (e->logprobs_n_top < 0)
            throw std::runtime_error("mli_engine_set_prompt_logprobs: an engine without logprobs (mli_engine_set_logprobs comes "
                                     "first: it supplies n_top)");
        if (e->cfg.kind == MLI_ENGINE_CONTIGUOUS || e->cfg.kind == MLI_ENGINE_PAGED_FP8)
            throw std::runtime_error("mli_engine_set_prompt_logprobs: prompt log-probabilities serve the fp32 and bf16 paged "
                                     "engines");
        if (e->release_pages)
            throw std::runtime_error("mli_engine_set_prompt_logprobs: not with page release (mli_engine_set_page_release: its "
                                     "prefill skips dead pages, so the prompt's K / V are not all there)");
        if (enabled && e->options().alibi_slopes)
            throw std::runtime_error("mli_engine_set_prompt_logprobs: not with ALiBi (mli_engine_set_alibi: the prompt scan has "
                                     "no bias, so the prompt would be scored under another model than the one that decodes)");
        if (enabled && e->options().rope_table)
            throw std::runtime_error("mli_engine_set_prompt_logprobs: not with RoPE (mli_engine_set_rope: the prompt scan's q is "
                                     "not rotated, so the prompt would be scored under another model than the one that decodes)");
        if (!e->prompt_shape_ok())
            throw std::runtime_error("mli_engine_set_prompt_logprobs: the prompt scan does not take this (n_batch, n_sequence, "
                                     "emb_dim, n_heads, n_kv_heads): rows of at most two 16-byte lane loads");
        e->prompt_logprobs_wanted = enabled != 0;
    })
}

int mli_engine_get_finished_prompt_logprobs(mli_engine* e, int index, float* token_logprobs, int capacity, int* n_scored,
                                            int* top_ids, float* top_logprobs, int top_capacity) {
    MLI_GUARD({
        if (!e || !n_scored) throw std::runtime_error("null argument");
        if (!e->prompt_logprobs_wanted)
            throw std::runtime_error("mli_engine_get_finished_prompt_logprobs: an engine without prompt log-probabilities "
                                     "(mli_engine_set_prompt_logprobs)");
        const auto& items = e->item_storage.get_finished_items();
        if (index < 0 || index >= (int)items.size()) throw std::out_of_range("finished item index");
        const int id = std::next(items.begin(), index)->first;
        if (!e->prompt_logprobs || !e->prompt_logprobs->records.count(id))
            throw std::runtime_error("no prompt figures for item " + std::to_string(id));
        const auto& r = e->prompt_logprobs->records.at(id);
        *n_scored = (int)r.token_logprob.size();
        if (token_logprobs && capacity > 0)
            std::memcpy(token_logprobs, r.token_logprob.data(), sizeof(float) * std::min<size_t>(capacity, r.token_logprob.size()));
        const size_t n = top_capacity > 0 ? std::min<size_t>(top_capacity, r.top_ids.size()) : 0;
        if (top_ids && n) std::memcpy(top_ids, r.top_ids.data(), sizeof(int) * n);
        if (top_logprobs && n) std::memcpy(top_logprobs, r.top_logprobs.data(), sizeof(float) * n);
    })
}

int mli_engine_use_private_stream(mli_engine* e) {
    MLI_GUARD({
        mli::runtime::use_device(e->cfg.device);
        if (!e->stream) e->stream = mli::runtime::create_stream();
    })
}

int mli_engine_set_pipelined(mli_engine* e, int enabled) {
    MLI_GUARD({
        if (e->started) throw std::runtime_error("set_pipelined after the engine has started");
        e->pipelined = enabled != 0 ? 1 : 0;
    })
}

int mli_engine_step(mli_engine* e, int* done) {
    MLI_GUARD({
        if (e->pipelined == 1) throw std::runtime_error("a pipelined engine is run to completion (mli_engine_run)");
        mli_engine::Scope scope(e);
        e->step();
        if (done) *done = e->done() ? 1 : 0;
    })
}

int mli_engine_run(mli_engine* e, mli_engine_stats* stats) {
    MLI_GUARD({
        mli_engine::Scope scope(e);
        if (e->use_pipelined()) {
            e->run_pipelined();
        } else {
            if (!e->started) e->start();
            while (!e->done()) e->step();
        }
        if (stats) e->fill(stats);
    })
}

int mli_engine_get_stats(mli_engine* e, mli_engine_stats* stats) {
    MLI_GUARD({
        mli_engine::Scope scope(e);
        e->fill(stats);
    })
}

int mli_engine_decoder_result(mli_engine* e, void** device_ptr, int* count) {
    MLI_GUARD({
        *device_ptr = e->result_device.data();
        *count = (int)e->result_device.get_total_size();
    })
}

int mli_engine_stream(mli_engine* e, void** stream) {
    MLI_GUARD({
        if (!e || !stream) throw std::runtime_error("null argument");
        *stream = e->stream;
    })
}

int mli_engine_get_finished(mli_engine* e, int index, int* id, int* tokens, int capacity, int* n_tokens) {
    MLI_GUARD({
        const auto& items = e->item_storage.get_finished_items();
        if (index < 0 || index >= (int)items.size()) throw std::out_of_range("finished item index");
        auto it = std::next(items.begin(), index);
        *id = it->first;
        *n_tokens = (int)it->second.size();
        if (tokens) std::memcpy(tokens, it->second.data(), sizeof(int) * std::min<size_t>(capacity, it->second.size()));
    })
}

}  // extern "C"
