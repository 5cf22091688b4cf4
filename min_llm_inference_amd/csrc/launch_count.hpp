// Per-thread launch counters (mli_launch_count / mli_launch_counts_reset, include/mli_kernels.h): which branch of a launcher
// a call took, recorded on the host where the kernel is enqueued.  Host code only -- no kernel reads or writes them.  The
// scope is the tuning knobs' (thread_local): an engine runs in its caller's thread, so the caller reads what its engine ran.
#pragma once

#include <cstdint>
#include <cstring>

namespace mli {

// One entry per launcher branch; kLaunchFamilyNames (below) holds the ABI names in this order.
enum LaunchFamily {
    kLfGemmF32Panel,      // proj_gemm_panel.hip: the latency-shaped 32x32 kernel
    kLfGemmF32Rows64,     // proj_gemm.hip: 64-row tiles, one wave loads and multiplies (float4 and scalar-load forms)
    kLfGemmF32Rows64Split,  // ... loader waves + MFMA waves (512 threads)
    kLfGemmF32Rows128,    // ... 128-row tiles
    kLfGemmBf16Widened,   // bf16 pages through the fp32 MFMA kernel ("bf16_native_mfma" 0)
    kLfGemmBf16Rows64,    // proj_gemm_bf16.hip (bf16 and fp8 pages): 64-row tiles, 32 k per stage
    kLfGemmBf16Deep,      // ... 64-row tiles, 128 k per stage
    kLfGemmBf16Rows128,   // ... 128-row tiles
    kLfGemmBf16Dma,       // ... the LDS-DMA loader-wave / MFMA-wave projection
    kLfGemmBf16Fill,      // ... the prefill fill of bf16 / fp8 pages
    kLfLatestCompact,     // a decode projection launched over the compacted list of non-empty rows (beside its kernel's family)
    kLfFillFlat,          // a prefill fill launched over the flat (new row, token) list (beside its kernel's family)
    kLfFillPerRow,        // ... over one tile grid per new row
    kLfPrefillFused,      // mli_[paged_]prefill[_window]: the encoder as the fill's prologue
    kLfPrefillTwoLaunch,  // ... encoder + fill
    kLfScanEqualShares,   // attention_stream.hip
    kLfScanChunked,       // attention_fused.hip: the single-head lean / materialising chunked scan, every grid form
    kLfScanRowsOrdered,   // ... of them, the one-workgroup-per-row grids that take the rows longest first
    kLfScanRowsGridOrder, // ... and those in grid order
    kLfScanHeadsWindow,   // attention_heads.hpp / attention_window.hpp: several heads, a window, sinks, grouped heads
    kLfScanPrompt,        // attention_prompt.hpp: the causal multi-query scan over prompt positions
    kLfScanHeadsAlibi,    // attention_alibi.hpp: the multi-head scans with a linear position bias per query head
    kLfGemmF32Rope,       // proj_gemm.hip: a tiled fp32-MFMA form with rotary position embeddings (beside that form's family)
    kLfGemmBf16Rope,      // proj_gemm_bf16.hip: a tiled bf16-MFMA form with rotary position embeddings (beside that form's family)
    kLfScanHeadsSoftcap,  // attention_softcap.hpp: the multi-head scans with logit soft-capping
    kLfScanPromptSoftcap, // attention_prompt.hpp: the prompt scan with logit soft-capping
    kLfScanHeadsSinkLogits,   // attention_sink_logits.hpp: the multi-head scans with a learned sink logit per query head
    kLfScanPromptSinkLogits,  // attention_prompt.hpp: the prompt scan with a learned sink logit per query head
    kLaunchFamilies
};

constexpr const char* kLaunchFamilyNames[kLaunchFamilies] = {
    "gemm_f32_panel",  "gemm_f32_rows64",   "gemm_f32_rows64_split", "gemm_f32_rows128",  "gemm_bf16_widened",
    "gemm_bf16_rows64", "gemm_bf16_deep",   "gemm_bf16_rows128",     "gemm_bf16_dma",     "gemm_bf16_fill",
    "latest_compact",  "fill_flat",         "fill_per_row",          "prefill_fused",     "prefill_two_launch",
    "scan_equal_shares", "scan_chunked",    "scan_rows_ordered",     "scan_rows_grid_order", "scan_heads_window",
    "scan_prompt",     "scan_heads_alibi",  "gemm_f32_rope",         "gemm_bf16_rope",    "scan_heads_softcap",
    "scan_prompt_softcap", "scan_heads_sink_logits", "scan_prompt_sink_logits",
};

inline thread_local uint64_t g_launch_counts[kLaunchFamilies] = {};

inline void count_launch(LaunchFamily f) { ++g_launch_counts[f]; }

inline int launch_family_of(const char* name) {
    if (name == nullptr) return -1;
    for (int i = 0; i < kLaunchFamilies; ++i)
        if (std::strcmp(name, kLaunchFamilyNames[i]) == 0) return i;
    return -1;
}

}  // namespace mli
