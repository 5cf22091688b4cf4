// The causal multi-query prompt scan over bf16 pages: attention_prompt.hpp has the kernel, the launcher and the account.
#include "attention_prompt.hpp"

namespace mli {
template int launch_prompt_scan<ElemBF16>(const float*, const void* const*, const int*, const int*, const int*, const int*, float*,
                                          int, int, int, int, int, int, int, int, int, int, int, hipStream_t);
template int launch_prompt_softcap_scan<ElemBF16>(const float*, const void* const*, const int*, const int*, const int*, const int*,
                                                  float*, int, int, int, int, int, int, int, int, int, int, int, float, hipStream_t);
template int launch_prompt_sink_logits_scan<ElemBF16>(const float*, const void* const*, const int*, const int*, const int*,
                                                      const int*, float*, int, int, int, int, int, int, int, int, int, int, int,
                                                      const float*, hipStream_t);
}
