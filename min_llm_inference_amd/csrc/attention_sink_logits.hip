// The multi-head paged decode scan with learned attention-sink logits over fp32 pages: attention_sink_logits.hpp has the account,
// attention_heads.hpp the kernel.
#include "attention_sink_logits.hpp"

namespace mli {
template int launch_heads_sink_logits_scan<ElemF32>(const float*, const void* const*, const int*, float*, int, int, int, int, int,
                                                    int, ScanKind, int, int, const float*, void*, size_t, hipStream_t);
}
