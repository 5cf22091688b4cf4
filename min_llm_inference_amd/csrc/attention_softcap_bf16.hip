// The multi-head paged decode scan with logit soft-capping over bf16 pages: attention_softcap.hpp has the account,
// attention_heads.hpp the kernel.
#include "attention_softcap.hpp"

namespace mli {
template int launch_heads_softcap_scan<ElemBF16>(const float*, const void* const*, const int*, float*, int, int, int, int, int, int,
                                                 ScanKind, int, int, float, void*, size_t, hipStream_t);
}
