// The multi-head paged decode scan over bf16 pages: attention_heads.hpp has the kernel, the launcher and the account.
#include "attention_heads.hpp"

namespace mli {
template int launch_heads_scan<ElemBF16>(const float*, const void* const*, const int*, float*, int, int, int, int, int, int, ScanKind,
                                         int, int, void*, size_t, hipStream_t);
}
