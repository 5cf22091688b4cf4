// The multi-head paged decode scan with ALiBi over fp32 pages: attention_alibi.hpp has the account, attention_heads.hpp the kernel.
#include "attention_alibi.hpp"

namespace mli {
template int launch_heads_alibi_scan<ElemF32>(const float*, const void* const*, const int*, float*, int, int, int, int, int, int,
                                              ScanKind, int, int, const float*, void*, size_t, hipStream_t);
}
