// The single-head paged decode scan under a window over fp8 pages: attention_window.hpp has the kernel, the launcher and
// the account.
#include "attention_window.hpp"

namespace mli {
template int launch_window_decode<ElemFP8>(const float*, const void* const*, const int*, float*, int, int, int, ScanKind, int, int,
                                           void*, size_t, hipStream_t);
}
