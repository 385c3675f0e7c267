// The v3 decode GEMV's instantiations WITHOUT the run-time flag paths (FL = false): the decode engine's plain launches.
// Also the home of the compile-time-K instances of the engine's Llama-2 launches (gemv_v3_dispatch.h: V3_CTK), which exist in this
// half only.  A translation unit of its own so that the two halves of the instantiation set compile in parallel (gemv_v3_dispatch.h).
#include "gemv_v3_dispatch.h"

namespace qeft {

hipError_t gemv_v3_dispatch_plain(const V3Args& a, const V3Plan& p, hipStream_t st) {
    return p.bits == 3 ? launch_b<3, V3_FAM_PLAIN>(a, p, st) : launch_b<4, V3_FAM_PLAIN>(a, p, st);
}

}  // namespace qeft
