// hvx_restricted_wide4.hip -- the one-launch restricted exact scan with a result list of 4 registers per lane: 65 <= k <= 256
// (hvx_restricted_direct.h has the kernel, hvx_restricted_exact.hip the story and the dispatch).
#include "hvx_restricted_direct.h"

hipError_t hvx::restricted_direct_launch_wide4(const void *args, bool ext, bool unrolled, hipStream_t s) { return launch_wide<4>(args, ext, unrolled, s); }
