// hvx_restricted_wide13.hip -- the one-launch restricted exact scan with a result list of 13 registers per lane: 257 <= k <= 800 =
// MAX_RESTRICTED_RESULT_COUNT (restricted.rs:55); hvx_restricted_direct.h has the kernel, hvx_restricted_exact.hip the story and the dispatch.
#include "hvx_restricted_direct.h"

hipError_t hvx::restricted_direct_launch_wide13(const void *args, bool ext, bool unrolled, hipStream_t s) { return launch_wide<13>(args, ext, unrolled, s); }
