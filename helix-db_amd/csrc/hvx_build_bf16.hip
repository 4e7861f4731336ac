// hvx_build_bf16.hip -- build_link_wg_kernel over bf16 rows: the link step of the batched build / insert of a bf16 image (hvx_build.hip
// picks it per image; the kernel and what BF changes in it: hvx_build_link_wg.h).
#include "hvx_build_link_wg.h"

namespace hvx {
BuildKernel build_link_wg_bf16_kernel(uint32_t metric) {
    return metric == kL2 ? build_link_wg_kernel<kL2, true, true> : build_link_wg_kernel<kCosine, true, true>;
}
} // namespace hvx
