// hvx_hnsw_wave_prof.hip -- phase-timing build of the wave kernel (L2, R=3, dim 768 only); launched
// instead of the production kernel when HVX_WAVE_PROF is set, for kernel tuning.
#include "hvx_hnsw_wave.h"

namespace hvx {
hipError_t launch_hnsw_wave_prof(const HnswArgs &a, uint32_t b, const WavePlan &p, hipStream_t s) {
#ifdef HVX_TUNING // the non-strict arms, phase-timed (slot 6 = decision epoch + candidate selection)
    if (p.ad) return p.metric == kL2 ? launch_wave_kernel<kL2, 3, 24, false, true, true, false>(a, b, p, s)
                                     : launch_wave_kernel<kCosine, 3, 24, false, true, true, false>(a, b, p, s);
#endif
    return launch_wave_kernel<kL2, 3, 24, false, true>(a, b, p, s);
}
} // namespace hvx
