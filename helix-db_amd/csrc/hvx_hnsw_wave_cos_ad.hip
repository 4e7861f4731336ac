// hvx_hnsw_wave_cos_ad.hip -- cosine, f32 rows, NON-strict layer-0 arms (SimHash threshold filter, sampling, adaptive
// bypass): AD instantiations of the one-wavefront-per-query HNSW kernel.
#include "hvx_hnsw_wave.h"

namespace hvx {
hipError_t launch_hnsw_wave_cos_ad(const HnswArgs &a, uint32_t b, const WavePlan &p, hipStream_t s) {
    return p.st ? launch_wave_r<kCosine, 3, 6, false, true, true>(a, b, p, s) : launch_wave_r<kCosine, 3, 6, false, true, false>(a, b, p, s);
}
} // namespace hvx
