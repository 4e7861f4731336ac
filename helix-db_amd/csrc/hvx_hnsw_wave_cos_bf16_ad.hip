// hvx_hnsw_wave_cos_bf16_ad.hip -- cosine, bf16 rows, NON-strict layer-0 arms: AD instantiations of the
// one-wavefront-per-query HNSW kernel.
#include "hvx_hnsw_wave.h"

namespace hvx {
hipError_t launch_hnsw_wave_cos_bf16_ad(const HnswArgs &a, uint32_t b, const WavePlan &p, hipStream_t s) {
    return p.st ? launch_wave_r<kCosine, 3, 6, true, true, true>(a, b, p, s) : launch_wave_r<kCosine, 3, 6, true, true, false>(a, b, p, s);
}
} // namespace hvx
