// hvx_hnsw_wave_occ2_cos_bf16_ad.hip -- the non-strict layer-0 arms over bf16 rows (config #4 storage), budgeted for TWO queries per
// SIMD, cosine: SearchParams::new(k) on execution lanes / the batcher for reduced-precision images.
#include "hvx_hnsw_wave.h"

namespace hvx {
hipError_t launch_hnsw_wave_occ2_cos_bf16_ad(const HnswArgs &a, uint32_t b, const WavePlan &p, hipStream_t s) {
    return p.st ? launch_wave_r<kCosine, 3, 6, true, true, true, 2>(a, b, p, s) : launch_wave_r<kCosine, 3, 6, true, true, false, 2>(a, b, p, s);
}
} // namespace hvx
