// hvx_hnsw_wave_occ2_bf16.hip -- two-queries-per-SIMD build of the wave kernel over bf16 rows (strict-exhaustive arm).
#include "hvx_hnsw_wave.h"

namespace hvx {
hipError_t launch_hnsw_wave_occ2_bf16(const HnswArgs &a, uint32_t b, const WavePlan &p, hipStream_t s) {
    return p.metric == kL2 ? launch_wave_r<kL2, 3, 6, true, false, true, 2>(a, b, p, s) : launch_wave_r<kCosine, 3, 6, true, false, true, 2>(a, b, p, s);
}
} // namespace hvx
