// hvx_hnsw_wave_l2.hip -- squared-Euclidean, f32 rows: instantiations of the one-wavefront-per-query HNSW kernel.
#include "hvx_hnsw_wave.h"

namespace hvx {
hipError_t launch_hnsw_wave_l2(const HnswArgs &a, uint32_t b, const WavePlan &p, hipStream_t s) {
    return launch_wave_r<kL2, 3, 6, false>(a, b, p, s);
}
} // namespace hvx
