// hvx_hnsw_wave_gen_cos.hip -- GENERIC (any dimension / summation tree) builds of the one-wavefront-per-query kernel with the
// non-strict layer-0 arms, metric kCosine: what serves `SearchParams::new(k)` on the shapes the unrolled builds do not.
#include "hvx_hnsw_wave.h"

namespace hvx {
hipError_t launch_hnsw_wave_gen_cos(const HnswArgs &a, uint32_t b, const WavePlan &p, hipStream_t s) {
    return p.st ? launch_wave_generic<kCosine, true, true, false>(a, b, p, s) : launch_wave_generic<kCosine, true, false, false>(a, b, p, s);
}
} // namespace hvx
