// hvx_hnsw_wave_build.hip -- BUILD instantiations of the one-wavefront-per-query kernel: the search side of a batched
// insert_hnsw (greedy descent above the node's level, search_layer_beam on every layer from there down; mutation.rs:787-895,
// 904-1005).  f32 rows, squared-Euclidean and cosine; consumed by hvx_build.hip.
#include "hvx_hnsw_wave.h"

namespace hvx {
hipError_t launch_hnsw_wave_build(const HnswArgs &a, uint32_t b, const WavePlan &p, hipStream_t s) {
    return p.metric == kL2 ? launch_wave_r<kL2, 3, 6, false, false, true, 1, true>(a, b, p, s) : launch_wave_r<kCosine, 3, 6, false, false, true, 1, true>(a, b, p, s);
}
} // namespace hvx
