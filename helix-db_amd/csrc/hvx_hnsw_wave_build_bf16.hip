// hvx_hnsw_wave_build_bf16.hip -- BUILD instantiations of the one-wavefront-per-query kernel over bf16 rows (round 6): the search side of
// a one-node insert / upsert into a bf16 image (config #4's storage).  The node's rounded vector is the f32 query (HnswArgs::queries), the
// rows it is compared with are the image's bf16 rows: f32 arithmetic on the rounded values in the reference's order, as every bf16 search.
#include "hvx_hnsw_wave.h"

namespace hvx {
hipError_t launch_hnsw_wave_build_bf16(const HnswArgs &a, uint32_t b, const WavePlan &p, hipStream_t s) {
    return p.metric == kL2 ? launch_wave_r<kL2, 3, 6, true, false, true, 1, true>(a, b, p, s) : launch_wave_r<kCosine, 3, 6, true, false, true, 1, true>(a, b, p, s);
}
} // namespace hvx
