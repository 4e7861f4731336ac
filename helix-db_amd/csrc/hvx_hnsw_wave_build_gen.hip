// hvx_hnsw_wave_build_gen.hip -- BUILD instantiations of the GENERIC one-wavefront-per-query kernel (NK = 0: any dimension incl. the
// scalar tail, any metric -- Manhattan's sequential order too --, the AVX / AVX+FMA / scalar summation trees): the search side of
// a batched insert_hnsw (mutation.rs:787-895, 904-1005) for the shapes the unrolled builds of hvx_hnsw_wave_build.hip do not
// serve, and for ef_construction up to 800.  f32 rows; consumed by hvx_build.hip.
#include "hvx_hnsw_wave.h"

namespace hvx {
hipError_t launch_hnsw_wave_build_gen(const HnswArgs &a, uint32_t b, const WavePlan &p, hipStream_t s) {
    switch (p.metric) {
    case kCosine: return launch_wave_generic<kCosine, false, true, true>(a, b, p, s);
    case kL2: return launch_wave_generic<kL2, false, true, true>(a, b, p, s);
    default: return launch_wave_generic<kL1, false, true, true>(a, b, p, s);
    }
}
} // namespace hvx
