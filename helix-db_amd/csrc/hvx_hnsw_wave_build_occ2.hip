// hvx_hnsw_wave_build_occ2.hip -- BUILD instantiations of the one-wavefront-per-query kernel budgeted for TWO wavefronts per SIMD
// (256 registers, 20 KiB of LDS each): the search side of a batched insert_hnsw (mutation.rs:787-895, 904-1005) for batches of
// more than 1 024 nodes, where the one-per-SIMD build would run the batch in two rounds.  Same algorithm, same results (a visited
// table that fills spills to the exact bitmap); consumed by hvx_build.hip.
#include "hvx_hnsw_wave.h"

namespace hvx {
hipError_t launch_hnsw_wave_build_occ2(const HnswArgs &a, uint32_t b, const WavePlan &p, hipStream_t s) {
    return p.metric == kL2 ? launch_wave_r<kL2, 3, 6, false, false, true, 2, true>(a, b, p, s) : launch_wave_r<kCosine, 3, 6, false, false, true, 2, true>(a, b, p, s);
}
} // namespace hvx
