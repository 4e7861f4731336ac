// hvx_hnsw_wave_occ2_l2_ad.hip -- the NON-strict layer-0 arms (SimHash filter, pre / post sampling, adaptive bypass: what
// SearchParams::new(k) selects, crates/db/src/execution/interpreter/access/search/storage.rs:140-141) budgeted for TWO queries per
// SIMD: f32 rows, squared-Euclidean.  For hosts that keep several batches in flight (execution lanes, the batcher): the row
// gathers of one query run underneath the policy / RNG / beam bookkeeping of the other.
#include "hvx_hnsw_wave.h"

namespace hvx {
hipError_t launch_hnsw_wave_occ2_l2_ad(const HnswArgs &a, uint32_t b, const WavePlan &p, hipStream_t s) {
    return p.st ? launch_wave_r<kL2, 3, 6, false, true, true, 2>(a, b, p, s) : launch_wave_r<kL2, 3, 6, false, true, false, 2>(a, b, p, s);
}
} // namespace hvx
