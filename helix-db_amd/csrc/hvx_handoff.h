// hvx_handoff.h -- the "last workgroup" hand-off: many workgroups each deliver a share of a result to HBM, the last one to deliver reads
// all of it and finishes the job in the same launch.  Used by the eager one-node insert steps (hvx_build.hip, hvx_build_wide_seq.hip), the fused delete step
// (hvx_delete.hip), the exact tail (hvx_flat_tail.hip) and the one-launch restricted scan (hvx_restricted_direct.h).
//
// No device-scope fence: an agent-scope release / acquire pair is an L2 write-back and an L2 INVALIDATE on this part (one L2 per XCD), and
// hundreds of short workgroups doing that to the L2 their neighbours are streaming rows through cost more than the work they hand off
// (first build of the exact tail: 200 us at 100 000 x 32).  Instead
//   * what is handed off is written with device-scope (write-through) stores and read with device-scope loads: st_agent / ld_agent;
//   * every wavefront waits until its stores have been acknowledged (vmcnt = 0: on gfx942 / gfx950 stores count in vmcnt, there is no
//     separate store counter).  A workgroup-scope release fence does NOT wait for them -- all wavefronts of a workgroup sit behind one
//     vector cache: the compiler omits vmcnt(0) outside threadgroup-split mode;
//   * a barrier, then thread 0 takes the ticket with a relaxed device-scope fetch_add; a second barrier publishes the answer.
// This lies outside the HIP memory model and holds for the hardware named below only.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx942__) && !defined(__gfx950__)
#error "hvx_handoff.h: the last-workgroup hand-off relies on stores being counted by vmcnt and on device-scope stores being written through (gfx942 / gfx950 only)"
#endif

namespace hvx {

template <typename T> __device__ __forceinline__ T ld_agent(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T> __device__ __forceinline__ void st_agent(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// every global store of this wavefront has been performed
__device__ __forceinline__ void stores_done() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Called by every thread of every workgroup that shares ticket word tickets[which], after its st_agent stores: true in the last of
// `expected` workgroups to get here.  s_flag: one word of LDS.  reset: the last workgroup writes the ticket back to zero (tickets that
// must be zero between launches and have nobody else to clear them).
__device__ __forceinline__ bool last_workgroup(uint32_t *tickets, uint32_t which, uint32_t expected, uint32_t *s_flag, bool reset) {
    stores_done();
    __syncthreads();
    if (threadIdx.x == 0) *s_flag = __hip_atomic_fetch_add(tickets + which, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == expected ? 1u : 0u;
    __syncthreads();
    const bool last = *s_flag != 0u;
    if (reset && last && threadIdx.x == 0) st_agent(tickets + which, 0u);
    return last;
}

} // namespace hvx
