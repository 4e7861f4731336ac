// audit_poke.hip -- test-only window onto the graph rows of a device image (tests/audit_harness.py, tests/test_gpu_audit.py).
// hvx_index_import rejects rows that are unsorted, duplicated, self-referencing or that name unknown ids, so the defects the audit
// (csrc/hvx_audit.hip) counts cannot be planted through the ABI.  This helper reads the image as the device holds it and overwrites
// single slots of it.  It is built with the library's own flags (struct hvx_index has the library's layout), holds no kernel -- only
// hipMemcpy on the pointers of ix->dev -- and is neither linked into the product library nor declared in include/helix_vec.h.
#include <hip/hip_runtime.h>

#include <mutex>

#include "hvx_host.h"

namespace {
enum { kN, kS0, kSu, kUpRows, kCapRows, kCapUpRows, kEntry, kHasEntry, kMaxLayer, kM, kM0, kHasDead, kHeaderWords };
}

// hdr [12]: n, s0, su, upper rows in use, row capacity, upper-row capacity, entry, has_entry, max_layer, m, m0, has_dead.  Every array
// pointer may be NULL (a first call reads the sizes): l0 [n][s0], up [upper rows in use][su], level [n], up_base [n],
// dead [(n + 31) / 32] (filled when has_dead).  Returns 0, or the hipError_t of the call that failed.
extern "C" int audit_poke_dump(hvx_index *ix, uint32_t *hdr, uint32_t *l0, uint32_t *up, uint16_t *level, uint32_t *up_base, uint32_t *dead) {
    if (!ix || !hdr) return -1;
    std::lock_guard<std::mutex> lock(ix->mu);
    hipError_t e = hipSetDevice(ix->device);
    if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
    if (e != hipSuccess) return (int)e;
    const hvx::DevIndex &d = ix->dev;
    hdr[kN] = d.n, hdr[kS0] = d.s0, hdr[kSu] = d.su, hdr[kUpRows] = (uint32_t)ix->up_rows_used;
    hdr[kCapRows] = (uint32_t)ix->cap_rows, hdr[kCapUpRows] = (uint32_t)ix->cap_up_rows;
    hdr[kEntry] = d.entry, hdr[kHasEntry] = d.has_entry, hdr[kMaxLayer] = d.max_layer;
    hdr[kM] = ix->desc.m, hdr[kM0] = ix->desc.m0, hdr[kHasDead] = d.dead ? 1u : 0u;
    auto pull = [&](void *dst, const void *src, size_t bytes) {
        if (e == hipSuccess && dst && bytes) e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    };
    pull(l0, d.l0, (size_t)d.n * d.s0 * 4);
    pull(up, d.up, (size_t)ix->up_rows_used * d.su * 4);
    pull(level, d.level, (size_t)d.n * 2);
    pull(up_base, d.up_base, (size_t)d.n * 4);
    if (d.dead) pull(dead, d.dead, (size_t)((d.n + 31u) / 32u) * 4);
    return (int)e;
}

// One u32 into slot `slot` of layer-0 row `row` (upper == 0) or of upper row `row` (upper != 0); rows up to the image's capacity, so
// that the spare rows past n can be written too.  Returns 0, -2 for a slot outside the arrays, or the hipError_t of the copy.
extern "C" int audit_poke_write(hvx_index *ix, uint32_t upper, uint64_t row, uint32_t slot, uint32_t value) {
    if (!ix) return -1;
    std::lock_guard<std::mutex> lock(ix->mu);
    const hvx::DevIndex &d = ix->dev;
    const uint64_t rows = upper ? ix->cap_up_rows : ix->cap_rows;
    const uint32_t stride = upper ? d.su : d.s0;
    if (row >= rows || slot >= stride) return -2;
    hipError_t e = hipSetDevice(ix->device);
    if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
    uint32_t *dst = const_cast<uint32_t *>(upper ? d.up : d.l0) + (size_t)row * stride + slot;
    if (e == hipSuccess) e = hipMemcpy(dst, &value, 4, hipMemcpyHostToDevice);
    return (int)e;
}
