// hvx_csr_view.h -- the CSR as the graph kernels see it: both adjacencies, by value in a kernel's arguments.
#pragma once
#include <cstdint>

namespace hvx {

struct CsrView {
    const uint64_t *out_off, *in_off;
    const uint32_t *out_tgt, *in_tgt, *out_lab, *in_lab; // labels null when the graph is unlabeled
    uint32_t n;
};

} // namespace hvx
