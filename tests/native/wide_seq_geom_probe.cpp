// wide_seq_geom_probe.cpp -- prints what wide_seq_geom() (helix-db_amd/csrc/hvx_build_dev.h) decides for the one-node steps of images with
// degree limits above 32: the matrix regions inside the scratch insert_range sizes from it, the grids, the link step's LDS bytes, and
// the pair prefix of a list of link degrees.  tests/test_build_wide_seq_host.py checks the output.  Host only: no device is touched.
//   wide_seq_geom_probe                       G / R lines for (m, m0) in {(32, 64), (24, 48), (17, 33), (16, 32), (40, 80)} x 1..6 layers
//   wide_seq_geom_probe prefix MAXN D0 D1 ..  the pair prefix of links whose lists hold D0, D1, .. ids: ns + 1 numbers
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../helix-db_amd/csrc/hvx_build_dev.h"

using namespace hvx;

int main(int argc, char **argv) {
    if (argc >= 3 && !strcmp(argv[1], "prefix")) {
        const uint32_t maxn = (uint32_t)atoi(argv[2]);
        uint32_t base = 0;
        for (int i = 3; i < argc; ++i) {
            printf("%u ", base);
            base += wide_seq_list_pairs((uint32_t)atoi(argv[i]), maxn);
        }
        printf("%u\n", base);
        return 0;
    }
    const uint32_t limits[][2] = {{32, 64}, {24, 48}, {17, 33}, {16, 32}, {40, 80}};
    for (const auto &mm : limits)
        for (uint32_t layers = 1; layers <= 6; ++layers) {
            const WideSeqGeom g = wide_seq_geom(mm[0], mm[1], layers);
            printf("G m=%u m0=%u layers=%u ok=%d total=%zu link_lds=%u sel_g0=%u sel_gu=%u link_g0=%u link_gu=%u link_rs=%u list=%u log=%u\n", mm[0], mm[1], layers, (int)g.ok,
                   g.total_floats(), g.link_lds, g.sel_g0, g.sel_gu, g.link_g0, g.link_gu, kWideSeqRS, kWideSeqRow, kWideSeqPairs);
            if (!g.ok) continue;
            for (uint32_t L = 0; L < layers; ++L) {
                const int u = L ? 1 : 0;
                printf("R m=%u m0=%u layers=%u layer=%u kind=select off=%zu floats=%u rw=%u rows=%u\n", mm[0], mm[1], layers, L, g.sel_off(L), g.sel_dm[u], g.sel_rw[u],
                       g.sel_dm[u] / g.sel_rw[u]);
                for (uint32_t t = 0; t < g.maxn[u]; ++t)
                    printf("R m=%u m0=%u layers=%u layer=%u kind=link%u off=%zu floats=%u rw=%u rows=%u\n", mm[0], mm[1], layers, L, t, g.link_off(L, t), g.link_dm, kWideSeqRS,
                           g.link_dm / kWideSeqRS);
            }
        }
    return 0;
}
