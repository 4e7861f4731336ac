// shortest_path_host_probe.cpp -- runs the host shortest path (helix-db_amd/csrc/hvx_shortest_path_host.h, the only project header it
// includes) over a graph and requests read from a text file: "n m labelled", m lines "src dst label" with the sources ascending and every
// row ascending by target, then "k" and k lines "source target max_depth direction n_labels [labels]".  Prints one line per request:
// the path's length, then its nodes.  tests/test_shortest_path_host.py compiles it with -fsanitize=address,undefined and holds the output
// to the Python twin.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../helix-db_amd/csrc/hvx_shortest_path_host.h"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned long long n = 0, m = 0, k = 0;
    int labelled = 0;
    if (fscanf(f, "%llu %llu %d", &n, &m, &labelled) != 3) return 2;
    std::vector<uint64_t> off(n + 1, 0), tgt(m);
    std::vector<uint32_t> lab(m);
    for (size_t i = 0; i < m; ++i) {
        unsigned long long s, d;
        unsigned l;
        if (fscanf(f, "%llu %llu %u", &s, &d, &l) != 3 || s >= n) return 2;
        ++off[s + 1];
        tgt[i] = d;
        lab[i] = l;
    }
    for (size_t u = 0; u < n; ++u) off[u + 1] += off[u];
    hvx_sp::HostGraph g;
    if (hvx_sp::build_incoming(n, m, off.data(), tgt.data(), labelled ? lab.data() : nullptr, &g)) {
        printf("bad graph\n");
        return 0;
    }
    if (fscanf(f, "%llu", &k) != 1) return 2;
    for (size_t i = 0; i < k; ++i) {
        unsigned long long s, t;
        unsigned max_depth, direction, n_labels;
        if (fscanf(f, "%llu %llu %u %u %u", &s, &t, &max_depth, &direction, &n_labels) != 5 || s >= n || t >= n) return 2;
        std::vector<uint32_t> allowed(n_labels);
        for (unsigned j = 0; j < n_labels; ++j)
            if (fscanf(f, "%u", &allowed[j]) != 1) return 2;
        const std::vector<uint64_t> path = hvx_sp::shortest_path(g, s, t, max_depth, direction, allowed.data(), n_labels);
        printf("%zu", path.size());
        for (uint64_t v : path) printf(" %llu", (unsigned long long)v);
        printf("\n");
    }
    fclose(f);
    return 0;
}
