// sp_dense_plan_probe.cpp -- runs the round plan of hvx_shortest_path_batch_dense (helix-db_amd/csrc/hvx_shortest_path_dense_plan.h, the
// only project header it includes) over cases read from a text file: one line "n b scratch_bytes" each.  Prints one line per case:
// "refused", or groups, groups per round, rounds, words, the four byte offsets and the byte count, then for EVERY round its first group,
// groups, first request and requests summed up as four checksums (sum of each) and the last round's four values.
// tests/test_shortest_path_dense_host.py compiles it with -fsanitize=address,undefined and holds the output to Python's big integers.
#include <cstdio>

#include "../../helix-db_amd/csrc/hvx_shortest_path_dense_plan.h"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned long long n, b, scratch;
    while (fscanf(f, "%llu %llu %llu", &n, &b, &scratch) == 3) {
        hvx_spd::RoundPlan p;
        if (!hvx_spd::plan_rounds(n, (uint32_t)b, scratch, &p)) {
            printf("refused\n");
            continue;
        }
        printf("%llu %llu %llu %llu %llu %llu %llu %llu %llu", (unsigned long long)p.groups, (unsigned long long)p.groups_per_round,
               (unsigned long long)p.rounds, (unsigned long long)p.words, (unsigned long long)p.seen_off, (unsigned long long)p.cur_off,
               (unsigned long long)p.next_off, (unsigned long long)p.lvl_off, (unsigned long long)p.bytes);
        unsigned long long sum_g0 = 0, sum_ng = 0, sum_r0 = 0, sum_nr = 0;
        hvx_spd::Round last = {0, 0, 0, 0};
        for (uint64_t r = 0; r < p.rounds; ++r) {
            last = hvx_spd::round_of(p, (uint32_t)b, r);
            sum_g0 += last.group0; sum_ng += last.n_groups; sum_r0 += last.request0; sum_nr += last.n_requests;
        }
        printf(" %llu %llu %llu %llu %llu %llu %u %u\n", sum_g0, sum_ng, sum_r0, sum_nr, (unsigned long long)last.group0,
               (unsigned long long)last.n_groups, last.request0, last.n_requests);
    }
    fclose(f);
    return 0;
}
