// Host-only probe of the bf16 column-block staging of build_link_wg_kernel (helix-db_amd/csrc/hvx_device.h: bf16_block_piece,
// bf16_piece_widen): rows of distinct bf16 values are packed into the interleaved device layout with bf16_slot_of, every column block
// is staged the way the kernel's commit step does it, and the staged floats must be the plain-order row, element for element.
// usage: probe dim ck
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../helix-db_amd/csrc/hvx_device.h"

using namespace hvx;

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const uint32_t dim = (uint32_t)atoi(argv[1]), ck = (uint32_t)atoi(argv[2]);
    if (dim % 64u != 0u || ck % 2u != 0u || ck == 0u) return 2;
    const uint32_t nrows = 5, nk = dim >> 5, nblocks = (nk + ck - 1u) / ck, ldp = ck * 32u + 32u;
    // distinct bf16 bit patterns (positive normal numbers), different in every row
    std::vector<uint16_t> plain((size_t)nrows * dim), packed((size_t)nrows * dim);
    for (uint32_t r = 0; r < nrows; ++r)
        for (uint32_t i = 0; i < dim; ++i) {
            plain[(size_t)r * dim + i] = (uint16_t)(0x1000u + r * 0x0800u + i);
            packed[(size_t)r * dim + bf16_slot_of(i)] = plain[(size_t)r * dim + i];
        }
    unsigned long checked = 0;
    for (uint32_t blk = 0; blk < nblocks; ++blk) {
        const uint32_t ckb = nk - blk * ck < ck ? nk - blk * ck : ck, cw = ckb * 4u; // chunks / pieces per row of this block
        std::vector<uint32_t> lds((size_t)nrows * ldp, 0xDEADBEEFu);
        for (uint32_t e = 0; e < nrows * ck * 4u; ++e) {
            const Bf16BlockPiece pc = bf16_block_piece(e, blk, ck);
            if (pc.row >= nrows) { fprintf(stderr, "piece %u: row %u\n", e, pc.row); return 1; }
            if (pc.col >= cw) continue; // the partial last block
            if (pc.src >= dim / 8u || pc.dst + 36u > ckb * 32u) { fprintf(stderr, "piece %u of block %u out of range: src %u dst %u\n", e, blk, pc.src, pc.dst); return 1; }
            uint32_t w[4];
            memcpy(w, &packed[(size_t)pc.row * dim + (size_t)pc.src * 8u], 16);
            float lo[4], hi[4];
            bf16_piece_widen(w, lo, hi);
            for (int t = 0; t < 4; ++t) {
                uint32_t *d0 = &lds[(size_t)pc.row * ldp + pc.dst + (uint32_t)t], *d1 = d0 + 32;
                if (*d0 != 0xDEADBEEFu || *d1 != 0xDEADBEEFu) { fprintf(stderr, "block %u: float written twice (piece %u)\n", blk, e); return 1; }
                memcpy(d0, &lo[t], 4);
                memcpy(d1, &hi[t], 4);
            }
            // the eight pieces of an aligned group (one ds_write_b128 lane group) land on 32 different banks, twice: (a / 4) % 32
            if ((e & 7u) == 0u) {
                uint32_t seen = 0;
                for (uint32_t g = 0; g < 8u; ++g) {
                    const Bf16BlockPiece pg = bf16_block_piece(e + g, blk, ck);
                    if (pg.row != pc.row) { fprintf(stderr, "lane group of piece %u spans two rows\n", e); return 1; }
                    for (uint32_t t = 0; t < 4u; ++t) seen |= 1u << ((pg.row * ldp + pg.dst + t) % 32u);
                }
                if (seen != 0xFFFFFFFFu) { fprintf(stderr, "lane group of piece %u: bank conflict (banks %08x)\n", e, seen); return 1; }
            }
        }
        for (uint32_t r = 0; r < nrows; ++r)
            for (uint32_t i = 0; i < ldp; ++i) {
                const uint32_t got = lds[(size_t)r * ldp + i];
                if (i < ckb * 32u) {
                    const uint32_t want = (uint32_t)plain[(size_t)r * dim + blk * ck * 32u + i] << 16;
                    if (got != want) { fprintf(stderr, "dim %u ck %u block %u row %u float %u: %08x, want %08x\n", dim, ck, blk, r, i, got, want); return 1; }
                    ++checked;
                } else if (got != 0xDEADBEEFu) { fprintf(stderr, "block %u row %u: float %u beyond the block was written\n", blk, r, i); return 1; }
            }
    }
    // a whole row, piece by piece (stage_row<BF> and the build's query rows use bf16_piece_dst over all dim / 8 pieces)
    for (uint32_t t = 0; t < dim / 8u; ++t) {
        uint32_t w[4];
        memcpy(w, &packed[(size_t)t * 8u], 16);
        float lo[4], hi[4];
        bf16_piece_widen(w, lo, hi);
        const uint32_t d = bf16_piece_dst(t);
        for (uint32_t u = 0; u < 4u; ++u) {
            uint32_t g0, g1;
            memcpy(&g0, &lo[u], 4);
            memcpy(&g1, &hi[u], 4);
            if (d + 32u + u >= dim || g0 != (uint32_t)plain[d + u] << 16 || g1 != (uint32_t)plain[d + 32u + u] << 16) {
                fprintf(stderr, "whole row: piece %u lands at %u wrongly\n", t, d);
                return 1;
            }
        }
    }
    if (checked != (unsigned long)nrows * dim) { fprintf(stderr, "%lu of %u elements staged\n", checked, nrows * dim); return 1; }
    printf("ok %lu\n", checked);
    return 0;
}
