// Stand-alone host program of tests/test_host_visit_records.py: packs the per-block records of csrc/scn_blk_record.h from the separate
// plan arrays of every case in the file named on the command line and checks each field of each record against those arrays.  Built
// with -fsanitize=address,undefined and run directly; never loaded into Python.
//
// File: int32 n_cases, then per case  int32 n_blocks, int32 corrupt | blk_row0[n] i32 | src_ptr[n + 1] i32 | ell_ptr[n] i32 |
// blk_rows[n] u8 | width[n] u8 | tile_w[8 n] u8 | tile_wu[8 n] u8.  corrupt = 1: the case must be REFUSED (a source count past a byte).
// Prints "ok <cases> <blocks>" and returns 0, or says what differs and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "scn_blk_record.h"

template <typename T>
static bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n_cases = 0;
    if (fread(&n_cases, 4, 1, f) != 1) return 2;
    long blocks = 0;
    for (int c = 0; c < n_cases; ++c) {
        int32_t head[2];
        if (fread(head, 4, 2, f) != 2) return 2;
        const int n = head[0];
        std::vector<int32_t> row0, src_ptr, ell_ptr;
        std::vector<uint8_t> rows, width, tw, twu;
        if (!read_vec(f, row0, n) || !read_vec(f, src_ptr, (size_t)n + 1) || !read_vec(f, ell_ptr, n) || !read_vec(f, rows, n) ||
            !read_vec(f, width, n) || !read_vec(f, tw, (size_t)8 * n) || !read_vec(f, twu, (size_t)8 * n))
            return 2;
        std::vector<scn::BlockRec> rec(n);                       // exactly n records: a write past the last one is the sanitizer's to find
        if (n) memset(rec.data(), 0xA5, rec.size() * sizeof(scn::BlockRec));
        const bool ok = scn::pack_block_records(n, row0.data(), rows.data(), src_ptr.data(), ell_ptr.data(), width.data(), tw.data(), twu.data(),
                                                rec.data());
        if (ok == (head[1] != 0)) {
            printf("case %d: pack returned %d, corrupt = %d\n", c, (int)ok, head[1]);
            return 1;
        }
        if (!ok) continue;
        for (int b = 0; b < n; ++b) {
            const scn::BlockRec& r = rec[b];
            // the record as the kernels read it: eight 32-bit words
            uint32_t w[8];
            memcpy(w, &r, 32);
            bool same = (int32_t)w[0] == row0[b] && (int32_t)w[1] == ell_ptr[b] && (int32_t)w[2] == src_ptr[b] &&
                        (int)(w[3] & 255u) == src_ptr[b + 1] - src_ptr[b] && (w[3] >> 8 & 255u) == rows[b] && (w[3] >> 16 & 255u) == width[b] &&
                        (w[3] >> 24) == 0;
            for (int i = 0; i < 8; ++i)
                same = same && (w[4 + i / 4] >> (8 * (i % 4)) & 255u) == tw[(size_t)8 * b + i] && (w[6 + i / 4] >> (8 * (i % 4)) & 255u) == twu[(size_t)8 * b + i];
            if (!same || ((uintptr_t)&r & 31) != 0) {
                printf("case %d, block %d: the record differs from the arrays\n", c, b);
                return 1;
            }
        }
        blocks += n;
    }
    fclose(f);
    printf("ok %d %ld\n", (int)n_cases, blocks);
    return 0;
}
