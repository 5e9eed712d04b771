// Stand-alone host check of the step epilogue's block ranges (csrc/scn_step_ranges.h), built with -fsanitize=address,undefined by
// tests/test_host_step_ranges.py and run directly.  Input file: int32 n_cases, then per case EPI_JOBS int64 block counts and one int64
// `valid`; then int32 n_helpers and per helper four int64 (c_aux, c_dz, first form, plan blocks).
// Per case the ranges are checked against brute force: an owner array filled job by job from the counts -- every block of the grid
// has exactly one job, epi_job_of names it with the right index inside the job, every job has as many blocks as its count, and the
// blocks just outside the grid have none.  Prints "ok <cases> <blocks checked>" and one line per helper with the three grids.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "scn_step_ranges.h"

using namespace scn;

static bool read_all(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n_cases = 0;
    if (!read_all(f, &n_cases, 4)) return 2;
    long long checked = 0;
    for (int32_t k = 0; k < n_cases; ++k) {
        int64_t counts[EPI_JOBS], valid = 0;
        if (!read_all(f, counts, sizeof(counts)) || !read_all(f, &valid, 8)) return 2;
        EpiRanges r;
        const bool ok = epi_ranges(counts, &r);
        if (ok != (valid != 0)) { printf("case %d: epi_ranges returned %d\n", k, (int)ok); return 1; }
        if (!ok) continue;
        std::vector<int> owner;
        std::vector<int32_t> index;
        for (int j = 0; j < EPI_JOBS; ++j)
            for (int64_t i = 0; i < counts[j]; ++i) { owner.push_back(j); index.push_back((int32_t)i); }
        if ((int64_t)owner.size() != epi_total(r)) { printf("case %d: total %d, want %zu\n", k, epi_total(r), owner.size()); return 1; }
        std::vector<int64_t> seen(EPI_JOBS, 0);
        for (int32_t b = 0; b < epi_total(r); ++b) {
            int32_t rel = -7;
            const int j = epi_job_of(r, b, &rel);
            if (j != owner[b] || rel != index[b]) { printf("case %d block %d: job %d rel %d, want %d %d\n", k, b, j, rel, owner[b], index[b]); return 1; }
            ++seen[j];
            ++checked;
        }
        for (int j = 0; j < EPI_JOBS; ++j)
            if (seen[j] != counts[j]) { printf("case %d job %d: %lld blocks, want %lld\n", k, j, (long long)seen[j], (long long)counts[j]); return 1; }
        int32_t rel = 0;
        if (epi_job_of(r, -1, &rel) != -1 || epi_job_of(r, epi_total(r), &rel) != -1 || epi_job_of(r, INT32_MAX, &rel) != -1) {
            printf("case %d: a block outside the grid has a job\n", k);
            return 1;
        }
    }
    printf("ok %d %lld\n", n_cases, checked);
    int32_t n_helpers = 0;
    if (!read_all(f, &n_helpers, 4)) return 2;
    for (int32_t k = 0; k < n_helpers; ++k) {
        int64_t h[4];
        if (!read_all(f, h, sizeof(h))) return 2;
        printf("%lld %lld %lld\n", (long long)epi_reduce_blocks(h[0], h[1]), (long long)epi_first_blocks((int)h[2]), (long long)epi_clear_blocks(h[3]));
    }
    fclose(f);
    return 0;
}
