// Block ranges of the step epilogue (scn_step_epilogue; no HIP dependency: a host program can include this file on its own).
// One launch runs every job a micro-batch deferred; each job keeps the workgroups its stand-alone launch had, and a workgroup finds
// its job by its index: job j owns the blocks [end[j - 1], end[j]) (end[-1] = 0).  An absent job owns none.
//   job 0                  the loss sum                       (masked_ce_kernel: 1 block)
//   job 1                  the readout's weight gradient      (readout_dw_kernel: 1 block)
//   jobs 2 .. 5            blocked_dw_reduce of one backward  (ceil(c_aux * 3 * cd / 64) blocks each)
//   job 6                  the first layer's dW reduce        (96 blocks: 32 channels; 48: the slab-pair form)
//   job 7                  the clear of the readout gradient  (one block per trajectory)
//   jobs 8 .. 11           clear_mask_kernel of one tensor    (min(plan blocks, 2048) each)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SCN_RANGES_FN __host__ __device__ inline
#else
#define SCN_RANGES_FN inline
#endif

namespace scn {

constexpr int EPI_MAX_REDUCES = 4, EPI_MAX_CLEARS = 4;
constexpr int EPI_JOB_LOSS = 0, EPI_JOB_READOUT_DW = 1, EPI_JOB_REDUCE = 2, EPI_JOB_FIRST = EPI_JOB_REDUCE + EPI_MAX_REDUCES,
              EPI_JOB_READOUT_CLEAR = EPI_JOB_FIRST + 1, EPI_JOB_CLEAR = EPI_JOB_READOUT_CLEAR + 1, EPI_JOBS = EPI_JOB_CLEAR + EPI_MAX_CLEARS;
constexpr int EPI_FIRST_NONE = 0, EPI_FIRST_C32 = 1, EPI_FIRST_PAIR = 2;
constexpr int64_t EPI_MAX_BLOCKS = 1 << 30;

struct EpiRanges {
    int32_t end[EPI_JOBS];
};

// the stand-alone launches' grids
SCN_RANGES_FN int64_t epi_reduce_blocks(int64_t c_aux, int64_t cd) { return (c_aux * 3 * cd + 63) / 64; }
SCN_RANGES_FN int64_t epi_first_blocks(int form) { return form == EPI_FIRST_C32 ? 96 : (form == EPI_FIRST_PAIR ? 48 : 0); }
SCN_RANGES_FN int64_t epi_clear_blocks(int64_t plan_blocks) { return plan_blocks < 2048 ? plan_blocks : 2048; }

// ranges from the jobs' block counts; false where a count is negative or the grid would pass EPI_MAX_BLOCKS
SCN_RANGES_FN bool epi_ranges(const int64_t* counts, EpiRanges* r) {
    int64_t at = 0;
    for (int j = 0; j < EPI_JOBS; ++j) {
        if (counts[j] < 0 || counts[j] > EPI_MAX_BLOCKS) return false;
        at += counts[j];
        if (at > EPI_MAX_BLOCKS) return false;
        r->end[j] = (int32_t)at;
    }
    return true;
}

SCN_RANGES_FN int32_t epi_total(const EpiRanges& r) { return r.end[EPI_JOBS - 1]; }

// the job of a block and the block's index inside it; -1 for a block outside the grid
SCN_RANGES_FN int epi_job_of(const EpiRanges& r, int32_t block, int32_t* rel) {
    if (block < 0) return -1;
    int32_t begin = 0;
    for (int j = 0; j < EPI_JOBS; ++j) {
        if (block < r.end[j]) {
            *rel = block - begin;
            return j;
        }
        begin = r.end[j];
    }
    return -1;
}

}  // namespace scn
