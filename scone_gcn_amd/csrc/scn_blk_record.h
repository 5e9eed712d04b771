// The packed per-block record of the block plan (no HIP dependency: a host program can include this file on its own).
// build_block_plan keeps a block's header in separate arrays (blk_row0, blk_rows, src_ptr, width, ell_ptr, tile_w, tile_wu), which a
// kernel's unit prologue reads with one load each.  The visiting backwards (scn_blk_bwd.inc) take a unit's header from ONE 32-byte,
// 32-byte aligned record instead -- through an LDS table their window scan fills (scn_window_scan.inc), or as one 32-byte load:
//   word 0  row0      first output row                         word 3  nsrc | rows << 8 | width << 16   (a byte each; nsrc <= 128,
//   word 1  ell_ptr   first ELL entry                                  rows <= 64, width <= 254)
//   word 2  src_ptr   first entry of src_rows                  words 4-5 / 6-7  tile_w[8] / tile_wu[8] of the 8-wave kernels
// The separate arrays stay: every other kernel reads them, and the records are packed FROM them.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace scn {

constexpr int BLK_REC_WAVES = 8;                                  // = BK_WAVES (scn_internal.h; asserted where both are seen)
struct alignas(32) BlockRec {
    int32_t row0, ell_ptr, src_ptr;
    uint8_t nsrc, rows, width, pad;
    uint8_t tile_w[BLK_REC_WAVES], tile_wu[BLK_REC_WAVES];
};
static_assert(sizeof(BlockRec) == 32 && alignof(BlockRec) == 32, "one 32-byte record per block");

// records of n_blocks blocks from the plan's arrays (src_ptr has n_blocks + 1 entries, tile_w / tile_wu eight per block).  Returns
// false where a field does not fit its byte (no plan has such a block: BK_SRC = 128, BK_R = 64, widths <= 254).
inline bool pack_block_records(int n_blocks, const int32_t* blk_row0, const uint8_t* blk_rows, const int32_t* src_ptr, const int32_t* ell_ptr,
                               const uint8_t* width, const uint8_t* tile_w, const uint8_t* tile_wu, BlockRec* out) {
    for (int b = 0; b < n_blocks; ++b) {
        const int32_t nsrc = src_ptr[b + 1] - src_ptr[b];
        if (nsrc < 0 || nsrc > 255) return false;
        BlockRec& r = out[b];
        r.row0 = blk_row0[b];
        r.ell_ptr = ell_ptr[b];
        r.src_ptr = src_ptr[b];
        r.nsrc = (uint8_t)nsrc;
        r.rows = blk_rows[b];
        r.width = width[b];
        r.pad = 0;
        for (int i = 0; i < BLK_REC_WAVES; ++i) {
            r.tile_w[i] = tile_w[(size_t)b * BLK_REC_WAVES + i];
            r.tile_wu[i] = tile_wu[(size_t)b * BLK_REC_WAVES + i];
        }
    }
    return true;
}

}  // namespace scn
