// Bit arithmetic on a workgroup's keep window (keep_window, scn_blk_fwd.inc): 64 bits, bit j = slab k0 + j of the block is kept.
// Pure integer functions, host and device, nothing else of the library: the kept forward walks its visits with them in SGPRs
// and tests/test_host_keep_visits.py checks them on the CPU against brute force.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SCN_KEEP_HD __host__ __device__ __forceinline__
#else
#define SCN_KEEP_HD inline
#endif

namespace scn {

// the window cut to a range of n slabs, 1 <= n <= 64: the bits from n on are other workgroups' slabs (or no slab at all).
// (~0 >> (64 - n), not (1 << n) - 1: at n = 64 the latter shifts by the type's width)
SCN_KEEP_HD uint64_t keep_cut(uint64_t win, int n) { return win & (~0ull >> (64 - n)); }
// number of visits = set bits
SCN_KEEP_HD int keep_count(uint64_t win) { return __builtin_popcountll(win); }
// position of the lowest set bit: the slab (relative to k0) of the first visit still in `win`; win != 0
SCN_KEEP_HD int keep_first(uint64_t win) { return __builtin_ctzll(win); }
// `win` without its first visit
SCN_KEEP_HD uint64_t keep_next(uint64_t win) { return win & (win - 1); }

// A mask's unit list (scn_keep_mask_units, scn_mask_hop_units) names every non-empty word of the mask once: entry = block * words +
// word, words = the mask's words per block (>= 1).  The block and the word of an entry:
SCN_KEEP_HD int unit_block(uint32_t entry, int words) { return (int)(entry / (uint32_t)words); }
SCN_KEEP_HD int unit_word(uint32_t entry, int words) { return (int)(entry % (uint32_t)words); }
// a window whose bit j is slab first + j, restricted to the slabs of mask word `word` (slabs 32 * word .. 32 * word + 31): what ONE
// entry of the list stands for -- a block with bits in two words of a window is two entries, each item once.  first, word >= 0.
SCN_KEEP_HD uint64_t keep_word_cut(uint64_t win, int first, int word) {
    const int64_t lo = (int64_t)32 * word - first;            // the window's bit of the word's first slab (may lie outside it)
    if (lo >= 64 || lo <= -32) return 0ull;
    return win & (lo >= 0 ? 0xffffffffull << lo : 0xffffffffull >> -lo);
}

}  // namespace scn
