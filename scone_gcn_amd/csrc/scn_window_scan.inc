// batched window scan of the masked blocked kernels -- part of scn_blocked.hip (one translation unit; included inside namespace scn)
// ------------------------------------------------------------------------------------------------
// A masked launch (fwd_c32_w16_kernel<KEEP>, bwd_c32_bf16_kernel<VISIT>, gather3_c1_keep_kernel) visits a fraction of a per cent of its
// (block, slab) items, yet every workgroup used to walk ALL of its units one at a time: load the unit's block (P.assign), wait, load
// the block's mask words, wait, leave the empty block on a scalar branch -- two dependent memory round trips per unit, ~130 per
// workgroup and launch at the benchmark's size, which was most of what such a launch cost (profiles/window_scan_ab.txt).
// The blocks and windows of a workgroup's units do not depend on anything the visits compute, so they are fetched for WSCAN_CAP
// units at once, ahead of the block loop, in TWO round trips:
//   * wave 0 of the workgroup scans; lane l of chunk j handles unit first + (64 j + l) * stride.  All WSCAN_CHUNKS block loads are
//     issued together, then all 3 * WSCAN_CHUNKS mask-word loads (keep_window_lane: three loads, no branch), then the windows are
//     cut to the workgroup's slab range (keep_cut);
//   * the units whose window is non-zero are compacted IN ORDER (ballot + mbcnt per chunk, a running base across chunks) into an LDS
//     table [count][block x CAP][window lo x CAP][window hi x CAP] behind the kernel's own LDS (WSCAN_LDS_BYTES more per launch);
//   * a barrier publishes the table; every wave then walks it with uniform LDS reads made scalar (readfirstlane), which also claims
//     them: nothing of the scan is in flight when a slab loop starts (see keep_window, scn_blk_fwd.inc).
// A workgroup with more than WSCAN_CAP units (small grids on large plans) repeats this per WSCAN_CAP units: one barrier before a scan
// (every wave has left the previous table) and one after it.  The sequence a workgroup sees -- the same blocks in the same ascending
// unit order with the same windows as the one-at-a-time walk, minus the empty ones -- is what scn_window_scan_probe writes out.
// LIST MODE (the forward-side launches with a UnitList; include/scone_hip.h, "Unit lists").  A launch ends with its busiest
// workgroup, and a cone's items lie in a few neighbouring blocks per trajectory, so the static shares are uneven: on the benchmark's
// masks the busiest workgroup has 3 .. 6 x the mean visits (tools/cone_balance.py, profiles/cone_unit_list_ab.txt).  The forward-side
// kernels write items that do not depend on the workgroup computing them, so there the scan's SOURCE changes and nothing else: a
// unit is an entry of the mask's device-wide list of non-empty words (written by the mask kernels), workgroup g of G takes entries
// g, g + G, ..., the block comes from the entry and the window is the block's, restricted to the entry's word.  Compaction, table,
// barriers, the multi-scan loop and everything behind the table are the static walk's; the mode is a runtime branch in wave 0's scan,
// ahead of the block loop.  The visiting backwards keep the static walk (an empty UnitList, a compile-time constant there): dW is
// summed in visit order.
// ------------------------------------------------------------------------------------------------
constexpr int WSCAN_CHUNK = 64, WSCAN_CHUNKS = 4, WSCAN_CAP = WSCAN_CHUNK * WSCAN_CHUNKS;
constexpr int WSCAN_LDS_BYTES = 16 + WSCAN_CAP * 12;        // [count, 3 pad words][block][window lo][window hi]
// RECORD TABLE (the visiting backwards with their records switch on; scn_blk_bwd.inc).  A unit's top used to read the block's header
// from five arrays -- a trip to memory that depends on the table's block index and that everything else of the top depends on.  The
// scan knows the blocks one trip earlier: with `recs` set, wave 0 also loads the packed records (scn_blk_record.h) of the scan's first
// WSCAN_HDR_CAP live entries, all loads issued together, into a second LDS table `hdr` (eight words per entry) -- one more round trip
// per SCAN, none per unit.  An entry past the cap reads its record from global memory at the unit's top (record()).  `recs` is a
// compile-time null in every other kernel, which then carries none of this.
constexpr int WSCAN_HDR_CAP = WSCAN_CHUNK, WSCAN_HDR_BYTES = WSCAN_HDR_CAP * 32;
static_assert(sizeof(BlockRec) == 32, "eight words per record");

// the bits of block b for the 64 slabs from `first` on (bit j = slab first + j), per lane: three loads, no branch (words past the
// row: no slab)
__device__ __forceinline__ uint64_t keep_window_lane(const KeepMask km, int b, int first) {
    const uint32_t* mw = km.bits + (size_t)b * km.words;
    const int w0 = first >> 5, sh = first & 31;
    const int last = km.words - 1, w1 = w0 + 1 < last ? w0 + 1 : last, w2 = w0 + 2 < last ? w0 + 2 : last;
    const uint32_t a = mw[w0], c1 = mw[w1], d2 = mw[w2];
    const uint32_t c = w0 + 1 <= last ? c1 : 0u, d = w0 + 2 <= last ? d2 : 0u;
    uint64_t win = (((uint64_t)c << 32) | a) >> sh;
    if (sh) win |= (uint64_t)d << (64 - sh);
    return win;
}

// The walk over a workgroup's units u = first, first + stride, ... < last (block_range) whose window keep_cut(window of block(u) from
// slab0, n_it) is non-zero, WSCAN_CAP units per scan.  Across a block's slab loop it holds ONE scalar of its own, the number of scans
// done: the range is recomputed from the grid where a scan needs it, and the cursor over the table is the kernel's own unit counter
// (SCN_UNIT_BEGIN_MASKED, scn_blk_common.inc).  `on` = false (the forms without a mask): never used, the compiler drops it.  Every
// member is workgroup-uniform, and every thread of the workgroup makes the same calls (scan_units holds barriers).
struct WindowWalk {
    uint32_t* tbl;
    const int32_t* assign;
    KeepMask km;
    UnitList ul;
    int n_blocks, slab0, n_it, scans;
    const BlockRec* recs;                                             // the plan's packed records: the scan fills `hdr` (null: no record table)
    uint32_t* hdr;                                                    // LDS, WSCAN_HDR_BYTES, 16-byte aligned
    __device__ __forceinline__ WindowWalk(bool on, char* lds, int n_blocks_, const int32_t* assign_, KeepMask km_, int slab0_, int n_it_,
                                          UnitList ul_ = UnitList{nullptr, nullptr}, const BlockRec* recs_ = nullptr, char* hdr_ = nullptr)
        : tbl((uint32_t*)lds), assign(assign_), km(km_), ul(ul_), n_blocks(on ? n_blocks_ : 0), slab0(slab0_), n_it(n_it_), scans(0),
          recs(recs_), hdr((uint32_t*)hdr_) {}
    // wave 0: the WSCAN_CAP units from cu on, compacted into the table.  LIST MODE (ul.units, see below): a unit is an entry of the
    // mask's unit list -- its block comes from the entry, its window is the block's, restricted to the entry's word.
    __device__ __forceinline__ void scan(int cu, int last, int stride) {
        const int lane = threadIdx.x & 63;
        const bool lst = ul.units != nullptr;
        uint32_t ent[WSCAN_CHUNKS];
        bool ok[WSCAN_CHUNKS];
#pragma unroll
        for (int j = 0; j < WSCAN_CHUNKS; ++j) {
            const int64_t u = (int64_t)cu + (int64_t)(j * WSCAN_CHUNK + lane) * stride;
            ok[j] = u < last;
            const int uc = ok[j] ? (int)u : cu;                       // (a lane past the range reads unit cu again: no branch)
            ent[j] = lst ? ul.units[uc] : (uint32_t)(assign ? assign[uc] : uc);
        }
        int blk[WSCAN_CHUNKS];
#pragma unroll
        for (int j = 0; j < WSCAN_CHUNKS; ++j) blk[j] = lst ? unit_block(ent[j], km.words) : (int)ent[j];
        uint64_t win[WSCAN_CHUNKS];
#pragma unroll
        for (int j = 0; j < WSCAN_CHUNKS; ++j) win[j] = keep_window_lane(km, blk[j], slab0);
        int base = 0;
#pragma unroll
        for (int j = 0; j < WSCAN_CHUNKS; ++j) {
            uint64_t w = ok[j] ? keep_cut(win[j], n_it) : 0ull;
            if (lst) w = keep_word_cut(w, slab0, unit_word(ent[j], km.words));
            const uint64_t live = __builtin_amdgcn_ballot_w64(w != 0);
            const int pos = base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(live >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)live, 0u));
            if (w != 0) {                                             // (pos < WSCAN_CAP: one entry per unit at the most)
                tbl[4 + pos] = (uint32_t)blk[j];
                tbl[4 + WSCAN_CAP + pos] = (uint32_t)w;
                tbl[4 + 2 * WSCAN_CAP + pos] = (uint32_t)(w >> 32);
            }
            base += __builtin_popcountll(live);
        }
        if (lane == 0) {
            tbl[0] = (uint32_t)base;
            if (lst) tbl[1] = (uint32_t)last;                         // the list's length, parked for more()
        }
        if (recs) {                                                   // the record table: entry `lane` of the compacted table, one lane each
            static_assert(WSCAN_HDR_CAP == WSCAN_CHUNK, "one lane per entry of the record table");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // this wave's table writes have landed (other lanes wrote the entry)
            if (lane < (base < WSCAN_HDR_CAP ? base : WSCAN_HDR_CAP)) {
                const u32x4* src = (const u32x4*)(recs + tbl[4 + lane]);
                const u32x4 lo = src[0], hi = src[1];
                *(u32x4*)(hdr + lane * 8) = lo;
                *(u32x4*)(hdr + lane * 8 + 4) = hi;
            }
        }
    }
    // The record of table entry e (its block: blk), eight words as scn_blk_record.h lays them out, wave-uniform: from the record
    // table, or for an entry past its cap from global memory as one 32-byte read.  Only with `recs` set.
    __device__ __forceinline__ void record(int e, int blk, uint32_t (&w)[8]) const {
        u32x4 lo, hi;
        if (e < WSCAN_HDR_CAP) {
            lo = *(const u32x4*)(hdr + e * 8);
            hi = *(const u32x4*)(hdr + e * 8 + 4);
        } else {
            const u32x4* src = (const u32x4*)(recs + blk);
            lo = src[0];
            hi = src[1];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            w[i] = __builtin_amdgcn_readfirstlane(lo[i]);
            w[4 + i] = __builtin_amdgcn_readfirstlane(hi[i]);
        }
    }
    // first unit of the next scan and the range's end and stride.  LIST MODE: workgroup g takes entries g, g + G, g + 2 G, ... of
    // the device-wide list (G workgroups, one slab range: the dispatch sees to it), so a launch's units are spread evenly whatever
    // blocks they lie in; the list's length is one load per scan (`fresh`), and more() reads it back from the table's pad word, so
    // that the walk still holds one scalar of its own across a slab loop.
    __device__ __forceinline__ int64_t next_unit(int& last, int& stride, bool fresh) const {
        if (ul.units) {
            stride = (int)gridDim.x;
            last = (int)__builtin_amdgcn_readfirstlane(fresh ? *ul.count : tbl[1]);
            return (int64_t)blockIdx.x + (int64_t)scans * WSCAN_CAP * stride;
        }
        int first;
        block_range(n_blocks, first, last, stride);
        return (int64_t)first + (int64_t)scans * WSCAN_CAP * stride;
    }
    // whether units are left to scan (list mode: no scan done = the first one found the list too short for this workgroup)
    __device__ __forceinline__ bool more() const {
        if (ul.units && scans == 0) return false;
        int last, stride;
        return next_unit(last, stride, false) < last;
    }
    // scans the next WSCAN_CAP units (none left: no entries) and sets the table cursor: entries e = u, u + u_stride, ... < u_end
    __device__ __forceinline__ void scan_units(int& u, int& u_end, int& u_stride) {
        int last, stride;
        const int64_t cu = next_unit(last, stride, true);
        u = 0;
        u_end = 0;
        u_stride = 1;
        if (cu >= last) return;
        __syncthreads();                                              // every wave has left the previous table
        if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0) scan((int)cu, last, stride);
        __syncthreads();
        u_end = (int)__builtin_amdgcn_readfirstlane(tbl[0]);
        ++scans;
    }
    // entry e of the table: its block and its (cut, non-zero) window
    __device__ __forceinline__ int block(int e) const { return (int)__builtin_amdgcn_readfirstlane(tbl[4 + e]); }
    __device__ __forceinline__ uint64_t window(int e) const {
        const uint32_t lo = __builtin_amdgcn_readfirstlane(tbl[4 + WSCAN_CAP + e]), hi = __builtin_amdgcn_readfirstlane(tbl[4 + 2 * WSCAN_CAP + e]);
        return ((uint64_t)hi << 32) | lo;
    }
};

// Diagnostic kernel of scn_window_scan_probe: the walk on a caller-chosen grid, written out.  Workgroup g leaves its sequence in
// out_block / out_window [g * cap ..] (the first `cap` entries of it) and its length in out_count[g]; unit_block[u] = the block of
// unit u under the grid's assignment.
__global__ __launch_bounds__(256) void window_scan_probe_kernel(PlanDev P, KeepMask km, int slab0, int n_it, int cap,
                                                                int32_t* __restrict__ out_block, uint64_t* __restrict__ out_window,
                                                                int32_t* __restrict__ out_count, int32_t* __restrict__ unit_block) {
    __shared__ __attribute__((aligned(16))) char tbl[WSCAN_LDS_BYTES];
    WindowWalk walk(true, tbl, P.n_blocks, P.assign, km, slab0, n_it);
    int len = 0;
    do {
        int e, e_end, e_stride;
        walk.scan_units(e, e_end, e_stride);
        for (; e < e_end; e += e_stride) {
            if (threadIdx.x == 0 && len < cap) {
                out_block[(size_t)blockIdx.x * cap + len] = walk.block(e);
                out_window[(size_t)blockIdx.x * cap + len] = walk.window(e);
            }
            ++len;
        }
    } while (walk.more());
    if (threadIdx.x == 0) out_count[blockIdx.x] = len;
    if (unit_block)
        for (int u = blockIdx.x * 256 + threadIdx.x; u < P.n_blocks; u += gridDim.x * 256) unit_block[u] = P.assign ? P.assign[u] : u;
}
