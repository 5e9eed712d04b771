// device side: LDS layout, gather and pipeline helpers shared by the blocked kernels -- part of scn_blocked.hip (one translation unit; included inside namespace scn)
// ------------------------------------------------------------------------------------------------
// LDS layout and pipeline helpers
// ------------------------------------------------------------------------------------------------
// [buf0: BK_SRC*PIECE][buf1: BK_SRC*PIECE][ell_v: BK_ELL_CAP float2][srcrows: BK_SRC i32][slot: BK_ELL_CAP u8][self: BK_R u8][extra]
struct Smem {
    char* buf0;
    int buf_stride;
    __device__ __forceinline__ char* buf(int i) const { return buf0 + i * buf_stride; }
    float2* v;
    int32_t* srcrows;
    uint8_t* slot;
    uint8_t* self;
};
__host__ __device__ static inline size_t smem_bytes(int piece, int extra = 0) {
    size_t b = (size_t)2 * BK_SRC * piece + (size_t)BK_ELL_CAP * 9 + BK_SRC * 4 + BK_R;
    return ((b + 15) / 16) * 16 + extra;
}
__device__ __forceinline__ Smem carve(char* base, int piece) {
    Smem s;
    s.buf0 = base;
    s.buf_stride = BK_SRC * piece;
    s.v = (float2*)(base + 2 * BK_SRC * piece);
    s.srcrows = (int32_t*)(s.v + BK_ELL_CAP);
    s.slot = (uint8_t*)(s.srcrows + BK_SRC);
    s.self = s.slot + BK_ELL_CAP;
    return s;
}

struct BlockMeta { int row0, rows, nsrc, w; };

__device__ __forceinline__ BlockMeta load_block(const PlanDev& P, int b, const Smem& sm) {
    BlockMeta m;
    m.row0 = P.blk_row0[b];
    m.rows = P.blk_rows[b];
    const int sp0 = P.src_ptr[b];
    m.nsrc = P.src_ptr[b + 1] - sp0;
    m.w = P.width[b];
    const int ep = P.ell_ptr[b];
    for (int i = threadIdx.x; i < m.nsrc; i += BK_THREADS) sm.srcrows[i] = P.src_rows[sp0 + i];
    for (int i = threadIdx.x; i < m.w * m.rows; i += BK_THREADS) {
        sm.slot[i] = P.ell_slot[ep + i];
        sm.v[i] = P.ell_v[ep + i];
    }
    if (threadIdx.x < BK_R) sm.self[threadIdx.x] = P.self_slot[(size_t)b * BK_R + threadIdx.x];
    return m;
}

// two consecutive ELL entries of a row: slots and (val0, val1) pairs, one 2-byte and one 16-byte LDS read
struct EllPair { int s0, s1; f32x4 v; };
__device__ __forceinline__ EllPair ell_load(const Smem& sm, int idx) {
    EllPair e;
    const uint32_t ss = *(const uint16_t*)(sm.slot + idx);
    e.s0 = ss & 255;
    e.s1 = ss >> 8;
    e.v = *(const f32x4*)(sm.v + idx);
    return e;
}

// XOR swizzle of the 16-byte chunk index inside a staged piece (involution for a fixed slot): keeps the
// lane = (point, channel slice) gather spread over the LDS banks.
//   512-B pieces (C=32): chunk = n*8 + h*4 + q ; 256-B pieces (C=16): chunk = n*4 + g.
__device__ __forceinline__ int swz32(int slot, int chunk) {
    return chunk ^ ((((slot >> 1) & 1) << 2) | ((slot & 1) << 1) | ((chunk >> 4) & 1));
}
__device__ __forceinline__ int swz16(int slot, int chunk) { return chunk ^ (slot & 3); }

// ---- C = 32 (512-byte pieces): LDS carve with 16-bit pre-encoded ELL slots, and the gather built on it ----
// [buf0][buf1][ell_v: BK_ELL_CAP float2][srcrows: BK_SRC i32][enc: BK_ELL_CAP u16][self: BK_R u8][extra]
// streamed tensors of the backward (aux read once, dx written once per launch): non-temporal, so that the L2 keeps the staged
// halo rows neighbouring blocks share: -1.4 % (SCN_NO_NT: plain accesses, for A/B runs).  The forward's output stores are
// left plain: non-temporal they cost it 1-3 %.
#ifdef SCN_NO_NT
#define SCN_ST_STREAM(ptr, val) (*(ptr) = (val))
#define SCN_LD_STREAM(ptr) (*(ptr))
#else
#define SCN_ST_STREAM(ptr, val) __builtin_nontemporal_store((val), (ptr))
#define SCN_LD_STREAM(ptr) __builtin_nontemporal_load(ptr)
#endif

struct SmemC32 {
    char* buf0;
    __device__ __forceinline__ char* buf(int i) const { return buf0 + i * (BK_SRC * 512); }
    float2* v;
    int32_t* srcrows;
    uint16_t* enc;
    uint8_t* self;
};
__host__ __device__ static inline size_t smem_bytes_c32(int extra = 0) {
    size_t b = (size_t)2 * BK_SRC * 512 + (size_t)BK_ELL_CAP * 10 + BK_SRC * 4 + BK_R;
    return ((b + 15) / 16) * 16 + extra;
}
__device__ __forceinline__ SmemC32 carve_c32(char* base) {
    SmemC32 s;
    s.buf0 = base;
    s.v = (float2*)(base + 2 * BK_SRC * 512);
    s.srcrows = (int32_t*)(s.v + BK_ELL_CAP);
    s.enc = (uint16_t*)(s.srcrows + BK_SRC);
    s.self = (uint8_t*)(s.enc + BK_ELL_CAP);
    return s;
}
static_assert(BK_SRC * 512 == 65536 && BK_SRC <= 128, "gather_c32 XORs slot*512 (< 2^16) with the buffer bit 2^16");

template <int NT>
__device__ __forceinline__ BlockMeta load_block_c32(const PlanDev& P, int b, const SmemC32& sm) {
    BlockMeta m;
    m.row0 = P.blk_row0[b];
    m.rows = P.blk_rows[b];
    const int sp0 = P.src_ptr[b];
    m.nsrc = P.src_ptr[b + 1] - sp0;
    m.w = P.width[b];
    const int ep = P.ell_ptr[b];
    for (int i = threadIdx.x; i < m.nsrc; i += NT) sm.srcrows[i] = P.src_rows[sp0 + i];
    for (int i = threadIdx.x; i < m.w * m.rows; i += NT) {
        sm.enc[i] = P.ell_enc[ep + i];
        sm.v[i] = P.ell_v[ep + i];
    }
    if (threadIdx.x < BK_R) sm.self[threadIdx.x] = P.self_slot[(size_t)b * BK_R + threadIdx.x];
    return m;
}

// load_block_c32 of the visiting backwards' unit pipeline (scn_blk_bwd.inc): one round trip for the header scalars and one for the
// metadata, as there, but the second also carries the source rows of the NEXT unit's block nb (ahead: there is one) into rows_next,
// so that the current unit's last visit can stage the next unit's first slab; the block's own rows go to rows_cur unless they are
// there already (have_rows: the previous unit brought them).  The wave's tile widths ride with the header instead of waiting for
// it behind the __syncthreads() (as compiled by hipcc 7.2 the two byte loads sink back behind the barrier, and the header's loads
// split into more waited batches than load_block_c32's: profiles/visit_prefetch_ab.txt, section 3 -- the next thing to mend).
// n_next = the next block's source count (ahead only).
template <int NT>
__device__ __forceinline__ BlockMeta load_block_c32_ahead(const PlanDev& P, int b, const SmemC32& sm, int32_t* rows_cur, bool have_rows, bool ahead,
                                                          int nb, int32_t* rows_next, int& n_next, int wave, int& tw, int& twu) {
    static_assert(BK_SRC <= NT, "a block's source rows: one per thread");
    BlockMeta m;
    m.row0 = P.blk_row0[b];
    m.rows = P.blk_rows[b];
    const int sp0 = P.src_ptr[b];
    m.nsrc = P.src_ptr[b + 1] - sp0;
    m.w = P.width[b];
    const int ep = P.ell_ptr[b];
    const int np0 = P.src_ptr[nb];                                // (nb = b without a next unit)
    n_next = P.src_ptr[nb + 1] - np0;
    tw = P.tile_w[b * BK_WAVES + wave];
    twu = P.tile_wu[b * BK_WAVES + wave];
    const int t = threadIdx.x;
    const bool l0 = !have_rows && t < m.nsrc, l1 = ahead && t < n_next;
    int32_t r0 = 0, r1 = 0;
    if (l0) r0 = P.src_rows[sp0 + t];
    if (l1) r1 = P.src_rows[np0 + t];
    for (int i = t; i < m.w * m.rows; i += NT) {
        sm.enc[i] = P.ell_enc[ep + i];
        sm.v[i] = P.ell_v[ep + i];
    }
    if (t < BK_R) sm.self[t] = P.self_slot[(size_t)b * BK_R + t];
    if (l0) rows_cur[t] = r0;
    if (l1) rows_next[t] = r1;
    return m;
}

// load_block_c32_ahead with the header taken from the block's packed record (scn_blk_record.h): rw = its eight words, already in
// SGPRs (WindowWalk::record), and np0 / n_next = the next unit's source range from ITS record -- so nothing here depends on a trip to
// memory, and every load of the unit's top (own rows unless have_rows, the next unit's rows, the ELL tile in up to three pieces per
// thread, the self slots) is issued before the first of them is used: one waited batch ahead of the caller's __syncthreads(), and the
// wave's tile widths come out of the record's words, so nothing is loaded behind it.
template <int NT>
__device__ __forceinline__ BlockMeta load_block_c32_rec(const PlanDev& P, int b, const uint32_t (&rw)[8], const SmemC32& sm, int32_t* rows_cur,
                                                        bool have_rows, bool ahead, int np0, int n_next, int32_t* rows_next, int wave, int& tw,
                                                        int& twu) {
    static_assert(BK_SRC <= NT, "a block's source rows: one per thread");
    static_assert((BK_R & (BK_R - 1)) == 0, "t & (BK_R - 1) below");
    constexpr int NE = (BK_ELL_CAP + NT - 1) / NT;                // ELL entries per thread
    BlockMeta m;
    m.row0 = (int)rw[0];
    const int ep = (int)rw[1], sp0 = (int)rw[2];
    m.nsrc = (int)(rw[3] & 255u);
    m.rows = (int)(rw[3] >> 8 & 255u);
    m.w = (int)(rw[3] >> 16 & 255u);
    tw = (int)(rw[4 + (wave >> 2)] >> (8 * (wave & 3)) & 255u);
    twu = (int)(rw[6 + (wave >> 2)] >> (8 * (wave & 3)) & 255u);
    const int t = threadIdx.x, ne = m.w * m.rows;
    const bool l0 = !have_rows && t < m.nsrc, l1 = ahead && t < n_next;
    // every load is unconditional -- a thread without an element reads element 0 of the array (every plan array has one) and drops
    // it -- so that no branch and no merge of a loaded value stands between two loads: predicated, hipcc 7.2 waited for each ELL
    // piece's slots before requesting the next piece
    uint16_t enc[NE];
    float2 v[NE];
    const int32_t r0 = P.src_rows[l0 ? sp0 + t : 0], r1 = P.src_rows[l1 ? np0 + t : 0];
#pragma unroll
    for (int j = 0; j < NE; ++j) {
        const int i = t + j * NT < ne ? ep + t + j * NT : 0;
        enc[j] = P.ell_enc[i];
        v[j] = P.ell_v[i];
    }
    const uint8_t self = P.self_slot[(size_t)b * BK_R + (t & (BK_R - 1))];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NE; ++j)
        if (t + j * NT < ne) {
            sm.enc[t + j * NT] = enc[j];
            sm.v[t + j * NT] = v[j];
        }
    if (t < BK_R) sm.self[t] = self;
    if (l0) rows_cur[t] = r0;
    if (l1) rows_next[t] = r1;
    return m;
}

// Gather of one lane's NQ 16-byte chunks of row `row` from the staged 512-byte pieces: identity term gs, and the ELL row
// (entry pairs) accumulated into gl (val0 operator) and gu (val1 operator).
//  * cb[q] = (this lane's swizzled chunk index << 4) | (buffer index << 16); the LDS address of a chunk is cb[q] ^ enc with
//    enc = slot*512 | (slot&3)*32 straight from the plan: one v_xor per read instead of five address instructions -- these
//    kernels are VALU-issue bound (profiles/r01_pmc_fwd_bwd_c32_bf16.txt), so instruction count is what matters;
//  * all 2*NQ LDS reads of an entry pair are issued before the first FMA and the next pair's slots / values are fetched
//    behind them: left to itself hipcc serialises read -> s_waitcnt lgkmcnt(0) -> use under register pressure.
template <int NQ>
__device__ __forceinline__ void read_self_c32(const SmemC32& sm, int row, const uint32_t (&cb)[NQ], f32x4 (&gs)[NQ]) {
    const uint32_t slot = sm.self[row];
    const uint32_t enc = (slot << 9) | ((slot & 3) << 5);
#pragma unroll
    for (int q = 0; q < NQ; ++q) gs[q] = *(const f32x4*)(sm.buf0 + (cb[q] ^ enc));
}

template <int NQ, bool DUAL = true, bool SELF = true, bool PEEL = true>     // DUAL = false: operator with one value array, gu is left untouched
__device__ __forceinline__ void gather_c32(const SmemC32& sm, int row, int w, int tw, int twu, const uint32_t (&cb)[NQ],   // SELF = false: gs is left untouched (read_self_c32 later)
                                           f32x4 (&gs)[NQ], f32x4 (&gl)[NQ], f32x4 (&gu)[NQ]) {
#if defined(SCN_AB_GATHER_NO_PEEL) || defined(SCN_AB_GATHER_SCALAR)   // diagnostic builds: zeroed accumulators, every pair accumulates
    constexpr bool kPeel = false;
#else
    constexpr bool kPeel = PEEL;
#endif
    const char* lds = sm.buf0;
    const int rb = row * w;                                   // w is even: entry pairs are 4-byte aligned
    uint32_t ss = *(const uint32_t*)(sm.enc + rb);
    f32x4 v = *(const f32x4*)(sm.v + rb);
    {
        const uint32_t slot = sm.self[row];
        const uint32_t enc = (slot << 9) | ((slot & 3) << 5);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            if (SELF) gs[q] = *(const f32x4*)(lds + (cb[q] ^ enc));
            if (!kPeel) {                                     // zeroed accumulators, every pair accumulates
                gl[q] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (DUAL) gu[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    // the plan puts the entries of the second operator first (its pattern is a subset): entries t >= twu only feed gl.
    // `first`: the row group's first pair ASSIGNS the accumulators (no zeroing moves: 8 * NQ VALU per gather)
    auto pair = [&](int t, auto both, auto first) {
        const uint32_t e0 = ss & 0xffffu, e1 = ss >> 16;
        const f32x4 vc = v;
        f32x4 d0[NQ], d1[NQ];
        // the next pair's slots / values: in the 16-wave kernels (NQ = 2) requested AHEAD of this pair's data, so that they are the
        // oldest LDS operations in flight and the FMAs can start on counted waits as the data reads land; requested behind the data
        // hipcc 7.2 waits lgkmcnt(0) before the first FMA there (in the NQ = 4 backward it counts either way: left as it was)
        if (NQ == 2 && t + 2 < tw) {
            ss = *(const uint32_t*)(sm.enc + rb + t + 2);
            v = *(const f32x4*)(sm.v + rb + t + 2);
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) d0[q] = *(const f32x4*)(lds + (cb[q] ^ e0));
#pragma unroll
        for (int q = 0; q < NQ; ++q) d1[q] = *(const f32x4*)(lds + (cb[q] ^ e1));
        if (NQ != 2 && t + 2 < tw) {
            ss = *(const uint32_t*)(sm.enc + rb + t + 2);
            v = *(const f32x4*)(sm.v + rb + t + 2);
        }
        __builtin_amdgcn_sched_barrier(0);
#ifdef SCN_AB_GATHER_SCALAR                                   // diagnostic builds (with -fno-slp-vectorize): v_fma_f32 instead of v_pk_fma_f32
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                gl[q][j] = __builtin_fmaf(vc[0], d0[q][j], gl[q][j]);
                if (decltype(both)::value) gu[q][j] = __builtin_fmaf(vc[1], d0[q][j], gu[q][j]);
            }
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                gl[q][j] = __builtin_fmaf(vc[2], d1[q][j], gl[q][j]);
                if (decltype(both)::value) gu[q][j] = __builtin_fmaf(vc[3], d1[q][j], gu[q][j]);
            }
#else
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            if (decltype(first)::value) {
                gl[q] = vc[0] * d0[q];
                if (decltype(both)::value) gu[q] = vc[1] * d0[q];
                else if (DUAL) gu[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
                gl[q] += vc[0] * d0[q];
                if (decltype(both)::value) gu[q] += vc[1] * d0[q];
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            gl[q] += vc[2] * d1[q];
            if (decltype(both)::value) gu[q] += vc[3] * d1[q];
        }
#endif
        __builtin_amdgcn_sched_barrier(0);
    };
    int t = 0;
    if (kPeel) {
        if (tw > 0) {                                         // (tw, twu are wave-uniform)
            if (DUAL && twu > 0) pair(0, std::true_type{}, std::true_type{});
            else pair(0, std::false_type{}, std::true_type{});
            t = 2;
        } else {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                gl[q] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (DUAL) gu[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    if (DUAL)
        for (; t < twu; t += 2) pair(t, std::true_type{}, std::false_type{});
    for (; t < tw; t += 2) pair(t, std::false_type{}, std::false_type{});
}

// One LDS-DMA instruction (16 bytes per lane: global `sbase + voff` -> LDS `dst` + 16 * lane), written as inline assembly.
// hipcc 7.2 books __builtin_amdgcn_global_load_lds as a FLAT operation pending on BOTH memory counters, and while one may be
// pending it turns every LDS wait of the kernel into lgkmcnt(0): the gather then waited for all reads of an entry pair -- and the
// look-ahead entry behind them -- before its first FMA (a build without staging gets lgkmcnt(3), (2), (1), (0)).  The hardware
// counts the instruction on vmcnt only, which is what the kernels' own slab waits (inline assembly as well) wait for.  `sbase`
// and `dst_lds` (an LDS byte address: lds_addr_of) must be wave-uniform; M0 carries it (nothing else in these kernels uses M0).
__device__ __forceinline__ uint32_t lds_addr_of(const void* p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
}
__device__ __forceinline__ void lds_dma16(const char* sbase, uint32_t voff, uint32_t dst_lds) {
    const uint32_t m = __builtin_amdgcn_readfirstlane(dst_lds);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" : : "s"(m), "v"(voff), "s"(sbase) : "memory");
}

__device__ __forceinline__ void lds_dma4(const char* sbase, uint32_t voff, uint32_t dst_lds) {     // 4 bytes per lane
    const uint32_t m = __builtin_amdgcn_readfirstlane(dst_lds);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2" : : "s"(m), "v"(voff), "s"(sbase) : "memory");
}
__device__ __forceinline__ void lds_dma16_v(const char* vaddr, uint32_t dst_lds) {       // per-lane 64-bit source address
    const uint32_t m = __builtin_amdgcn_readfirstlane(dst_lds);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" : : "s"(m), "v"(vaddr) : "memory");
}

// LDS-DMA of nsrc pieces of slab-base Xs into buf: LDS image is lane-linear, the swizzle goes on the SOURCE chunk.
template <int PIECE, int SWZ>
__device__ __forceinline__ void dma_stage(const char* Xs, char* buf, const Smem& sm, int nsrc) {
    constexpr int CPP = PIECE / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int total = nsrc * CPP;
    const uint32_t dst0 = lds_addr_of(buf);
    for (int base = wave * 64; base < total; base += BK_THREADS) {
        const int c = base + lane;
        if (c < total) {
            const int slot = c / CPP, pos = c % CPP;
            int d = pos;
            if (SWZ == 32) d = swz32(slot, pos);
            if (SWZ == 16) d = swz16(slot, pos);
            lds_dma16(Xs, (uint32_t)sm.srcrows[slot] * PIECE + d * 16, dst0 + (uint32_t)(base * 16));   // (n_cols * PIECE < 2^32: plan guard)
        }
    }
}
__device__ __forceinline__ void wait_all_and_barrier() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
__device__ __forceinline__ void wait_vm_and_barrier() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// XCD-contiguous block range of this workgroup: blocks b = first, first+stride, ... < last
__device__ __forceinline__ void block_range(int n_blocks, int& first, int& last, int& stride) {
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    stride = gridDim.x >> 3;
    const int b0 = (int)((int64_t)n_blocks * xcd / 8);
    last = (int)((int64_t)n_blocks * (xcd + 1) / 8);
    first = b0 + j;
}

#define SCN_SLAB_RANGE() \
    const int slab0 = (int)((int64_t)blockIdx.y * n_slabs / gridDim.y), slab1 = (int)((int64_t)(blockIdx.y + 1) * n_slabs / gridDim.y)

// Work units of a kernel that accepts a WorkList `wl`: dense = (every block) x (this workgroup's slab range); listed = the
// listed blocks, each with its own slab list (gridDim.y == 1).  SCN_UNIT_BEGIN opens the unit loop and defines b (block),
// k0 / n_it (first entry / trip count) and SLAB_AT(it); all of it is wave-uniform (scalar loads).
#define SCN_UNIT_RANGE()                                                             \
    const bool listed = wl.block != nullptr;                                         \
    int u_, u_end_, u_stride_;                                                       \
    block_range(listed ? wl.n_work : P.n_blocks, u_, u_end_, u_stride_);             \
    SCN_SLAB_RANGE()
#define SCN_UNIT_BEGIN()                                                             \
    for (; u_ < u_end_; u_ += u_stride_) {                                           \
        const int b = listed ? wl.block[u_] : (P.assign ? P.assign[u_] : u_);        \
        const int k0 = listed ? wl.ptr[u_] : slab0;                                  \
        const int n_it = listed ? wl.ptr[u_ + 1] - k0 : slab1 - slab0;               \
        if (n_it <= 0) continue;
// The unit loop of a kernel that also has MASKED forms (MASKED: a compile-time constant; dense launches): there the units are the
// entries of the workgroup's batched window scan (WindowWalk, scn_window_scan.inc; its table lives at LDS, WSCAN_LDS_BYTES of the
// launch's dynamic LDS) -- the same blocks in the same ascending unit order, minus the ones whose window is empty -- and win_ is the
// unit's window, cut to this workgroup's slab range and non-zero.  The loop is SCN_UNIT_BEGIN's, token for token: a masked form points
// its counters at the table (u_ = entry, u_end_ = entries, u_stride_ = 1) and comes back for the next WSCAN_CAP units behind the loop
// (SCN_UNIT_END_MASKED, after the loop's closing brace), so the walk costs a masked form one scalar across its slab loop (the scans
// done) and a form without a mask nothing.  SCN_WINDOW_WALK declares the walk, once, behind SCN_UNIT_RANGE(); UL: the mask's unit list
// (the forward-side launches; WindowWalk's list mode) or an empty one.
#define SCN_WINDOW_WALK(MASKED, KM, LDS, UL) WindowWalk walk_((MASKED), (LDS), P.n_blocks, P.assign, (KM), slab0, slab1 - slab0, (UL))
// (the visiting backwards: RECS / HDR = the plan's packed records and the LDS record table the scans fill, or null -- WindowWalk::record)
#define SCN_WINDOW_WALK_RECS(MASKED, KM, LDS, UL, RECS, HDR) \
    WindowWalk walk_((MASKED), (LDS), P.n_blocks, P.assign, (KM), slab0, slab1 - slab0, (UL), (RECS), (HDR))
#define SCN_UNIT_BEGIN_MASKED(MASKED)                                                \
    scn_next_units_:                                                                 \
    if (MASKED) walk_.scan_units(u_, u_end_, u_stride_);                             \
    for (; u_ < u_end_; u_ += u_stride_) {                                           \
        const int b = (MASKED) ? walk_.block(u_) : (listed ? wl.block[u_] : (P.assign ? P.assign[u_] : u_)); \
        const uint64_t win_ = (MASKED) ? walk_.window(u_) : ~0ull;                   \
        const int k0 = listed ? wl.ptr[u_] : slab0;                                  \
        const int n_it = listed ? wl.ptr[u_ + 1] - k0 : slab1 - slab0;               \
        if (n_it <= 0) continue;
#define SCN_UNIT_END_MASKED(MASKED) \
    if ((MASKED) && walk_.more()) goto scn_next_units_
#define SLAB_AT(it) (listed ? wl.slab[k0 + (it)] : k0 + (it))
// the same as a scalar: the readfirstlane sits INSIDE the listed arm, so that the vector load of the list entry and its s_waitcnt
// vmcnt(0) -- a wait for every LDS-DMA and store the wave has in flight -- stay out of the dense path, whose slab index then never
// leaves the scalar unit (16-wave forward: -1 %).  Not used in the backward: there hipcc 7.2 answers it (and a scalar load of the
// entry alike) by turning the gather loop's counted lgkmcnt waits into lgkmcnt(0), +2-4 %.
#define SLAB_AT_U(it) (listed ? __builtin_amdgcn_readfirstlane(wl.slab[k0 + (it)]) : k0 + (it))
