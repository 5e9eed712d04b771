// dual SpMM kernels (two-buffer and four-stage ring) -- part of scn_blocked.hip (one translation unit; included inside namespace scn)
// ------------------------------------------------------------------------------------------------
// dual SpMM on K-float pieces (K % 4 == 0, K <= 128): ya = val0-operator * x, yb = val1-operator * x
// 16 waves per workgroup (no MFMA, few registers): thread = (row, 16-byte chunk), two items per thread;
// results are stored one slab late so the per-slab vmcnt(0) never waits on fresh stores.
// ------------------------------------------------------------------------------------------------
constexpr int Y_STRIDE = 4;      // floats per point of the shifted first-layer input y = (x, S_lo x, S_up x, 0): 16-byte records
constexpr int SP_THREADS = 1024;
constexpr int SP_ITEMS = 2;           // BK_R * 32 chunks / SP_THREADS
constexpr int SP_SLAB_GROUP = 8;      // slabs a workgroup processes per visit of a block

// A staged piece of the two-buffer SpMM is VIRTUAL: `batch` consecutive slabs of one source row side by side (K floats
// each, cpk = K/4 chunks), so that a narrow operand -- the 1-channel tensors of the first / last Bunch layer are K = 4 floats
// per row and slab: 64 work items per block -- fills the workgroup: chunk pos of a piece = chunk pos % cpk of slab pos / cpk.
// batch = 1 is the plain layout.
__device__ __forceinline__ void dma_stage_sp(const char* X, int slab0, int n_avail, size_t slab_bytes, char* buf, const Smem& sm,
                                             int nsrc, int k4, int cpk, int vcpp) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int total = nsrc * vcpp;
    const uint32_t dst0 = lds_addr_of(buf);
    for (int base = wave * 64; base < total; base += SP_THREADS) {
        const int c = base + lane;
        if (c < total) {
            const int slot = c / vcpp, pos = c - slot * vcpp;
            const int sl = pos / cpk, sub = pos - sl * cpk;
            if (sl < n_avail) {
                const char* g = X + (size_t)(slab0 + sl) * slab_bytes + (size_t)sm.srcrows[slot] * k4 + sub * 16;
                lds_dma16_v(g, dst0 + (uint32_t)(base * 16));          // (the lanes of a virtual piece read different slabs)
            }
        }
    }
}

// (plain pieces of one slab at Xs)
__device__ __forceinline__ void dma_stage_sp(const char* Xs, char* buf, const Smem& sm, int nsrc, int piece, int cpp) {
    dma_stage_sp(Xs, 0, 1, 0, buf, sm, nsrc, piece, cpp, cpp);
}

template <bool DUAL>
__global__ __launch_bounds__(SP_THREADS, 4) void spmm_blocked_kernel(PlanDev P, const float* __restrict__ X,
                                                                     float* __restrict__ ya, float* __restrict__ yb,
                                                                     int n_rows, int n_cols, int n_slabs, int K, int batch) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int k4 = K * 4, cpk = K / 4;                              // one slab's piece
    const int piece = k4 * batch, cpp = cpk * batch;                // the staged (virtual) piece
    const size_t in_slab_bytes = (size_t)n_cols * k4;
    const Smem sm = carve(smem, piece);
    uint8_t* tws = (uint8_t*)(smem + smem_bytes(piece));           // [BK_WAVES] per-row-group widths
    int b0, b_end, b_stride;
    block_range(P.n_blocks, b0, b_end, b_stride);
    const int n_units = (n_slabs + batch - 1) / batch;              // a unit = `batch` slabs (the last one may hold fewer)
    const int unit_lo = (int)((int64_t)blockIdx.y * n_units / gridDim.y), unit_hi = (int)((int64_t)(blockIdx.y + 1) * n_units / gridDim.y);
    if (unit_lo >= unit_hi) return;
    f32x4 pa[SP_ITEMS], pb[SP_ITEMS];
    int pend_slab0 = 0, pend_row0 = 0, pend_avail = 0;
    int pend_total = -1;
    auto store_pending = [&]() {
#pragma unroll
        for (int k = 0; k < SP_ITEMS; ++k) {
            const int idx = threadIdx.x + k * SP_THREADS;
            if (idx < pend_total) {
                const int r = idx / cpp, ch = idx - r * cpp;
                const int sl = ch / cpk, sub = ch - sl * cpk;
                if (sl < pend_avail) {
                    const size_t off = ((size_t)(pend_slab0 + sl) * n_rows + pend_row0 + r) * K + sub * 4;
                    // non-temporal: the outputs would otherwise evict the halo rows neighbouring blocks are about to read
                    __builtin_nontemporal_store(pa[k], (f32x4*)(ya + off));
                    if (DUAL) __builtin_nontemporal_store(pb[k], (f32x4*)(yb + off));
                }
            }
        }
    };
    // unit groups outside, blocks inside: all workgroups sweep their blocks for the same 8 slabs before moving on, which
    // keeps more of the halo rows that neighbouring blocks share within reach of the caches (-4 % at |E| = 1M; 4 or 16
    // slabs per group are worse, and so is giving a workgroup a contiguous block range)
    for (int u0 = unit_lo; u0 < unit_hi; u0 += SP_SLAB_GROUP)
    for (int bi = b0, u1 = min(u0 + SP_SLAB_GROUP, unit_hi); bi < b_end; bi += b_stride) {
        const int b = P.assign ? P.assign[bi] : bi;
        wait_all_and_barrier();
        BlockMeta m;
        {   // load_block with this kernel's thread count
            m.row0 = P.blk_row0[b];
            m.rows = P.blk_rows[b];
            const int sp0 = P.src_ptr[b];
            m.nsrc = P.src_ptr[b + 1] - sp0;
            m.w = P.width[b];
            const int ep = P.ell_ptr[b];
            for (int i = threadIdx.x; i < m.nsrc; i += SP_THREADS) sm.srcrows[i] = P.src_rows[sp0 + i];
            for (int i = threadIdx.x; i < m.w * m.rows; i += SP_THREADS) {
                sm.slot[i] = P.ell_slot[ep + i];
                sm.v[i] = P.ell_v[ep + i];
            }
            if (threadIdx.x < BK_WAVES) tws[threadIdx.x] = P.tile_w[b * BK_WAVES + threadIdx.x];
        }
        __syncthreads();
        const int total = m.rows * cpp;
        const bool wave_uniform_rows = cpp >= 8 && (64 % cpp) == 0;
        auto avail = [&](int u) { return min(batch, n_slabs - u * batch); };
        dma_stage_sp((const char*)X, u0 * batch, avail(u0), in_slab_bytes, sm.buf(0), sm, m.nsrc, k4, cpk, cpp);
        for (int u = u0; u < u1; ++u) {
            const int cur_off = ((u - u0) & 1) * sm.buf_stride;
            wait_vm_and_barrier();
            if (u + 1 < u1)
                dma_stage_sp((const char*)X, (u + 1) * batch, avail(u + 1), in_slab_bytes, sm.buf((u + 1 - u0) & 1), sm, m.nsrc, k4,
                             cpk, cpp);
            if (pend_total >= 0) store_pending();
#pragma unroll
            for (int k = 0; k < SP_ITEMS; ++k) {
                const int idx = threadIdx.x + k * SP_THREADS;
                f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
                if (idx < total) {
                    const int r = idx / cpp, ch = idx - r * cpp;
                    int tw = tws[r >> 3];
                    if (wave_uniform_rows) tw = __builtin_amdgcn_readfirstlane(tw);   // the wave's lanes share one row group
                    const int rb = r * m.w;
                    const char* cbase = sm.buf0 + cur_off + ch * 16;
#pragma unroll 2
                    for (int t = 0; t < tw; t += 2) {
                        const EllPair e = ell_load(sm, rb + t);
                        const f32x4 d0 = *(const f32x4*)(cbase + e.s0 * piece);
                        const f32x4 d1 = *(const f32x4*)(cbase + e.s1 * piece);
                        a0 += e.v[0] * d0;
                        if (DUAL) a1 += e.v[1] * d0;
                        a0 += e.v[2] * d1;
                        if (DUAL) a1 += e.v[3] * d1;
                    }
                }
                pa[k] = a0;
                pb[k] = a1;
            }
            pend_slab0 = u * batch;
            pend_avail = avail(u);
            pend_row0 = m.row0;
            pend_total = total;
        }
    }
    if (pend_total >= 0) store_pending();
}

constexpr auto spmm_blocked_single = spmm_blocked_kernel<false>;      // ya = S_a X (yb null)
constexpr auto spmm_blocked_dual = spmm_blocked_kernel<true>;         // and yb = S_b X

// ------------------------------------------------------------------------------------------------
// dual SpMM, K = 128 or 64, as a RING of four half-piece stages: the staged unit is half a row piece (K/2 floats of every
// source row), so the same 128 KB of LDS holds four stages instead of two buffers and three stages' LDS-DMAs are in flight
// while one is consumed (the two-buffer kernel has one slab in flight at a time: DMA-only it runs 9.1 ms against 7.8 for
// the traffic, profiles/HISTORY.md section 3).  NI = LDS-DMA instructions per wave and stage (BK_SRC * K/8 chunks / 1024 lanes), issued
// by EVERY wave with clamped source addresses so that `s_waitcnt vmcnt(NI * stages still in flight)` means the same thing in
// every wave; loads complete in order among loads, so counting only them is safe with the result stores in between.
// ------------------------------------------------------------------------------------------------
constexpr int RING_SLAB_GROUP = 16;   // slabs per block visit: the ring's three-stage fill makes a visit dearer than in the two-buffer kernel (8: +1 %, 32: +1 %)

template <int NI>
__device__ __forceinline__ void wait_ring(int later) {           // `later` = stages issued after the one needed (wave-uniform)
    if (later >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NI) : "memory");
    else if (later == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

template <bool DUAL, int NI>
__global__ __launch_bounds__(SP_THREADS, 4) void spmm_ring_kernel(PlanDev P, const float* __restrict__ X,
                                                                  float* __restrict__ ya, float* __restrict__ yb,
                                                                  int n_rows, int n_cols, int n_slabs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int K = 64 * NI, PIECE = K * 4, HALF = PIECE / 2, CPH = HALF / 16;     // chunks per half piece: 16 or 8
    constexpr int STAGE = BK_SRC * HALF;                                             // 32 KB / 16 KB; 4 stages = both buffers
    static_assert(BK_SRC * CPH == NI * SP_THREADS, "every lane issues exactly NI LDS-DMA chunks per stage");
    const Smem sm = carve(smem, PIECE);
    const uint32_t lds0 = lds_addr_of(smem);                  // LDS byte address of the dynamic shared memory
    uint8_t* tws = (uint8_t*)(smem + smem_bytes(PIECE));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int b0, b_end, b_stride;
    block_range(P.n_blocks, b0, b_end, b_stride);
    const int slab_lo = (int)((int64_t)blockIdx.y * n_slabs / gridDim.y), slab_hi = (int)((int64_t)(blockIdx.y + 1) * n_slabs / gridDim.y);
    if (slab_lo >= slab_hi) return;
    f32x4 pa = {0.f, 0.f, 0.f, 0.f}, pb = pa;
    float *pend_a = nullptr, *pend_b = nullptr;
    for (int slab0 = slab_lo; slab0 < slab_hi; slab0 += RING_SLAB_GROUP)
    for (int bi = b0, slab1 = min(slab0 + RING_SLAB_GROUP, slab_hi); bi < b_end; bi += b_stride) {
        const int b = P.assign ? P.assign[bi] : bi;
        wait_all_and_barrier();
        BlockMeta m;
        {
            m.row0 = P.blk_row0[b];
            m.rows = P.blk_rows[b];
            const int sp0 = P.src_ptr[b];
            m.nsrc = P.src_ptr[b + 1] - sp0;
            m.w = P.width[b];
            const int ep = P.ell_ptr[b];
            for (int i = threadIdx.x; i < m.nsrc; i += SP_THREADS) sm.srcrows[i] = P.src_rows[sp0 + i];
            for (int i = threadIdx.x; i < m.w * m.rows; i += SP_THREADS) {
                sm.slot[i] = P.ell_slot[ep + i];
                sm.v[i] = P.ell_v[ep + i];
            }
            if (threadIdx.x < BK_WAVES) tws[threadIdx.x] = P.tile_w[b * BK_WAVES + threadIdx.x];
        }
        __syncthreads();
        // this lane's NI chunks of a stage: chunk c = slot * CPH + pos, clamped into the block's sources
        // (a block of rows without entries -- isolated nodes cluster in the holes of the complex -- has no sources at all:
        // nothing is staged for it, its rows are written as zeros; has_src is uniform over the workgroup)
        uint32_t goff[NI];
        const bool has_src = m.nsrc > 0;
        const int total = m.nsrc * CPH;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = has_src ? min((i * (SP_THREADS / 64) + wave) * 64 + lane, total - 1) : 0;
            goff[i] = has_src ? (uint32_t)sm.srcrows[c / CPH] * PIECE + (c % CPH) * 16 : 0u;
        }
        const int n_stage = 2 * (slab1 - slab0);
        auto issue = [&](int q) {                                   // stage q = (slab slab0 + q/2, half q&1)
            const char* src = (const char*)X + (size_t)(slab0 + (q >> 1)) * n_cols * PIECE + (q & 1) * HALF;
            const uint32_t dst = lds0 + (uint32_t)((sm.buf0 - smem) + (q & 3) * STAGE);
#pragma unroll
            for (int i = 0; i < NI; ++i) lds_dma16(src, goff[i], dst + (uint32_t)(((i * (SP_THREADS / 64) + wave) * 64) * 16));
        };
        // SCN_SPMM_FLOOR (diagnostic builds only, tools/spmm_ceiling.sh; results are WRONG by design): 1 = LDS-DMA + stores, no
        // gather (what the memory system alone takes); 2 = gather + stores on whatever LDS holds, no LDS-DMA
#if defined(SCN_SPMM_FLOOR) && SCN_SPMM_FLOOR == 2
        const bool do_dma = false;
#else
        const bool do_dma = has_src;
#endif
        if (do_dma)
            for (int q = 0; q < 3 && q < n_stage; ++q) issue(q);
        // this thread's item of every stage: (row r, 16-byte chunk ch of the half piece)
        const int idx = threadIdx.x, r = idx / CPH, ch = idx - r * CPH;
        const bool live = r < m.rows;
#if defined(SCN_SPMM_FLOOR) && SCN_SPMM_FLOOR == 1
        const int tw = 0;
#else
        const int tw = live ? __builtin_amdgcn_readfirstlane(tws[min(r, BK_R - 1) >> 3]) : 0;   // CPH >= 8: a wave's lanes share a row group
#endif
        const int rb = r * m.w;
        for (int q = 0; q < n_stage; ++q) {
            wait_ring<NI>(min(n_stage - 1 - q, 2));
            if (do_dma && q + 3 < n_stage) issue(q + 3);
            if (pend_a) {                                           // non-temporal, one stage late (see spmm_blocked_kernel)
                __builtin_nontemporal_store(pa, (f32x4*)pend_a);
                if (DUAL) __builtin_nontemporal_store(pb, (f32x4*)pend_b);
            }
            f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
            if (live) {
                const char* cbase = sm.buf0 + (q & 3) * STAGE + ch * 16;
#pragma unroll 2
                for (int t = 0; t < tw; t += 2) {
                    const EllPair e = ell_load(sm, rb + t);
                    const f32x4 d0 = *(const f32x4*)(cbase + e.s0 * HALF);
                    const f32x4 d1 = *(const f32x4*)(cbase + e.s1 * HALF);
                    a0 += e.v[0] * d0;
                    if (DUAL) a1 += e.v[1] * d0;
                    a0 += e.v[2] * d1;
                    if (DUAL) a1 += e.v[3] * d1;
                }
            }
            pa = a0;
            pb = a1;
            const size_t off = ((size_t)(slab0 + (q >> 1)) * n_rows + m.row0 + r) * K + (q & 1) * (K / 2) + ch * 4;
            pend_a = live ? ya + off : nullptr;
            pend_b = live && DUAL ? yb + off : nullptr;
        }
    }
    if (pend_a) {
        __builtin_nontemporal_store(pa, (f32x4*)pend_a);
        if (DUAL) __builtin_nontemporal_store(pb, (f32x4*)pend_b);
    }
}

template <int NI> constexpr auto spmm_ring_single = spmm_ring_kernel<false, NI>;      // ya = S_a X (yb null); NI = K / 64
template <int NI> constexpr auto spmm_ring_dual = spmm_ring_kernel<true, NI>;         // and yb = S_b X
