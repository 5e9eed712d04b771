// first-layer weight gradient streams, work-list helpers, fixed-order reductions -- part of scn_blocked.hip (one translation unit; included inside namespace scn)
// ------------------------------------------------------------------------------------------------
// First-layer weight gradient with the shift moved to the cheap side (scn_conv_dw_first):
//   dW_g[0][c] = sum_p (S_g x)[p] * dz[p][c]     instead of     sum_p x[p] * (S_g^T dz)[p][c]
// gather3_c1_kernel computes Y[p] = (x, S_lo x, S_up x)[p] from the 16-byte input pieces (the gather of fwd_c1, 12 bytes per
// point out); dw_first_stream_kernel then reads dz exactly once, coalesced, with no LDS gather at all -- an HBM stream.
// ------------------------------------------------------------------------------------------------
// KEEP (gather3_c1_keep_kernel): only the (block, slab) items of a keep mask are visited, as in fwd_c32_w16_kernel<KEEP> -- the blocks
// with a kept slab and their windows from the batched scan (scn_window_scan.inc), the slab loop over a window's set bits (scn_keep_bits.h).
// The records of a kept item are the plain kernel's bits, every other row of Y is left untouched; X is read in full (it is the input).
template <bool KEEP>
__device__ __forceinline__ void gather3_c1_body(const PlanDev& P, const float* __restrict__ X, float* __restrict__ Y, int n_rows,
                                                int n_cols, int n_slabs, const KeepMask km, const UnitList ul) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PIECE = 16;
    const Smem sm = carve(smem, PIECE);
    const int tid = threadIdx.x;
    int u, b_end, b_stride;
    block_range(P.n_blocks, u, b_end, b_stride);
    SCN_SLAB_RANGE();
    if (slab0 >= slab1) return;
    // KEEP: the blocks of this workgroup that have a kept slab, from the batched scan ahead of the loop (scn_window_scan.inc; its
    // table sits behind the kernel's own LDS)
    WindowWalk walk(KEEP, smem + smem_bytes(PIECE), P.n_blocks, nullptr, km, slab0, slab1 - slab0, ul);
next_units:
    if (KEEP) walk.scan_units(u, b_end, b_stride);                // (u, b_end, b_stride now walk the scan's table)
    for (; u < b_end; u += b_stride) {
        const int b = KEEP ? walk.block(u) : u;
        uint64_t keep = KEEP ? walk.window(u) : ~0ull;            // KEEP: the cursor, its lowest set bit is the next visit's slab
        wait_all_and_barrier();
        const BlockMeta m = load_block(P, b, sm);
        __syncthreads();
        const int tw = tid < m.rows * BK_NS ? P.tile_w[b * BK_WAVES + (tid >> 5)] : 0;   // (not in the slab loop: see fwd_c1_kernel)
        auto visit = [&](int slab, int it, int next) {            // slab `slab` staged in buffer it & 1; next: the slab to stage meanwhile, or -1
            const float* st = (const float*)sm.buf(it & 1);
            wait_vm_and_barrier();
            if (next >= 0)
                dma_stage<PIECE, 0>((const char*)X + (size_t)next * n_cols * PIECE, sm.buf((it + 1) & 1), sm, m.nsrc);
            if (tid < m.rows * BK_NS) {
                const int rt = tid >> 2, n = tid & 3;
                float zs = st[sm.self[rt] * 4 + n], zl = 0.f, zu = 0.f;
                const int rb = rt * m.w;
                for (int t = 0; t < tw; t += 2) {
                    const EllPair e = ell_load(sm, rb + t);
                    const float d0 = st[e.s0 * 4 + n], d1 = st[e.s1 * 4 + n];
                    zl = fmaf(e.v[0], d0, zl);
                    zu = fmaf(e.v[1], d0, zu);
                    zl = fmaf(e.v[2], d1, zl);
                    zu = fmaf(e.v[3], d1, zu);
                }
                *(f32x4*)(Y + (((size_t)slab * n_rows + m.row0) * BK_NS + tid) * Y_STRIDE) = f32x4{zs, zl, zu, 0.f};
            }
        };
        if (KEEP) {
            dma_stage<PIECE, 0>((const char*)X + (size_t)(slab0 + keep_first(keep)) * n_cols * PIECE, sm.buf(0), sm, m.nsrc);
            for (int it = 0; keep; ++it) {
                const int slab = slab0 + keep_first(keep);
                keep = keep_next(keep);
                visit(slab, it, keep ? slab0 + keep_first(keep) : -1);
            }
        } else {
            dma_stage<PIECE, 0>((const char*)X + (size_t)slab0 * n_cols * PIECE, sm.buf(0), sm, m.nsrc);
            for (int slab = slab0; slab < slab1; ++slab) visit(slab, slab - slab0, slab + 1 < slab1 ? slab + 1 : -1);
        }
    }
    if (KEEP && walk.more()) goto next_units;
}
__global__ __launch_bounds__(BK_THREADS, 2) void gather3_c1_kernel(PlanDev P, const float* __restrict__ X,
                                                                   float* __restrict__ Y, int n_rows, int n_cols,
                                                                   int n_slabs) {
    gather3_c1_body<false>(P, X, Y, n_rows, n_cols, n_slabs, KeepMask{nullptr, 0}, UnitList{nullptr, nullptr});
}
__global__ __launch_bounds__(BK_THREADS, 2) void gather3_c1_keep_kernel(PlanDev P, const float* __restrict__ X,
                                                                        float* __restrict__ Y, int n_rows, int n_cols,
                                                                        int n_slabs, KeepMask km, UnitList ul) {
    gather3_c1_body<true>(P, X, Y, n_rows, n_cols, n_slabs, km, ul);
}

constexpr int DWS_THREADS = 256, DWS_BLOCKS = 1024;
template <int C>
__global__ __launch_bounds__(DWS_THREADS) void dw_first_stream_kernel(const float* __restrict__ Y,
                                                                      const float* __restrict__ DZ,
                                                                      float* __restrict__ partial, int64_t n_points) {
    constexpr int CQ = C / 4;                                     // channel quads per point; DWS_THREADS % CQ == 0
    __shared__ f32x4 red[3 * DWS_THREADS];
    const int tid = threadIdx.x;
    const int64_t total = n_points * CQ, stride = (int64_t)gridDim.x * DWS_THREADS;
    f32x4 acc[3];
    acc[0] = acc[1] = acc[2] = f32x4{0.f, 0.f, 0.f, 0.f};
    int64_t i = (int64_t)blockIdx.x * DWS_THREADS + tid;
    for (; i + 3 * stride < total; i += 4 * stride) {            // four independent 16-byte loads in flight per thread
        f32x4 d[4];
        float y[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t j = i + u * stride;
            d[u] = *(const f32x4*)(DZ + j * 4);
            const f32x4 yq = *(const f32x4*)(Y + (j / CQ) * Y_STRIDE);
            y[u][0] = yq[0]; y[u][1] = yq[1]; y[u][2] = yq[2];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc[0] += y[u][0] * d[u];
            acc[1] += y[u][1] * d[u];
            acc[2] += y[u][2] * d[u];
        }
    }
    for (; i < total; i += stride) {
        const f32x4 d = *(const f32x4*)(DZ + i * 4);
        const float* yp = Y + (i / CQ) * Y_STRIDE;
        acc[0] += yp[0] * d;
        acc[1] += yp[1] * d;
        acc[2] += yp[2] * d;
    }
#pragma unroll
    for (int g = 0; g < 3; ++g) red[g * DWS_THREADS + tid] = acc[g];
    __syncthreads();
    if (tid < 3 * CQ) {                                           // threads with equal tid % CQ hold the same channels
        const int g = tid / CQ, cq = tid - g * CQ;
        f32x4 sum = {0.f, 0.f, 0.f, 0.f};
        for (int t = cq; t < DWS_THREADS; t += CQ) sum += red[g * DWS_THREADS + t];
        float* outp = partial + (size_t)blockIdx.x * (3 * C) + g * C + cq * 4;
        outp[0] = sum[0]; outp[1] = sum[1]; outp[2] = sum[2]; outp[3] = sum[3];
    }
}

// Zero-skipping variants of the two streaming pieces: one work item = (listed block, one of its slabs) = a contiguous run of
// rows*ns points.  dw_first_list_kernel accumulates like dw_first_stream_kernel over the listed items only (everything else
// of dz is exactly zero); clear_list_kernel writes zeros over the listed items of a [S][rows][ns][c] tensor, which returns
// a buffer of the zero-skipping mode to its all-zero state.
template <int C>
__global__ __launch_bounds__(DWS_THREADS) void dw_first_list_kernel(PlanDev P, WorkList wl, const float* __restrict__ Y,
                                                                    const float* __restrict__ DZ,
                                                                    float* __restrict__ partial, int n_rows) {
    constexpr int CQ = C / 4;
    __shared__ f32x4 red[3 * DWS_THREADS];
    const int tid = threadIdx.x;
    f32x4 acc[3];
    acc[0] = acc[1] = acc[2] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int u = blockIdx.x; u < wl.n_work; u += gridDim.x) {
        const int b = wl.block[u];
        const int row0 = P.blk_row0[b], rows = P.blk_rows[b];
        const int count = rows * BK_NS * CQ;                      // float4 items of the block's rows in one slab
        for (int k = wl.ptr[u]; k < wl.ptr[u + 1]; ++k) {
            const size_t p0 = ((size_t)wl.slab[k] * n_rows + row0) * BK_NS;   // first point
            for (int i = tid; i < count; i += DWS_THREADS) {     // i % CQ == tid % CQ: DWS_THREADS % CQ == 0
                const f32x4 d = *(const f32x4*)(DZ + (p0 * CQ + i) * 4);
                const float* yp = Y + (p0 + i / CQ) * Y_STRIDE;
                acc[0] += yp[0] * d;
                acc[1] += yp[1] * d;
                acc[2] += yp[2] * d;
            }
        }
    }
#pragma unroll
    for (int g = 0; g < 3; ++g) red[g * DWS_THREADS + tid] = acc[g];
    __syncthreads();
    if (tid < 3 * CQ) {
        const int g = tid / CQ, cq = tid - g * CQ;
        f32x4 sum = {0.f, 0.f, 0.f, 0.f};
        for (int t = cq; t < DWS_THREADS; t += CQ) sum += red[g * DWS_THREADS + t];
        float* outp = partial + (size_t)blockIdx.x * (3 * C) + g * C + cq * 4;
        outp[0] = sum[0]; outp[1] = sum[1]; outp[2] = sum[2]; outp[3] = sum[3];
    }
}

__global__ __launch_bounds__(256) void clear_list_kernel(PlanDev P, WorkList wl, float* __restrict__ T, int n_rows,
                                                         int row_floats) {
    for (int u = blockIdx.x; u < wl.n_work; u += gridDim.x) {
        const int b = wl.block[u];
        const int row0 = P.blk_row0[b], count = P.blk_rows[b] * row_floats / 4;
        for (int k = wl.ptr[u]; k < wl.ptr[u + 1]; ++k) {
            f32x4* t = (f32x4*)(T + ((size_t)wl.slab[k] * n_rows + row0) * row_floats);
            for (int i = threadIdx.x; i < count; i += 256) t[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
}

// The mask-driven twin: +0 over the block's rows of slab s for every set bit (b, s) of a mask of scn_keep_mask's geometry (a bit at or
// past n_slabs names no slab).  Plain 16-byte vector stores, no atomics; a workgroup walks a listed block's words with scalar loads.
// The workgroup's blocks b = blockIdx.x + k * gridDim.x are tested FIRST, one per thread with all loads in flight together (256 per
// pass), and the non-empty ones listed in LDS; only those are then walked (a zero store is the same in any order).
// (the body: workgroup `bid` of `grid`, its first 256 threads -- the kernel below, and a role of the step epilogue)
__device__ __forceinline__ void clear_mask_body(int bid, int grid, const PlanDev& P, KeepMask km, float* __restrict__ T, int n_rows,
                                                int n_slabs, int row_floats) {
    __shared__ int32_t live[256];
    __shared__ int32_t n_live;
    for (int64_t b0 = bid; b0 < P.n_blocks; b0 += (int64_t)grid * 256) {
        if (threadIdx.x == 0) n_live = 0;
        __syncthreads();
        const int64_t bt = b0 + (int64_t)threadIdx.x * grid;
        if (bt < P.n_blocks) {
            const uint32_t* tw = km.bits + (size_t)bt * km.words;
            uint32_t any = 0;
            for (int w = 0; w < km.words; ++w) any |= tw[w];
            if (any) live[atomicAdd(&n_live, 1)] = (int32_t)bt;
        }
        __syncthreads();
        const int n = n_live;
        for (int j = 0; j < n; ++j) {
            const int b = __builtin_amdgcn_readfirstlane(live[j]);
            const uint32_t* mw = km.bits + (size_t)b * km.words;
            const int row0 = P.blk_row0[b], count = P.blk_rows[b] * row_floats / 4;
            for (int w = 0; w < km.words; ++w) {
                for (uint32_t bits = mw[w]; bits; bits &= bits - 1) {
                    const int s = 32 * w + __builtin_ctz(bits);
                    if (s >= n_slabs) break;
                    f32x4* t = (f32x4*)(T + ((size_t)s * n_rows + row0) * row_floats);
                    for (int i = threadIdx.x; i < count; i += 256) t[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
        }
        __syncthreads();                                          // (the list is rewritten by the next pass)
    }
}
__global__ __launch_bounds__(256) void clear_mask_kernel(PlanDev P, KeepMask km, float* __restrict__ T, int n_rows, int n_slabs,
                                                         int row_floats) {
    clear_mask_body(blockIdx.x, gridDim.x, P, km, T, n_rows, n_slabs, row_floats);
}

// dW_slot[0][cc] += sum over the stream kernel's partials: one wave per output element, lane l adds partials l, l+64, ...
// and the 64 lane sums are folded in a fixed butterfly order (deterministic).
__device__ __forceinline__ void dw_first_reduce_body(int o, int lane, const float* __restrict__ partial, int n_partials, int c,
                                                     float* __restrict__ dW0, float* __restrict__ dW1, float* __restrict__ dW2) {
    // o = slot * c + cc
    float s = 0.f;
    for (int b = lane; b < n_partials; b += 64) s += partial[(size_t)b * (3 * c) + o];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0) {
        const int slot = o / c, cc = o - slot * c;
        float* d = slot == 0 ? dW0 : (slot == 1 ? dW1 : dW2);
        d[cc] += s;
    }
}
__global__ __launch_bounds__(64) void dw_first_reduce_kernel(const float* __restrict__ partial, int n_partials, int c,
                                                             float* __restrict__ dW0, float* __restrict__ dW1,
                                                             float* __restrict__ dW2) {
    dw_first_reduce_body(blockIdx.x, threadIdx.x, partial, n_partials, c, dW0, dW1, dW2);
}

// dW_slot[i] += sum over partials.  layout: partial[b][ca*3c + slot*c + cc].  One workgroup per 64 outputs: wave w adds the
// partials w, w + 16, ... (lanes = outputs: coalesced rows), the sixteen wave sums are combined in a fixed order -- deterministic,
// and a handful of independent loads per thread instead of one thread walking all partials (60 us per launch on a small complex,
// where the grid splits blocks x slabs into several hundred partials: the dearest kernel of that step).
__device__ __forceinline__ void blocked_dw_reduce_body(int bid, const float* __restrict__ partial, int n_partials, int c_aux, int c,
                                                       float* __restrict__ dW0, float* __restrict__ dW1, float* __restrict__ dW2) {
    __shared__ float part[16][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = bid * 64 + lane;
    const int per = c_aux * 3 * c;
    float s = 0.f;
    if (i < per) {
        int b = w;
        for (; b + 48 < n_partials; b += 64) {
            const float a0 = partial[(size_t)b * per + i], a1 = partial[(size_t)(b + 16) * per + i],
                        a2 = partial[(size_t)(b + 32) * per + i], a3 = partial[(size_t)(b + 48) * per + i];
            s += a0; s += a1; s += a2; s += a3;
        }
        for (; b < n_partials; b += 16) s += partial[(size_t)b * per + i];
    }
    part[w][lane] = s;
    __syncthreads();
    if (w == 0 && i < per) {
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) t += part[j][lane];
        const int ca = i / (3 * c), rem = i - ca * 3 * c, slot = rem / c, cc = rem - slot * c;
        float* d = slot == 0 ? dW0 : (slot == 1 ? dW1 : dW2);
        if (d) d[ca * c + cc] += t;
    }
}
__global__ __launch_bounds__(1024) void blocked_dw_reduce(const float* __restrict__ partial, int n_partials, int c_aux, int c,
                                                          float* __restrict__ dW0, float* __restrict__ dW1, float* __restrict__ dW2) {
    blocked_dw_reduce_body(blockIdx.x, partial, n_partials, c_aux, c, dW0, dW1, dW2);
}
