// fused layer backward kernel (f16 hi + lo split on the MFMA; plain, power, slab-pair and fused-first forms) -- part of scn_blocked.hip (one translation unit; included inside namespace scn)
// ------------------------------------------------------------------------------------------------
// backward, c_dz = c_aux = 32 on the f16 MFMA with the two-way split of scn_blk_fwd.inc (v_mfma_f32_32x32x16_f16, three products):
//   dgrad      D[pt][ca]  = sum_{g,c} G_g[pt][c] W_g[ca][c]   A = split(G_g sG) in its gather layout (lane = point p, channels
//                           16h+8t+j), B = split(W_g sW) fragments kept in LDS (12 KB)
//   transpose  T_g[pt][c] = sum_k G_g[pt][k] I[k][c]           the same A fragments against a 0/1 selection matrix: the D
//                           layout hands every lane 16 points of ONE channel (exact: each part is an f16 value), which is
//                           the B operand the weight gradient needs -- no LDS round trip, the pack is an exact conversion
//   dW_g       D[ca][c]  += sum_pt aux[pt][ca] T_g[pt][c]      A = split(aux tile sigma) straight from the dgrad D layout
// 48 MFMAs per 32-point tile (the three-way bf16 split of rounds 1-4: 90) and 2 VALU instructions per split value (5.5).
// Scales (powers of two, wave-uniform, all bookkeeping on the scalar unit).  The weight gradient contracts over the POINTS of a
// tile, so G gets ONE scale sG = 2^eG per 32-point tile (from the largest of the tile's 32 x 96 gathered values); the input gradient
// is un-scaled with 1 / (sG sW) in its act' multiply.  The tile's contribution to dW must land in an accumulator that lives across
// tiles: the wave keeps a running exponent E = min over its tiles so far of (eG + eA) (eA: the exponent the aux tile could take
// on its own; 14 under tanh, |aux| <= 1) and splits the aux tile with sigma = 2^(E - eG) <= 2^eA, so that every MFMA adds
// (true product) 2^E; when a tile lowers E the accumulators are multiplied by 2^(E_new - E_old) first (exact), and by 2^-E at the
// end.  A tile far below the wave's largest loses low bits RELATIVE TO THAT LARGEST tile only -- the error of the sum stays
// <= ~3 * 2^-22 * sum |aux G|.
// ------------------------------------------------------------------------------------------------
constexpr int B32_WFRAG_BYTES = 3 * 2 * 2 * 64 * 16;      // [segment][k-step][hi, lo][lane] x 8 f16
// 2^k as a float, k clamped to the normal range
__device__ __forceinline__ float exp2i(int k) {
    k = k < -126 ? -126 : (k > 127 ? 127 : k);
    return __uint_as_float((uint32_t)(k + 127) << 23);
}
// eG of pow2_scale(mbits): the scale is 2^(141 - biased exponent), exponent clamped as there
__device__ __forceinline__ int pow2_scale_exp(uint32_t mbits) {
    uint32_t e = mbits >> 23 & 0xffu;
    e = e < 15u ? 15u : (e > 254u ? 254u : e);
    return 141 - (int)e;
}
// Wave priorities of the 8-wave backward (two waves per SIMD, arbitrated by priority, then AGE).  Default (0): gather 3, dgrad
// chain 1, last dW chain 0.  A/B switch SCN_BWD_PRIO: 1 = one level per segment (gather 3, segments 2 / 1 / 0: the wave that is
// behind always outranks the one ahead); 2 = the default with the YOUNGER wave of every SIMD (waves 4-7) one level up.
#ifndef SCN_BWD_PRIO
#define SCN_BWD_PRIO 0
#endif
#if SCN_BWD_PRIO == 1
#define SCN_BWD_PRIO_GATHER() __builtin_amdgcn_s_setprio(3)
#define SCN_BWD_PRIO_DGRAD()
#define SCN_BWD_PRIO_SEG(u) do { if ((u) == 0) __builtin_amdgcn_s_setprio(2); if ((u) == 1) __builtin_amdgcn_s_setprio(1); if ((u) == 2) __builtin_amdgcn_s_setprio(0); } while (0)
#define SCN_BWD_PRIO_DW()
#elif SCN_BWD_PRIO == 2
#define SCN_BWD_PRIO_GATHER() do { if (wave >= 4) __builtin_amdgcn_s_setprio(3); else __builtin_amdgcn_s_setprio(2); } while (0)
#define SCN_BWD_PRIO_DGRAD() do { if (wave >= 4) __builtin_amdgcn_s_setprio(2); else __builtin_amdgcn_s_setprio(1); } while (0)
#define SCN_BWD_PRIO_SEG(u)
#define SCN_BWD_PRIO_DW() do { if (wave >= 4) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0); } while (0)
#else
#define SCN_BWD_PRIO_GATHER() __builtin_amdgcn_s_setprio(3)
#define SCN_BWD_PRIO_DGRAD() __builtin_amdgcn_s_setprio(1)
#define SCN_BWD_PRIO_SEG(u)
#define SCN_BWD_PRIO_DW() __builtin_amdgcn_s_setprio(0)
#endif
constexpr int B32_EXTRA_BYTES = B32_WFRAG_BYTES + 2048 + 64;   // weight fragments, selection fragments, one word per wave (weights_abs_max)
static_assert(B32_EXTRA_BYTES <= 160 * 1024 - (2 * BK_SRC * 512 + BK_ELL_CAP * 10 + BK_SRC * 4 + BK_R + 16), "weight + selection fragments fit behind the staging buffers");

// FORM: the kernel's form, an OR of the BWD_* bits below; the kernel's first lines name them and assert which combinations exist.
// What DZ0 carries depends on the form, and has ONE name each (top of the kernel): dz_own (EXT0), dx_partial (ACCUM), y_rec (FIRST);
// it is null in every other form.  A mask (DZMASK's source mask, VISIT's visit mask) comes typed, in `km`, the launch's flags in `flags`, and the plan's
// packed block records (VISIT; null elsewhere) in `recs`.
// EXT0 (see fwd_c32_w16_kernel): segment 0 of G is the upstream gradient itself (DZ0, own rows from HBM), the staged tensor
// DZ is S^T dz: segment 1 its own row, segment 2 its gathered shift (S^T)^2 dz.  Composes with PAIR (Ebli at hidden 16).
// PAIR: C = 16 on TWO slabs per visit -- the staged 512-byte piece is a point's 32 VIRTUAL channels (slab A's 16, slab B's 16:
// the LDS-DMA's per-lane source address does the pairing), the weights are the block-diagonal diag(W, W), and aux / dx /
// the weight-gradient blocks are addressed per slab; everything between is the C = 32 kernel as it stands.
// y broadcast of the FIRST variant below.  A 32-point tile needs 16 points x 3 values of y per half wave (PAIR: per 16-lane group:
// slab A's channels, slab B's).  Lane 16 s + j of register q holds value 16 q + j of its group's 48 values [r][g] -- so both 16-lane
// rows of a half (plain form) hold the same sixteen values -- and DPP row_newbcast:j hands lane j of its OWN row to every lane of
// the row: no LDS crossbar (ds_swizzle: 48 more LDS-pipe instructions per tile until round 3), one VALU move per value at most
// (the compiler may fold it into the FMA as a DPP operand).
template <int R>
__device__ __forceinline__ void first_dw_step(const float (&yv)[3], float dx, float (&dwf)[3]) {
#ifndef SCN_FIRST_DPP_MOV     // default: the broadcast as the DPP operand of the FMA itself, one instruction per value (the compiler emits
                              // v_mov_b32_dpp + v_fmac: +0.8 % against ds_swizzle, the fused form -1.3 %; profiles/r04_first_dpp_ab.txt).
                              // Inline assembly hides the instruction from the hazard recogniser: a DPP source written by the VALU instruction
                              // just before needs two wait states, so the first use of each y register carries its own s_nop 1.
#define SCN_Y_FMA(G) do { if ((3 * R + G) % 16 == 0) \
        asm volatile("s_nop 1\n\tv_fmac_f32_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0xf" : "+v"(dwf[G]) : "v"(yv[(3 * R + G) / 16]), "v"(dx)); \
    else asm volatile("v_fmac_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" \
             : "+v"(dwf[G]) : "v"(yv[(3 * R + G) / 16]), "v"(dx), "n"((3 * R + G) % 16)); } while (0)
    SCN_Y_FMA(0); SCN_Y_FMA(1); SCN_Y_FMA(2);
#undef SCN_Y_FMA
#else
#define SCN_Y_BCAST(G) \
    __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(yv[(3 * R + G) / 16]), 0x150 + ((3 * R + G) % 16), 0xf, 0xf, false))
    dwf[0] = fmaf(SCN_Y_BCAST(0), dx, dwf[0]);
    dwf[1] = fmaf(SCN_Y_BCAST(1), dx, dwf[1]);
    dwf[2] = fmaf(SCN_Y_BCAST(2), dx, dwf[2]);
#undef SCN_Y_BCAST
#endif
}
template <int... Rs>
__device__ __forceinline__ void first_dw_tile(std::integer_sequence<int, Rs...>, const float (&yv)[3], const f32x16& dx,
                                              float (&dwf)[3]) {
    (first_dw_step<Rs>(yv, dx[Rs], dwf), ...);
}

// the aux-free form's side of the same hand-over: value I of the lane group's 48, and the first layer's output at point pt(R, h) in
// this lane's channel rebuilt from its three (first_layer_value: what fwd_c1_kernel stores)
template <int I>
__device__ __forceinline__ float first_y_at(const float (&yv)[3]) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(yv[I / 16]), 0x150 + (I % 16), 0xf, 0xf, false));
}
template <int ACT, int... Rs>
__device__ __forceinline__ void first_aux_tile(std::integer_sequence<int, Rs...>, const float (&yv)[3], const float (&fwp)[3],
                                               float (&a)[16]) {
    ((a[Rs] = first_layer_value(ACT, first_y_at<3 * Rs>(yv), first_y_at<3 * Rs + 1>(yv), first_y_at<3 * Rs + 2>(yv), fwp[0], fwp[1],
                                fwp[2])), ...);
}

// FIRST: this layer's input is the FIRST layer's output (aux = H1 = act(y . W_first), y = the shifted 1-channel input saved by
// scn_conv_forward_first).  The input gradient dx = dL/d(pre-activation of layer 1) is then needed for one thing only -- the
// first layer's weight gradient dW_first[g][c] = sum_p y[p][g] dx[p][c] -- so it is contracted with y right here, in registers
// (y is broadcast across the lanes of a half wave with ds_swizzle: 48 cross-lane reads + 48 FMAs per tile), and never written:
// no 4*E*C-byte dx tensor, no separate streaming kernel over it.  DZ0 carries y in this variant (y_rec).
// FROMY (FIRST, plain C = 32): aux = H1 is not read at all -- `fw` carries the first layer's three weight rows and the tile's sixteen
// aux values per lane are rebuilt from the y records the lane group already holds for dW_first (the same row_newbcast hand-over,
// first_layer_value: the bits fwd_c1_kernel would have stored), after the zero-tile early-out.
// DZMASK (plain C = 32, dense launches): the layer is the LAST one and DZ is the readout's gradient, which lives on the rows the
// readout reads -- `km` carries a bit per (plan block, slab) (scn_keep_mask, one hop out: scn_mask_hop) that is set wherever one of
// the block's SOURCE blocks holds such a row.  A visit whose bit
// is clear would stage and gather zeros only to find the zero-tile early-out: it stages nothing, waits for nothing, requests no aux,
// gathers nothing and writes the early-out's zero tile.  Every (block, slab) item is still visited and dx is still written in full:
// this is not the zero-skipping mode.  The decision depends on the trajectories' last nodes, never on a value.  The block's bits
// come as keep_window's 64-bit window (scn_blk_fwd.inc); with a NaN / Inf weight the plain path has no early-out (0 * Inf), so the
// window is all ones there and the kernel is the plain one.  A visit with its bit clear reads NEITHER staging buffer: they hold
// other slabs' data.
// VISIT (plain C = 32 and FIRST + FROMY, dense launches): the mirror of fwd_c32_w16_kernel<KEEP> -- only the (block, slab) items of a
// visit mask V are VISITED.  The workgroup's blocks with a visit and their 64-bit windows (cut to its slab range) come from one batched
// scan ahead of the block loop (scn_window_scan.inc), in unit order; a block with an empty window never enters the loop, and the slab
// loop runs over the window's set bits with its cursor in SGPRs (scn_keep_bits.h): no memory operation for the walk inside the slab loop.  A visit that runs is staged, gathered, contracted
// (or early-outed) and stored exactly as in the plain forms, in ascending slab order on the plain call's grid, so wherever every
// item outside V would have taken the zero-tile early-out the weight-gradient partials see the same tiles in the same order.  dx
// (plain form) is written on the visited items only; aux / y outside V and dz of items no visited item stages are not read.  V is
// `km` in both forms (the host builds it with keep_mask_of, as for the forward's KEEP forms).  A NaN / Inf weight
// does NOT widen the window (DZMASK does): V is visited regardless, see scn_conv_backward_visit in include/scone_hip.h.
// UNIT PIPELINE of the VISIT forms.  On a cone a unit has 1.3 visits on average, so the slab pipeline inside a unit (visit it + 1 is
// staged from the side slots of visit it's contraction) rarely has a second visit to work on, and every unit started with four
// dependent trips to memory and nothing beside them: header scalars, source rows + ELL tile, the wave's tile widths, the first slab's
// LDS-DMA (profiles/visit_prefetch_ab.txt: two thirds of the busiest workgroup's time).  The workgroup's scan table already names
// its next unit, so:
//   * the staging parity runs over the workgroup's WHOLE visit sequence (vpar), not per unit: a unit's last visit gathers from one
//     64 KB buffer and the other is free;
//   * a unit's prologue also fetches the NEXT unit's source rows, in the round trip of its own metadata, into a second 512-byte row
//     buffer behind the scan table (load_block_c32_ahead); the prologue's __syncthreads() publishes them;
//   * the unit's LAST visit stages the next unit's first slab from them through the very side slots (and the early-out's branch)
//     that stage "the next visit" otherwise: rows, chunk count and slab are the next unit's;
//   * the next unit's prologue then finds its rows in place and its slab on the way: it loads the ELL tile only, and the tile
//     widths ride with the header scalars.
// The ELL tile itself cannot be written ahead (one tile fits the LDS, and the current unit's waves gather through it up to the
// barrier at the next unit's top).  No arithmetic changes: the same tiles in the same order into the same accumulators.  A unit
// without a successor in the table (the last entry of a scan, the workgroup's last unit) stages nothing ahead, and the unit behind
// it runs the full prologue.  SCN_VISIT_PREFETCH=0 compiles the unit loop without any of this; a launch without
// VISIT_FLAG_PREFETCH in its `flags` argument takes that loop at run time.
#ifndef SCN_VISIT_PREFETCH
#define SCN_VISIT_PREFETCH 1
#endif
// PACKED RECORDS at the unit's top (VISIT_FLAG_RECORDS, on top of the unit pipeline).  The pipeline left a unit's top with two dependent
// trips: the header scalars (five arrays, a cold line each) and then the metadata they address; and the two tile-width bytes were
// loaded again behind the __syncthreads().  The window scan knows a unit's block one trip before the unit starts, so it also fetches
// the blocks' 32-byte records (scn_blk_record.h) into an LDS table behind the second source-row buffer (scn_window_scan.inc).  A unit's
// top then reads header, tile widths and the NEXT unit's source range as uniform LDS reads made scalar, and issues everything else
// (own rows unless staged, next rows, ELL tile, self slots) under one wait ahead of the __syncthreads() (load_block_c32_rec); nothing
// is loaded behind it.  The same blocks, rows and widths as from the separate arrays: no visit, order or arithmetic changes.  A launch
// without the flag (scn_conv_visit_records) takes the loop above as it was.
// (Touching the next unit's ELL lines ahead, from its record, during a unit's first visit was built and measured: it COST the two
// launches 4.7 and 1.3 us, profiles/visit_records_ab.txt section 2.)
constexpr int VISIT_FLAG_PREFETCH = 1, VISIT_FLAG_RECORDS = 2;
constexpr int VISIT_ROWS_BYTES = BK_SRC * 4;                  // the second source-row buffer: dynamic LDS of the VISIT launches, behind the scan table
static_assert((WSCAN_LDS_BYTES + VISIT_ROWS_BYTES) % 16 == 0, "the record table (WSCAN_HDR_BYTES behind the row buffer) starts 16-byte aligned");
static_assert(WSCAN_LDS_BYTES % 16 == 0, "the second source-row buffer starts 16-byte aligned");
enum : unsigned { BWD_EXT0 = 1, BWD_PAIR = 2, BWD_FIRST = 4, BWD_ACCUM = 8, BWD_FROMY = 16, BWD_DZMASK = 32, BWD_VISIT = 64 };
template <int ACT, unsigned FORM = 0>
__global__ __launch_bounds__(BK_THREADS, 2) void bwd_c32_bf16_kernel(PlanDev P, const float* __restrict__ DZ,
                                                                     const float* __restrict__ DZ0,
                                                                     const float* __restrict__ W0,
                                                                     const float* __restrict__ W1,
                                                                     const float* __restrict__ W2,
                                                                     const float* __restrict__ aux,
                                                                     float* __restrict__ dx, float* __restrict__ partial,
                                                                     int n_rows, int n_cols, int n_slabs, WorkList wl,
                                                                     float* __restrict__ partial_first, FirstW fw, KeepMask km,
                                                                     int flags, const BlockRec* __restrict__ recs) {
    constexpr bool EXT0 = (FORM & BWD_EXT0) != 0, PAIR = (FORM & BWD_PAIR) != 0, FIRST = (FORM & BWD_FIRST) != 0, ACCUM = (FORM & BWD_ACCUM) != 0,
                   FROMY = (FORM & BWD_FROMY) != 0, DZMASK = (FORM & BWD_DZMASK) != 0, VISIT = (FORM & BWD_VISIT) != 0;
    static_assert(!FROMY || (FIRST && !PAIR), "the aux-free form exists for the fused-first C = 32 kernel");
    static_assert(!DZMASK || (!EXT0 && !PAIR && !FIRST && !ACCUM && !FROMY), "the source mask exists for the plain C = 32 kernel");
    static_assert(!FIRST || !EXT0, "the fused first-layer gradient exists for the plain forms (C = 32, and C = 16 on slab pairs)");
    static_assert(!VISIT || (!EXT0 && !PAIR && !ACCUM && !DZMASK && FIRST == FROMY), "the visit mask exists for the plain and the fused-first from-y C = 32 kernel");
    static_assert(!ACCUM || (!EXT0 && !FIRST && !PAIR), "the accumulate form exists for the plain C = 32 kernel");
    // the one thing DZ0 is in this form (null in a form that has none of the three)
    const float* const dz_own = EXT0 ? DZ0 : nullptr;          // EXT0: the upstream gradient itself, segment 0 of G
    const float* const dx_partial = ACCUM ? DZ0 : nullptr;     // ACCUM: the input gradient's partial sum, of dx's shape
    const float* const y_rec = FIRST ? DZ0 : nullptr;          // FIRST: the first layer's shifted-input records
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PIECE = 512, CPP = 32, NDMA = BK_SRC * CPP / BK_THREADS;
    constexpr int CH = PAIR ? 16 : 32;                       // channels of a stored point
    const SmemC32 sm = carve_c32(smem);
    const uint32_t lds0 = lds_addr_of(smem);                  // LDS byte address of staging buffer 0
    char* wfrag = smem + smem_bytes_c32();
    constexpr bool accumulate = ACCUM;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p = lane & 31, h = lane >> 5, n = p & 3, rt = wave * 8 + (p >> 2);
    STAMP_DECL;
    STAMP_UNIT_DECL;
    STAMP_MARK(0);
    // dgrad B fragments: (g, t, lane) holds W_g[ca = lane&31][c = 16*(lane>>5) + 8t + j] * sW, j = 0..7 (one scale for the three
    // matrices: their products share the dgrad accumulator)
    char* isel = wfrag + B32_WFRAG_BYTES;
    float invW;
    static_assert(3 * 2 * 64 <= BK_THREADS, "one fragment per thread");
    float w[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (threadIdx.x < 3 * 2 * 64) {
        const int f = threadIdx.x, g = f / 128, t = (f >> 6) & 1, l = f & 63;
        const float* Wg = g == 0 ? W0 : (g == 1 ? W1 : W2);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ca = l & 31, cc = 16 * (l >> 5) + 8 * t + j;
            w[j] = !PAIR ? Wg[ca * 32 + cc] : ((ca >> 4) == (cc >> 4) ? Wg[(ca & 15) * 16 + (cc & 15)] : 0.f);
        }
    }
    bool w_bad;                                               // a weight is NaN / Inf: no zero-tile early-out (scn_blk_fwd.inc)
    const float sW = pow2_scale(block_abs_max<BK_THREADS>(amax3(amax3(amax3(amax3(0.f, w[0], w[1]), w[2], w[3]), w[4], w[5]), w[6], w[7]),
                                                          any_not_finite(w), (uint32_t*)(isel + 2048), w_bad), invW);
    if (threadIdx.x < 3 * 2 * 64) {
        const int f = threadIdx.x, g = f / 128, t = (f >> 6) & 1, l = f & 63;
        const Split2 sp = split2(w, sW);
        char* base = wfrag + ((g * 2 + t) * 2) * 1024 + l * 16;
        *(f16x8*)(base) = sp.hi;
        *(f16x8*)(base + 1024) = sp.lo;
    }
    // selection fragments: k-step t, B[k = 8h + j][n = p] = (p == 16h + 8t + j) as f16 1.0; kept in LDS behind the weight fragments
    // (two lane-linear B fragments; read back right where a transpose needs them)
    if (threadIdx.x < 128) {
        const int t = threadIdx.x >> 6, l = threadIdx.x & 63, pp = l & 31, hh = l >> 5;
        u32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c0 = 16 * hh + 8 * t + 2 * i;
            v[i] = (pp == c0 ? 0x3C00u : 0u) | (pp == c0 + 1 ? 0x3C000000u : 0u);
        }
        *(u32x4*)(isel + t * 1024 + l * 16) = v;
    }
    f32x16 dWacc[3];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) dWacc[g][r] = 0.f;
    float dwf[3] = {0.f, 0.f, 0.f};                           // FIRST: this lane's share of dW_first[g][c = p]
    float fwp[3] = {0.f, 0.f, 0.f};                           // FROMY: the first layer's weights of this lane's channel p
    if (FROMY) {
#pragma unroll
        for (int g = 0; g < 3; ++g) fwp[g] = fw.w[g][p];
    }
    int e_run = 1 << 20;                                      // running exponent of the dW accumulators (see the header): none yet
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    SCN_UNIT_RANGE();
    // RECORDS (the VISIT forms with the unit pipeline on; see the header): the walk's scans also fill the record table
    const bool rec_on = VISIT && SCN_VISIT_PREFETCH != 0 && !listed && (flags & (VISIT_FLAG_PREFETCH | VISIT_FLAG_RECORDS)) == (VISIT_FLAG_PREFETCH | VISIT_FLAG_RECORDS);
    SCN_WINDOW_WALK_RECS(VISIT, km, smem + smem_bytes_c32(B32_EXTRA_BYTES),
                         (UnitList{nullptr, nullptr}),   // (dW is summed in visit order: the backward keeps its static units)
                         VISIT && rec_on ? recs : nullptr, smem + smem_bytes_c32(B32_EXTRA_BYTES) + WSCAN_LDS_BYTES + VISIT_ROWS_BYTES);
    uint32_t cqs[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) cqs[q] = (uint32_t)((n * 8 + h * 4 + q) ^ (n >> 1)) << 4;
    const size_t slab_bytes = (size_t)n_cols * (PAIR ? 256 : PIECE);
    const bool second = PAIR && (((lane >> 2) ^ wave) & 1);       // this lane's LDS-DMA chunks come from slab B (see dma_k)
    // UNIT PIPELINE (the VISIT forms; see the header).  All of it is workgroup-uniform and lives across units and table scans.
    constexpr bool PIPE = VISIT && SCN_VISIT_PREFETCH != 0;
    const bool pipe_on = PIPE && !listed && (flags & VISIT_FLAG_PREFETCH) != 0;
    int32_t* const srcrows_b = (int32_t*)(smem + smem_bytes_c32(B32_EXTRA_BYTES) + WSCAN_LDS_BYTES);   // the second source-row buffer, behind the scan's table
    const int sr_b = (int)(srcrows_b - sm.srcrows);             // its distance from the first, in rows
    int vpar = 0;                                               // staging buffer of the unit's first visit: the workgroup's visits so far, mod 2
    int sr_cur = 0;                                             // 0 / sr_b: which buffer holds the current unit's source rows
    int pf_total = -1;                                          // >= 0: the previous unit staged this one's first slab (into buffer vpar) from
                                                                // this many chunks, and left its rows in buffer sr_cur
    if (listed || slab0 < slab1) {
    STAMP_MARK(1);
    STAMP_START();
    // VISIT: the units are the blocks of this workgroup that have a visit, with their windows cut to its slab range, from the batched
    // scan ahead of the loop (scn_window_scan.inc): a block without a visit never enters the loop -- no barrier, no metadata.  The
    // table is the same in all eight waves.  (dense launches only: k0 = slab0)
    SCN_UNIT_BEGIN_MASKED(VISIT)
        uint64_t vw = VISIT ? win_ : 0;                           // the cursor: its lowest set bit is the visit handled next
        STAMP_UADD(4);
        STAMP_UCOUNT(0);
        // PIPE: the table's next entry is the next unit (none: the last entry of a scan or of the workgroup -- the unit behind it
        // takes the prologue below in full); `staged` = the previous unit brought this one's rows and first slab
        const bool has_next = PIPE && pipe_on && u_ + 1 < u_end_;
        const int nb = has_next ? walk_.block(u_ + 1) : b;
        const int n_first = has_next ? keep_first(walk_.window(u_ + 1)) : 0;   // the next unit's first visit: slab k0 + n_first
        const bool staged = PIPE && pf_total >= 0;
        const int sr_next = PIPE ? sr_b - sr_cur : 0;
        int n_next = 0, tw_p = 0, twu_p = 0;
        wait_all_and_barrier();
        STAMP_UADD(0);
        BlockMeta m;
        if (VISIT && rec_on) {                                   // the header from the unit's record, the next unit's source range from ITS record
            uint32_t rw[8], nw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            walk_.record(u_, b, rw);
            if (has_next) walk_.record(u_ + 1, nb, nw);
            n_next = (int)(nw[3] & 255u);
            m = load_block_c32_rec<BK_THREADS>(P, b, rw, sm, sm.srcrows + sr_cur, staged, has_next, (int)nw[2], n_next, sm.srcrows + sr_next, wave, tw_p,
                                               twu_p);
        } else if (PIPE && pipe_on) {
            m = load_block_c32_ahead<BK_THREADS>(P, b, sm, sm.srcrows + sr_cur, staged, has_next, nb, sm.srcrows + sr_next, n_next, wave, tw_p, twu_p);
        } else {
            m = load_block_c32<BK_THREADS>(P, b, sm);
        }
        // DZMASK: bit v = the slab k0 + v of visit v has a source to stage in this block (all ones under a NaN / Inf weight)
        const uint64_t dzm = DZMASK ? (keep_window(km, b, k0) | (w_bad ? ~0ull : 0ull)) : ~0ull;
        __syncthreads();
        STAMP_UADD(1);
        const int tw = PIPE && pipe_on ? tw_p : P.tile_w[b * BK_WAVES + wave];
        const int twu = EXT0 ? 0 : (PIPE && pipe_on ? twu_p : P.tile_wu[b * BK_WAVES + wave]);
        const int rtc = rt < m.rows ? rt : m.rows - 1;
        const int total_next = n_next * CPP;
        // LDS-DMA instruction k of this wave moves chunks c = (k * 8 + wave) * 64 + lane: slot = 2 * (k * 8 + wave) + (lane >> 5),
        // position lane & 31.  The swizzled source chunk only depends on slot & 3 = ((wave & 1) << 1) | (lane >> 5), i.e. it is ONE
        // lane constant for every k, and the slot's source row comes from LDS at a lane constant + 64 * k: no per-k offsets in
        // registers.  PAIR: virtual chunk n*8 + q*4 + g <- slab q, chunk n*4 + g; q = bit 2 of d = ((lane>>2) ^ wave) & 1 for every k.
        const int total = m.nsrc * CPP;
        const int dq = swz32(((wave & 1) << 1) | (lane >> 5), lane & 31);
        const uint32_t dchunk = PAIR ? (uint32_t)(((dq >> 3) * 4 + (dq & 3)) * 16) : (uint32_t)(dq * 16);
        const int32_t* my_src = sm.srcrows + 2 * wave + (lane >> 5);          // + 16 * k
        // (PIPE: sr = the source-row buffer to stage from, sr_cur or sr_next, and tot = the chunks of THAT unit's block)
        auto dma_k = [&](int k, const char* Xs, int bufi, int sr = 0, int tot = -1) {
            const int base = (k * BK_WAVES + wave) * 64;
            if (base + lane < (PIPE ? tot : total)) {
                const uint32_t off = (uint32_t)my_src[16 * k + (PIPE ? sr : 0)] * (PAIR ? 256u : (uint32_t)PIECE) + dchunk;
                const uint32_t dst = lds0 + (uint32_t)(bufi * (BK_SRC * 512) + base * 16);
                if (PAIR) lds_dma16_v(Xs + off, dst);               // (the two lane groups stage from different slabs)
                else lds_dma16(Xs, off, dst);
            }
        };
        const int n_vis = VISIT ? keep_count(vw) : (PAIR ? (n_it + 1) >> 1 : n_it);   // visits: slabs, slab pairs, or the window's set bits
        auto slab_of = [&](int vis, int q) {                     // q-th slab of a visit (the lone last slab stands in for its pair)
            // plain form: wave-uniform -- saying so BEFORE the address arithmetic keeps the 64-bit multiplies on the scalar unit and the
            // LDS-DMA takes (SGPR base + 32-bit lane offset) instead of a 64-bit VGPR address
            // (DZMASK: dense launches only -- no vector load of a list entry, whose vmcnt(0) would drain the zero tiles at every visit)
            if (DZMASK) return k0 + vis;
            if (!PAIR) return __builtin_amdgcn_readfirstlane(SLAB_AT(vis));
            return SLAB_AT(2 * vis + q < n_it ? 2 * vis + q : 2 * vis);
        };
        auto src_base = [&](int vis) {
            return (const char*)DZ + (size_t)slab_of(vis, second ? 1 : 0) * slab_bytes;
        };
        auto src_of = [&](int slab) { return (const char*)DZ + (size_t)slab * slab_bytes; };   // VISIT: by slab, not by visit index
        if (PIPE ? !staged : (!DZMASK || (dzm & 1))) {          // (PIPE, staged: on its way since the previous unit's last visit)
            const char* Xs = VISIT ? src_of(k0 + keep_first(vw)) : src_base(0);
#pragma unroll
            for (int i = 0; i < NDMA; ++i) dma_k(i, Xs, PIPE ? vpar : 0, sr_cur, total);
        }
        const int rows_left = m.rows - wave * 8;
        f32x4 G[3][4];
        for (int it = 0; it < n_vis; ++it) {
            if (DZMASK) {
                // A RUN of visits whose bit is clear -- no source of the (block, slab) holds a row the readout wrote: each is the
                // zero-tile early-out below without the staging, the wait, the aux requests and the gather that lead to it.  Its own
                // loop, on scalars and what it makes itself (lane index, zeros, row count): a value carried through the live visits
                // is spilled there, and a reload is a vmcnt(0) wait -- stores count on vmcnt, so it would drain the zero tiles in
                // flight, as the wait at the top of a staged visit does.  The barrier stays on every visit (workgroup-uniform bits:
                // it is needed only where a buffer is published or about to be overwritten; kept until measured otherwise).
                // The wave's 8-row tile is 4 KB in a row: four 16-byte stores per lane, row 2 j + (lane >> 5).
                const int rows_left_s = __builtin_amdgcn_readfirstlane(rows_left);
                while (!((dzm >> it) & 1)) {
                    STAMP_START();
                    __builtin_amdgcn_s_barrier();
                    asm volatile("" ::: "memory");
                    if (it + 1 < n_vis && ((dzm >> ((it + 1) & 63)) & 1)) {      // the next visit is a staged one
                        const char* Xn0 = src_base(it + 1);
#pragma unroll
                        for (int i = 0; i < NDMA; ++i) dma_k(i, Xn0, (it + 1) & 1);
                    }
                    if (dx) {
                        float* dp0 = dx + (((size_t)slab_of(it, 0) * n_rows + m.row0 + wave * 8) * BK_NS) * CH;
                        int ln;
                        float z;
                        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0\n\tv_mov_b32 %1, 0" : "=&v"(ln), "=v"(z));
#ifdef SCN_AB_DZMASK_DWORD_STORES                                       // diagnostic builds: the early-out's sixteen dword stores per lane
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            if (2 * (r >> 2) + (ln >> 5) < rows_left_s) SCN_ST_STREAM(dp0 + (ln & 31) + 128 * (ln >> 5) + ((r & 3) + 8 * (r >> 2)) * 32, z);
#else
                        const f32x4 z4 = {z, z, z, z};
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (2 * j + (ln >> 5) < rows_left_s) SCN_ST_STREAM((f32x4*)(dp0 + (j * 64 + ln) * 4), z4);
#endif
                    }
                    STAMP_ADD(4);
                    if (++it == n_vis) break;
                }
                if (it == n_vis) break;
            }
            // VISIT: this visit's slab and the next one's (its own where it is the last) off the cursor; the visit INDEX still counts
            // 0, 1, 2, ...: buffer parity and the staging guards run on it as in the other forms
            int v_slab = 0, v_next = 0;
            if (VISIT) {
                v_slab = k0 + keep_first(vw);
                vw = keep_next(vw);
                v_next = vw ? k0 + keep_first(vw) : v_slab;
            }
            const int slab = VISIT ? v_slab : slab_of(it, PAIR ? p >> 4 : 0);   // PAIR: lanes p >= 16 hold slab B's channels
            const bool lane_live = !PAIR || p < 16 || 2 * it + 1 < n_it;
            const uint32_t bufbit = (uint32_t)(((PIPE ? it + vpar : it) & 1) << 16);
            const uint32_t cbs[4] = {cqs[0] | bufbit, cqs[1] | bufbit, cqs[2] | bufbit, cqs[3] | bufbit};
            // DZMASK (workgroup-uniform, scalar): the next visit's slab is to be staged (it + 1 < n_vis <= 64 where it is used)
            const bool dz_next = !DZMASK || ((dzm >> ((it + 1) & 63)) & 1);
            STAMP_VISIT_TOP(VISIT && it == 0);
            STAMP_UCOUNT(1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            STAMP_VISIT_WAITED(VISIT && it == 0);
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            STAMP_ADD(1);
            const size_t tuni = (((size_t)slab * n_rows + m.row0 + wave * 8) * BK_NS) * CH;
            const float* ap = aux + (rows_left > 0 ? tuni : 0);
            float* dp = dx && lane_live ? dx + tuni : nullptr;
            const int L0 = (PAIR ? p & 15 : p) + 4 * CH * h;
            // the tile's 16 aux values and the first weight fragments are requested before the gather so that their latency
            // (HBM / LDS) is covered by it; they are issued ahead of the next slab's LDS-DMA, so waiting for them later leaves
            // the DMA in flight
            float a[16];
            if (!FROMY) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool ok = 2 * (r >> 2) + h < rows_left && lane_live;
                    const float v = SCN_LD_STREAM(ap + (ok ? L0 + ((r & 3) + 8 * (r >> 2)) * CH : 0));
                    a[r] = ok ? v : 0.f;
                }
            }
            // ACCUM form (plain kernel): dx_partial is a tensor of dx's shape holding the input gradient's partial sum
            // over the output blocks before this one (hidden widths above 32, see fwd_c32_w16_kernel); it may be dx itself
            float dxp[16];
            if (accumulate) {
                const float* pp = dx_partial + (rows_left > 0 ? tuni : 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool ok = 2 * (r >> 2) + h < rows_left && lane_live;
                    const float v = SCN_LD_STREAM(pp + (ok ? L0 + ((r & 3) + 8 * (r >> 2)) * CH : 0));
                    dxp[r] = ok ? v : 0.f;
                }
            }
            // FIRST: the tile's y records, three floats per lane, placed for the row broadcast (see first_dw_step); PAIR: `slab` is
            // this lane group's slab
            float yv[3] = {0.f, 0.f, 0.f};
            if (FIRST) {
                const float* yt = y_rec + (((size_t)slab * n_rows + m.row0 + wave * 8) * BK_NS) * Y_STRIDE;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const int idx = 16 * q + (lane & 15), r = idx / 3, g = idx - 3 * r;
                    const int ypt = (r & 3) + 8 * (r >> 2) + 4 * h;
                    if ((ypt >> 2) < rows_left && lane_live) yv[q] = yt[ypt * Y_STRIDE + g];
                }
            }
            constexpr int GSEQ[3] = {1, 2, 0};                           // segment order
            f16x8 wn[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) wn[i] = *(const f16x8*)(wfrag + lane * 16 + ((GSEQ[0] * 2 + 0) * 2 + i) * 1024);
            __builtin_amdgcn_sched_barrier(0);
            // ---------------- GATHER: all three segments (the tile's scale needs the largest of them all)
            if (EXT0) {
                // (PAIR: the lane's sixteen virtual channels 16 h .. 16 h + 15 are slab h's sixteen)
                const float* g0 = dz_own + (((size_t)(PAIR ? slab_of(it, h) : slab) * n_rows + m.row0 + rtc) * BK_NS + n) * CH + (PAIR ? 0 : 16 * h);
#pragma unroll
                for (int q = 0; q < 4; ++q) G[0][q] = *(const f32x4*)(g0 + 4 * q);
                f32x4 unused[4];
                gather_c32<4, false>(sm, rtc, m.w, tw, 0, cbs, G[1], G[2], unused);
            } else {
                SCN_BWD_PRIO_GATHER();
                gather_c32<4, true, true>(sm, rtc, m.w, tw, twu, cbs, G[0], G[1], G[2]);
                SCN_BWD_PRIO_DGRAD();
            }
            STAMP_ADD(2);
            // ---------------- SCALES of the tile (wave-uniform; header of this file)
            float sG, inv_gw, sigma;
            {
                float mg = 0.f;
#pragma unroll
                for (int g = 0; g < 3; ++g) mg = amaxn_4x4(mg, G[g][0], G[g][1], G[g][2], G[g][3]);     // (NaN counts: scn_blk_fwd.inc)
                // PAIR: the wave's tile is two slabs -- lanes h = 0 gathered slab A's sixteen channels, lanes h = 1 slab B's, and the
                // block-diagonal weights keep their products apart (columns / lanes p < 16 and p >= 16 of every D tile) -- so each
                // slab gets the scales of its own data; everything below is then per lane group instead of per wave
                uint32_t mgb, mgb_b = 0;
                if (PAIR) {
                    max_over_halves(__float_as_uint(mg), mgb, mgb_b);
                } else {
                    mgb = max_over_wave(__float_as_uint(mg));
                }
                uint32_t mgb_a = mgb;
                if (PAIR) mgb = umax32(mgb, mgb_b);
                // ZERO-TILE EARLY-OUT (see fwd_c32_w16_kernel): every gathered gradient of the tile is exactly zero, so its input
                // gradient is zero (the accumulate form: the partial sum it was given) and it adds nothing to the weight gradients.
                // The gradient of the readout lives on the edges around the last nodes; k layers down it is supported on their k-hop
                // neighbourhood -- nearly every tile of a real batch leaves here.  Its share of the staging is still issued.
                if (!w_bad && mgb == 0) {
                    const int vdma0 = it + 1;
                    const bool nx0 = PIPE && has_next && vdma0 == n_vis;   // (PIPE: the next unit's first slab from a unit's last visit, see below)
                    if (nx0 || (vdma0 < n_vis && dz_next)) {
                        const char* Xn0 = VISIT ? src_of(nx0 ? k0 + n_first : v_next) : src_base(vdma0);
#pragma unroll
                        for (int i = 0; i < NDMA; ++i) dma_k(i, Xn0, (PIPE ? vdma0 + vpar : vdma0) & 1, nx0 ? sr_next : sr_cur, nx0 ? total_next : total);
                    }
                    if (!FIRST && dp) {
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            if (2 * (r >> 2) + h < rows_left) SCN_ST_STREAM(dp + L0 + ((r & 3) + 8 * (r >> 2)) * CH, accumulate ? dxp[r] : 0.f);
                    }
                    STAMP_ADD(4);
                    continue;
                }
                if (FROMY) {                                        // aux[pt(r, h)][p] from the tile's y records (value 3 r + g of the lane group's 48)
                    first_aux_tile<ACT>(std::make_integer_sequence<int, 16>{}, yv, fwp, a);
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (!(2 * (r >> 2) + h < rows_left && lane_live)) a[r] = 0.f;
                }
                if (umax32(mgb_a, mgb_b) > 0x7f800000u) {           // a NaN in the tile (rare): the scales from the NaN-ignoring maximum
                    asm volatile("; NaN tile: scales without it");
                    float mf = 0.f;
#pragma unroll
                    for (int g = 0; g < 3; ++g) mf = amax_4x4(mf, G[g][0], G[g][1], G[g][2], G[g][3]);
                    if (PAIR) {
                        max_over_halves(__float_as_uint(mf), mgb_a, mgb_b);
                    } else {
                        mgb_a = max_over_wave(__float_as_uint(mf));
                    }
                }
                float inv_g, inv_g_b = 0.f;
                sG = pow2_scale(mgb_a, inv_g);
                const int eG = pow2_scale_exp(mgb_a);
                int eG_b = eG, eA = 14, eA_b = 14;                       // tanh: |aux| <= 1
                float sG_b = sG;
                if (PAIR) {
                    sG_b = pow2_scale(mgb_b, inv_g_b);
                    eG_b = pow2_scale_exp(mgb_b);
                }
                if (ACT != SCN_ACT_TANH) {
                    float ma = 0.f;
#pragma unroll
                    for (int r = 0; r < 16; r += 2) ma = amax3(ma, a[r], a[r + 1]);
                    if (PAIR) {                                          // (aux is addressed per slab by p >> 4: the even / odd 16-lane rows)
                        uint32_t ea, eb;
                        max_over_even_odd_rows(__float_as_uint(ma), ea, eb);
                        eA = pow2_scale_exp(ea);
                        eA_b = pow2_scale_exp(eb);
                    } else {
                        eA = pow2_scale_exp(max_over_wave(__float_as_uint(ma)));
                    }
                }
                const int u_a = eG + eA, u_b = eG_b + eA_b;
                const int u_t = (PAIR && u_b < u_a) ? u_b : u_a;
                if (u_t < e_run) {                                       // this tile is the wave's largest so far: accumulators into its units
                    asm volatile("; dW accumulators into the units of a larger tile (rare)");   // (keeps this a branch: if-converted it is 24 v_pk_mul_f32 per visit)
                    const float f = exp2i(u_t - e_run);
#pragma unroll
                    for (int g = 0; g < 3; ++g)
#pragma unroll
                        for (int r = 0; r < 16; ++r) dWacc[g][r] *= f;
                    e_run = u_t;
                }
                sigma = exp2i(e_run - eG);
                inv_gw = inv_g * invW;
                if (PAIR) {                                              // per lane group: G by h, aux / dX by p >> 4
                    if (h) sG = sG_b;
                    if (p >= 16) {
                        sigma = exp2i(e_run - eG_b);
                        inv_gw = inv_g_b * invW;
                    }
                }
            }
            // ---------------- CONTRACT
            STAMP_UCOUNT(2);
            const int vdma = it + 1;                                     // the visit whose slab this contraction stages
            // PIPE: a unit's LAST visit stages the first slab of the NEXT unit instead -- its rows (buffer sr_next, published by this
            // unit's __syncthreads()), its chunk count, its slab -- into the buffer this visit does not gather from (the visit counter
            // runs on across units: vpar)
            const bool nx = PIPE && has_next && vdma == n_vis;
            const bool more = nx || (vdma < n_vis && dz_next);          // (DZMASK: a slab without a source in the mask is not staged)
            const char* Xn = VISIT ? src_of(nx ? k0 + n_first : v_next) : src_base(more ? vdma : it);
            const int nbuf = (PIPE ? vdma + vpar : vdma) & 1;
            auto side = [&](int k) {                                     // (all eight right after the barrier instead: +2 %)
                if (k < NDMA && more) dma_k(k, Xn, nbuf, nx ? sr_next : sr_cur, nx ? total_next : total);
            };
            // Per segment g: [transpose + dgrad] over its two k-steps, then straight into dW_g.  The transpose keeps the two
            // parts of the split in TWO accumulators (T_hi, T_lo = hi / lo of G_g sG, one channel per lane): each holds exactly
            // f16-representable values, so the B operand of the weight gradient is an exact conversion (one v_cvt_pk per two
            // values) instead of a second split of their sum.
            f32x16 acc;
            Split2 At[2];
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int g = GSEQ[u];
                SCN_BWD_PRIO_SEG(u);
                f32x16 Th, Tl;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    float x8[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) x8[j] = G[g][2 * t + (j >> 2)][j & 3];
                    const Split2 zs = split2(x8, sG);
                    const f16x8 wh = wn[0], wl = wn[1];
                    const f16x8 It = *(const f16x8*)(isel + t * 1024 + lane * 16);
                    const int k0 = (u * 2 + t) * 2;                          // two LDS-DMA side slots per group (8 used)
                    Tl = __builtin_amdgcn_mfma_f32_32x32x16_f16(zs.lo, It, t == 0 ? zero16 : Tl, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(zs.lo, wh, (u == 0 && t == 0) ? zero16 : acc, 0, 0, 0);     // small terms first
                    if (u * 2 + t < 5) {                                     // next group's fragments, one group ahead
                        const int un = (u * 2 + t + 1) >> 1, tn = (u * 2 + t + 1) & 1;
                        const char* wb = wfrag + ((GSEQ[un] * 2 + tn) * 2) * 1024 + lane * 16;
#pragma unroll
                        for (int i = 0; i < 2; ++i) wn[i] = *(const f16x8*)(wb + i * 1024);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    side(k0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(zs.hi, wl, acc, 0, 0, 0);
                    side(k0 + 1);
                    Th = __builtin_amdgcn_mfma_f32_32x32x16_f16(zs.hi, It, t == 0 ? zero16 : Th, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(zs.hi, wh, acc, 0, 0, 0);
                }
                if (u == 0) {                                         // dW A fragments from the aux tile (k-step t <-> points pt(8t + j, h))
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        float x8[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j) x8[j] = a[8 * t + j];
                        At[t] = split2(x8, sigma);
                    }
                }
                if (u == 2) {
                    SCN_BWD_PRIO_DW();
                    STAMP_ADD(3);
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] *= act_grad_from_output(ACT, a[r]) * inv_gw;   // dX = acc / (sG sW) * act'(aux)
                    if (accumulate) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[r] += dxp[r];
                    }
                    if (FIRST)                                           // dW_first[g][c = p] += y[pt(r, h)][g] * dx[pt(r, h)][p]
                        first_dw_tile(std::make_integer_sequence<int, 16>{}, yv, acc, dwf);
                }
                // dW_g += aux^T T_g
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    f16x8 bh, bl;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {                        // (exact: the parts are f16 values)
                        const auto ph = __builtin_amdgcn_cvt_pkrtz(Th[8 * t + 2 * i], Th[8 * t + 2 * i + 1]);
                        const auto pl = __builtin_amdgcn_cvt_pkrtz(Tl[8 * t + 2 * i], Tl[8 * t + 2 * i + 1]);
                        bh[2 * i] = (_Float16)ph[0]; bh[2 * i + 1] = (_Float16)ph[1];
                        bl[2 * i] = (_Float16)pl[0]; bl[2 * i + 1] = (_Float16)pl[1];
                    }
                    const Split2& at = At[t];
                    auto store = [&](int r) {                            // only in the last segment: acc is complete there
                        if (!FIRST && u == 2 && dp && 2 * (r >> 2) + h < rows_left) SCN_ST_STREAM(dp + L0 + ((r & 3) + 8 * (r >> 2)) * CH, acc[r]);
                    };
                    const int r0 = 8 * t;
                    dWacc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(at.lo, bh, dWacc[g], 0, 0, 0);
                    store(r0); store(r0 + 1);
                    dWacc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(at.hi, bl, dWacc[g], 0, 0, 0);
                    store(r0 + 2); store(r0 + 3); store(r0 + 4);
                    dWacc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(at.hi, bh, dWacc[g], 0, 0, 0);
                    store(r0 + 5); store(r0 + 6); store(r0 + 7);
                }
            }
            STAMP_ADD(4);
        }
        if (PIPE && pipe_on) {                                   // hand-over: the visit counter runs on; what the last visit staged
            vpar = (vpar + n_vis) & 1;
            sr_cur = has_next ? sr_next : sr_cur;
            pf_total = has_next ? total_next : -1;
        }
    }
    SCN_UNIT_END_MASKED(VISIT);
    }
    STAMP_MARK(2);
    if (!VISIT) { STAMP_FLUSH(); }                             // (the VISIT forms flush per workgroup at the exit: the global sums' atomics would be most of a masked launch)
    wait_all_and_barrier();
    float* red = (float*)sm.buf(0);
    // out of the wave's running units: x 2^-e_run, in two exact steps where one factor would leave the normal range (a wave without
    // a tile: e_run is still its initial value and the accumulators are zero)
    const int k_un = e_run >= (1 << 20) ? 0 : -e_run;
    const int k_1 = k_un < -126 ? -126 : (k_un > 127 ? 127 : k_un);
    const float un1 = exp2i(k_1), un2 = exp2i(k_un - k_1);
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ca = (r & 3) + 8 * (r >> 2) + 4 * h;
            red[wave * 3072 + ca * 96 + g * 32 + p] = dWacc[g][r] * un1 * un2;
        }
    __syncthreads();
    if (PAIR) {                                               // dW = the two diagonal blocks of the virtual 32x32 gradient
        float* outp = partial + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 768;
        for (int i = threadIdx.x; i < 768; i += BK_THREADS) {
            const int ca = i / 48, rem = i - ca * 48, g = rem >> 4, cc = rem & 15;
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < BK_WAVES; ++w)
                s += red[w * 3072 + ca * 96 + g * 32 + cc] + red[w * 3072 + (16 + ca) * 96 + g * 32 + 16 + cc];
            outp[i] = s;
        }
    } else {
        float* outp = partial + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 3072;
        for (int i = threadIdx.x; i < 3072; i += BK_THREADS) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < BK_WAVES; ++w) s += red[w * 3072 + i];
            outp[i] = s;
        }
    }
    if (FIRST) {                                               // dW_first partial of this workgroup: [g][c], fixed order over (wave, h)
                                                               // (PAIR: c = 16 s + channel, the two slabs are folded by the reduce kernel)
        __syncthreads();
#pragma unroll
        for (int g = 0; g < 3; ++g) red[(wave * 2 + h) * 96 + g * 32 + p] = dwf[g];
        __syncthreads();
        if (threadIdx.x < 96) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < 2 * BK_WAVES; ++w) s += red[w * 96 + threadIdx.x];
            partial_first[(size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 96 + threadIdx.x] = s;
        }
    }
    if (VISIT) { STAMP_FLUSH_WG(); }
}

// The forms of bwd_c32_bf16_kernel by name (one function-pointer type, so partial_first, fw, km, flags and recs are always passed).  The
// static_asserts inside the kernel say which combinations exist; what DZ, DZ0, aux, fw and km carry in each (null where not named):
template <int ACT> constexpr auto bwd_c32_plain = bwd_c32_bf16_kernel<ACT>;                                              // DZ = dz
template <int ACT> constexpr auto bwd_c32_pair = bwd_c32_bf16_kernel<ACT, BWD_PAIR>;                                     // the same at C = 16, on slab pairs
template <int ACT> constexpr auto bwd_c32_plain_dzmask = bwd_c32_bf16_kernel<ACT, BWD_DZMASK>;                           // DZ = dz, staged by km = the source mask
template <int ACT> constexpr auto bwd_c32_power = bwd_c32_bf16_kernel<ACT, BWD_EXT0>;                                    // DZ = g1 = S^T dz, DZ0 = dz
template <int ACT> constexpr auto bwd_c32_power_pair = bwd_c32_bf16_kernel<ACT, BWD_EXT0 | BWD_PAIR>;                    // the same at C = 16
template <int ACT> constexpr auto bwd_c32_accum = bwd_c32_bf16_kernel<ACT, BWD_ACCUM>;                                   // DZ0 = dx_partial, added to dx
template <int ACT> constexpr auto bwd_c32_first = bwd_c32_bf16_kernel<ACT, BWD_FIRST>;                                   // DZ0 = y, dx null: -> partial_first
template <int ACT> constexpr auto bwd_c32_first_pair = bwd_c32_bf16_kernel<ACT, BWD_FIRST | BWD_PAIR>;                   // the same at C = 16
template <int ACT> constexpr auto bwd_c32_first_from_y = bwd_c32_bf16_kernel<ACT, BWD_FIRST | BWD_FROMY>;                // and aux null: rebuilt from y and fw
template <int ACT> constexpr auto bwd_c32_plain_visit = bwd_c32_bf16_kernel<ACT, BWD_VISIT>;                             // DZ = dz, km = the visit mask, flags
template <int ACT> constexpr auto bwd_c32_first_from_y_visit = bwd_c32_bf16_kernel<ACT, BWD_FIRST | BWD_FROMY | BWD_VISIT>;   // DZ0 = y, aux null, km = the visit mask, flags
