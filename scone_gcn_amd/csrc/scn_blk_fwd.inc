// fused layer forward kernels (fp16 hi + lo split of both operands on the f16 MFMA) and the first-layer forward -- part of scn_blocked.hip (one translation unit; included inside namespace scn)
// ------------------------------------------------------------------------------------------------
// The dense contraction act(sum_g Z_g W_g) of a layer runs on the f16 MFMA with BOTH operands split in two (round 5):
//   x * s = hi + lo + r,   hi = f16(x s),  lo = f16(x s - hi),  |r| <= 2^-22 |x s|      (s = a power of two, see below)
//   z * w = hh + hl + lh (+ ll, dropped: <= 2^-22 |z w|), every f16 product exact in fp32, fp32 accumulation in the MFMA
// -- the same mantissa budget and the same three products as the 3xTF32 emulation of fp32 GEMMs.  fp16 has 5 exponent bits, so
// every operand ROW of a product (a point's gathered channels; a weight set) is first scaled by the power of two that puts its
// largest magnitude into [2^14, 2^15): multiplications by powers of two are exact, f16 subnormals are kept by the MFMA
// (tools/ubench/mfma_f16_split.hip), so an element 2^-k below its row's maximum is still held to 2^-40+ of that maximum -- the
// error of a dot product stays <= ~3 * 2^-22 * sum_k |z_k w_k|, i.e. the bound a plain fp32 fma chain has (measured on K = 32, worst
// case over 51 200 outputs, uniform / 7 decades of range inside every row / 1e-12 / 1e6 data: 0.9-5.5e-7 of sum|z w| against
// 0.9-4.5e-7 for the exact three-way bf16 split of rounds 1-4 and 1.9-5.0e-7 for the fp32 fma chain; profiles/r05_f16_split_accuracy.txt).
// Why: the bf16x3 split cost 5.5 VALU instructions per value and six MFMAs per product; this one costs 2 (one v_fma_mix per
// half, scaling included) and three -- the fused kernels were bound by exactly those two instruction streams (profiles/HISTORY.md section 3.2).
// ------------------------------------------------------------------------------------------------
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ uint32_t umax32(uint32_t a, uint32_t b) { return a > b ? a : b; }

// power-of-two scale of a row whose largest magnitude has the bit pattern `mbits` (a non-negative float): s = 2^(14 - floor(log2 m)),
// so that m s lies in [2^14, 2^15) -- inside f16's range, 1 bit of headroom; inv = 1 / s.  The exponent is clamped to [15, 254]: an
// all-zero (or subnormal) row gets the largest finite scale, Inf / NaN keep propagating.
__device__ __forceinline__ float pow2_scale(uint32_t mbits, float& inv) {
    uint32_t e = mbits & 0x7f800000u;
    e = e < (15u << 23) ? (15u << 23) : (e > (254u << 23) ? (254u << 23) : e);
    inv = __uint_as_float(e - (14u << 23));
    return __uint_as_float((268u << 23) - e);
}

// x[j] * s -> hi[j] + lo[j]: one v_fma_mixlo / mixhi_f16 per half (fp32 fma, one rounding to f16; the residual x s - hi is exact in
// fp32).  Inline assembly: left to itself hipcc's SLP pass turns the scalar form into v_pk_fma_f32 + conversions both ways (3
// instructions per value, and packed fp32 FMAs hold the matrix pipe).  The partial-register writes (mixhi) are kept at least one
// instruction away from their readers inside a statement and every statement ends in s_nop 0 (gfx940+ dst-select forwarding hazard,
// which the compiler cannot see through inline assembly).
__device__ __forceinline__ void split2(const float (&x)[8], float s, f16x8& hi, f16x8& lo) {
    u32x4 h, l;
    // two statements of eight instructions (the scheduler may place MFMAs between them: -1.5 % in the backward against one of sixteen)
#define SCN_SPLIT_HALF(A, B, X0, X1, X2, X3)                                                                                  \
    asm("v_fma_mixlo_f16 %0, %4, %8, 0\n\tv_fma_mixlo_f16 %1, %6, %8, 0\n\tv_fma_mixhi_f16 %0, %5, %8, 0\n\tv_fma_mixhi_f16 %1, %7, %8, 0\n\t"   \
        "v_fma_mixlo_f16 %2, %4, %8, -%0 op_sel_hi:[0,0,1]\n\tv_fma_mixlo_f16 %3, %6, %8, -%1 op_sel_hi:[0,0,1]\n\t"                        \
        "v_fma_mixhi_f16 %2, %5, %8, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\tv_fma_mixhi_f16 %3, %7, %8, -%1 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\ts_nop 0" \
        : "=&v"(h[A]), "=&v"(h[B]), "=&v"(l[A]), "=&v"(l[B]) : "v"(x[X0]), "v"(x[X1]), "v"(x[X2]), "v"(x[X3]), "v"(s))
    SCN_SPLIT_HALF(0, 1, 0, 1, 2, 3);
    SCN_SPLIT_HALF(2, 3, 4, 5, 6, 7);
#undef SCN_SPLIT_HALF
    hi = __builtin_bit_cast(f16x8, h);
    lo = __builtin_bit_cast(f16x8, l);
}
struct Split2 { f16x8 hi, lo; };
__device__ __forceinline__ Split2 split2(const float (&x)[8], float s) {
    Split2 r;
    split2(x, s, r.hi, r.lo);
    return r;
}

// maximum of a non-negative float's bit pattern over the four lanes l, l ^ 16, l ^ 32, l ^ 48 (the lanes that share a point in the
// 16-wave kernels: one point's 32 channels) -- v_permlane16_swap / v_permlane32_swap, VALU only
__device__ __forceinline__ uint32_t max_over_rows(uint32_t m) {
    const auto r = __builtin_amdgcn_permlane16_swap(m, m, false, false);
    m = umax32(r[0], r[1]);
    const auto q = __builtin_amdgcn_permlane32_swap(m, m, false, false);
    return umax32(q[0], q[1]);
}
// the same over all 64 lanes, as a wave-uniform value: six in-place v_max_u32 with a DPP source (a lane without a source keeps its
// value), lane 63 ends up with the wave's maximum.  Inline assembly: from __builtin_amdgcn_update_dpp the compiler makes copy + v_mov_dpp
// + v_max per step; the s_nop 1 are the two wait states a DPP read needs after a VALU write of the same register.
__device__ __forceinline__ uint32_t max_over_wave(uint32_t m) {
    asm("s_nop 1\n\t"
        "v_max_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
        "v_max_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
        "v_max_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
        "v_max_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"      // lane 15 of every row: the row's maximum
        "v_max_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1\n\t"  // into rows 1 and 3
        "v_max_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 1"       // into rows 2 and 3: lane 63 holds the wave's
        : "+v"(m));
    return (uint32_t)__builtin_amdgcn_readlane((int)m, 63);
}
// m = max(m, |a|, |b|) in ONE instruction (the abs modifiers are free).  Inline assembly: fmaxf(fabsf(a), fabsf(b)) compiles to a
// canonicalising v_max_f32 |a|, |a| per operand first (fmaxf's signalling-NaN rule) -- 1.75 instructions per value instead of 0.5.
// A NaN operand is ignored (the other operands win), which is what the scale wants: the NaN itself still reaches the product.
// (several instructions per asm statement: between two statements of a dependent chain the compiler puts an s_nop of its own)
// the same reduction stopped half way, for lane groups with scales of their own (the slab-pair forms):
//   lo / hi  = maximum over lanes 0..31 / 32..63;   even / odd = maximum over the 16-lane rows 0 and 2 / 1 and 3
__device__ __forceinline__ void max_over_halves(uint32_t m, uint32_t& lo, uint32_t& hi) {
    asm("s_nop 1\n\t"
        "v_max_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
        "v_max_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
        "v_max_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
        "v_max_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
        "v_max_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1"
        : "+v"(m));
    lo = (uint32_t)__builtin_amdgcn_readlane((int)m, 31);
    hi = (uint32_t)__builtin_amdgcn_readlane((int)m, 63);
}
__device__ __forceinline__ void max_over_even_odd_rows(uint32_t m, uint32_t& even, uint32_t& odd) {
    asm("s_nop 1\n\t"
        "v_max_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
        "v_max_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
        "v_max_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
        "v_max_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\ts_nop 1"
        : "+v"(m));
    even = umax32((uint32_t)__builtin_amdgcn_readlane((int)m, 15), (uint32_t)__builtin_amdgcn_readlane((int)m, 47));
    odd = umax32((uint32_t)__builtin_amdgcn_readlane((int)m, 31), (uint32_t)__builtin_amdgcn_readlane((int)m, 63));
}
__device__ __forceinline__ float amax3(float m, float a, float b) {
    asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(m) : "v"(a), "v"(b));
    return m;
}
__device__ __forceinline__ float amax_f4(float m, const f32x4 a) { return amax3(amax3(m, a[0], a[1]), a[2], a[3]); }
__device__ __forceinline__ float amax_2x4(float m, const f32x4 a, const f32x4 b) {
    asm("v_max3_f32 %0, %0, |%1|, |%2|\n\tv_max3_f32 %0, %0, |%3|, |%4|\n\tv_max3_f32 %0, %0, |%5|, |%6|\n\tv_max3_f32 %0, %0, |%7|, |%8|"
        : "+v"(m) : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]));
    return m;
}
__device__ __forceinline__ float amax_4x4(float m, const f32x4 a, const f32x4 b, const f32x4 c, const f32x4 d) {
    asm("v_max3_f32 %0, %0, |%1|, |%2|\n\tv_max3_f32 %0, %0, |%3|, |%4|\n\tv_max3_f32 %0, %0, |%5|, |%6|\n\tv_max3_f32 %0, %0, |%7|, |%8|\n\t"
        "v_max3_f32 %0, %0, |%9|, |%10|\n\tv_max3_f32 %0, %0, |%11|, |%12|\n\tv_max3_f32 %0, %0, |%13|, |%14|\n\tv_max3_f32 %0, %0, |%15|, |%16|"
        : "+v"(m) : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]),
                    "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]), "v"(d[0]), "v"(d[1]), "v"(d[2]), "v"(d[3]));
    return m;
}

// NON-FINITE DATA.  The amax helpers ignore a NaN (what the scales want), so a tile holding nothing but zeros and NaNs would have
// m == 0 and take a zero-tile early-out.  The early-outs therefore decide on the NaN-PROPAGATING maximum (v_maximum3_f32, same
// cost): a NaN counts as non-zero.  A NaN in a point's maximum leaves its per-point scale at the clamp, where all of the point's
// outputs are NaN anyway; the per-tile scales of the backward take the NaN-ignoring maximum again (rare branch).  A non-finite weight
// turns the early-outs off altogether (0 * NaN and 0 * Inf are NaN).
__device__ __forceinline__ float amaxn_2x4(float m, const f32x4 a, const f32x4 b) {
    asm("v_maximum3_f32 %0, %0, |%1|, |%2|\n\tv_maximum3_f32 %0, %0, |%3|, |%4|\n\tv_maximum3_f32 %0, %0, |%5|, |%6|\n\tv_maximum3_f32 %0, %0, |%7|, |%8|"
        : "+v"(m) : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]));
    return m;
}
__device__ __forceinline__ float amaxn_4x4(float m, const f32x4 a, const f32x4 b, const f32x4 c, const f32x4 d) {
    return amaxn_2x4(amaxn_2x4(m, a, b), c, d);
}
__device__ __forceinline__ float amaxn3(float m, float a, float b) {
    asm("v_maximum3_f32 %0, %0, |%1|, |%2|" : "+v"(m) : "v"(a), "v"(b));
    return m;
}
__device__ __forceinline__ bool not_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }
template <int N>
__device__ __forceinline__ bool any_not_finite(const float (&w)[N]) {
    bool r = false;
#pragma unroll
    for (int j = 0; j < N; ++j) r |= not_finite(w[j]);
    return r;
}

// largest of the threads' non-negative floats `m` as a bit pattern, known to every thread of the workgroup: `red` = one LDS word per
// wave.  Ends in a barrier.  (The kernels hand in the largest |weight| of the values a thread has just loaded for its fragment: the
// weights are read from memory once.)  `bad`: whether any thread handed in nonfinite = true (bit 31 of a wave's word: the maximum
// of finite or infinite magnitudes stays below it).
template <int NT>
__device__ __forceinline__ uint32_t block_abs_max(float m, bool nonfinite, uint32_t* red, bool& bad) {
    const uint32_t mw = max_over_wave(__float_as_uint(m)) | (__builtin_amdgcn_ballot_w64(nonfinite) != 0 ? 0x80000000u : 0u);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mw;
    __syncthreads();
    uint32_t r = 0, f = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        r = umax32(r, red[w] & 0x7fffffffu);
        f |= red[w];
    }
    bad = (f >> 31) != 0;
    return r;
}

// ------------------------------------------------------------------------------------------------
// forward, C_in = C_out = 32, SIXTEEN waves per workgroup (4 per SIMD, <= 128 VGPRs):
//   wave = 4 rows x 4 trajectories = 16 points, lane = (point = lane&15, channel octet kq = lane>>4),
//   v_mfma_f32_16x16x32_f16 on the hi + lo split (three products); the split weights live in LDS (12 KB, lane-linear A fragments);
//   the data is the B operand (column = point), so a point's power-of-two scale is common to the four lanes that hold its channels
//   and the un-scaling of the D tile is lane-local.
// The 8-wave kernels are latency-bound (every pipe < 40 % busy, tools/stamps.py); twice the resident waves at half the
// per-wave work is the cheapest way to hide the LDS round trips of the gather.
// ------------------------------------------------------------------------------------------------
constexpr int W16_THREADS = 1024, W16_WAVES = 16;
// block row of row k (0..3) of wave w's quad: 8 * (w >> 1) + QUAD_ROWS[w & 1][k]
__device__ __forceinline__ int quad_row(int wave, int k) {
    return 8 * (wave >> 1) + ((((wave & 1) ? 0x7421 : 0x6530) >> (4 * k)) & 7);
}
constexpr int W16_WFRAG_BYTES = 3 * 2 * 2 * 64 * 16;      // [segment][co tile][hi, lo][lane] x 8 f16
constexpr int W16_EXTRA_BYTES = W16_WFRAG_BYTES + 16 + 64;  // + the quads' widths + one word per wave (weights_abs_max)
// Wave priorities of the 16-wave forward (A/B switch SCN_FWD_PRIO, see profiles/HISTORY.md section 3.2 "who waits at the slab barrier"): the
// SIMD arbitrates its four waves by priority, then AGE, so with equal priorities the oldest wave of a SIMD runs through its visit
// first and idles at the slab barrier while the youngest finishes alone at half the issue rate.
//   SCN_FWD_PRIO_SEQ = 0xABCDEFGH: priorities of the phases of a visit, early waves: gather A, contraction segments B C D; late
//   waves: contraction segments E F G, gather H (0x32103321: priority = remaining work of the visit, whoever is behind goes first)
//   SCN_FWD_PRIO = 2: static, youngest highest (wave >> 2);  3: static, the late half of the stagger at 1
#ifndef SCN_FWD_PRIO
#define SCN_FWD_PRIO 0
#endif
#if !defined(SCN_FWD_PRIO_SEQ) && SCN_FWD_PRIO == 0
#define SCN_FWD_PRIO_SEQ 0x32103321     // default since round 4: -2.2 % dense, -1.9 % on mostly-zero slabs (profiles/r04_sync_ab.txt); -DSCN_FWD_PRIO_SEQ=0 = none
#endif
#if SCN_FWD_PRIO_SEQ != 0
template <int I> __device__ __forceinline__ void fwd_prio() { __builtin_amdgcn_s_setprio((SCN_FWD_PRIO_SEQ >> (4 * (7 - I))) & 3); }
#define SCN_FWD_PRIO_GATHER() do { if (late) fwd_prio<7>(); else fwd_prio<0>(); } while (0)
#define SCN_FWD_PRIO_CONTRACT(g) do { if (late) { if ((g) == 0) fwd_prio<4>(); if ((g) == 1) fwd_prio<5>(); if ((g) == 2) fwd_prio<6>(); } \
                                       else { if ((g) == 0) fwd_prio<1>(); if ((g) == 1) fwd_prio<2>(); if ((g) == 2) fwd_prio<3>(); } } while (0)
#else
#define SCN_FWD_PRIO_GATHER()
#define SCN_FWD_PRIO_CONTRACT(g)
#endif

// EXT0: the operator has ONE value array and the layer is  act(X0 W0 + X W1 + (S X) W2)  -- segment 0 comes from a second
// tensor X0 (the lane's own rows, straight from HBM), segment 1 is the staged tensor's own row, segment 2 its gathered shift
// (Ebli on large complexes: X0 = H, X = S H, so the third term is S^2 H without ever forming S^2).
// ACCUM (plain form only): X0 is a tensor of the output's shape holding partial pre-activations and the
// result is act(X0 + the three terms) (X0 may be `out` itself: a lane reads exactly the 32 bytes it writes).  Hidden widths above 32
// run a layer as (input block, output block) pairs of 32 channels; this adds the pairs up without a pass of their own.
// FROMY (plain form only): the layer's input is the FIRST layer's output H1, which is never stored -- X carries the first layer's
// shifted-input records y[slab][row][trajectory] = (x, S_lo x, S_up x, 0) (16 bytes per point instead of 128) and `fw` the first
// layer's three weight rows.  Per slab the block's source rows' records are fetched with ordinary 16-byte loads and EXPANDED
// into the same swizzled LDS image the LDS-DMA builds from a stored H1 (first_layer_value: the bits fwd_c1_kernel would have
// written), so the gather, the split, the MFMA chain, the early-out and the stores are the plain form's.  Thread = (channel quad
// tid & 7, trajectory (tid >> 3) & 3, slots (tid >> 5) + 32 i, i = 0..3): four records and four ds_write_b128 per slab, 32
// consecutive lanes write one whole 512-byte piece.  The records of slab v + 1 are requested at the start of interval v and
// expanded between the wave's two phases; the slab barrier waits for the LDS writes (lgkmcnt) instead of the LDS-DMA (vmcnt).
constexpr int W16_FIRSTW_BYTES = 3 * 32 * 4;              // FROMY: the first layer's weights [g][32], behind the plain form's extra bytes
// KEEP (plain and from-y forms, dense launches): the layer is the LAST one and only the readout reads its output -- `km` holds a bit
// per (plan block, slab) (scn_keep_mask) and only the items whose bit is set are VISITED: a block's slab loop runs over the set
// bits of its window (visit i = the slab of the i-th set bit), a block without one never enters the block loop: the workgroup's blocks
// with a kept slab and their windows come from one batched scan ahead of the loop (scn_window_scan.inc), in unit order.  An item
// whose bit is clear is not staged, gathered or contracted, and no byte of its rows is written; a visit that runs is staged,
// gathered, contracted (or early-outed) and stored exactly as in the other forms, so a kept row holds the plain forward's bits.
// The decision depends on the trajectories' last nodes, never on a value.  (The slab-pair kernel fwd_c16_w16_kernel<KEEP> still
// visits every pair and only drops the store.)
// keep_window (the slab-pair form and the backward's DZMASK; the visiting forms take their windows from the scan, which follows the
// same rule): the bits of block b for the KEEP_WINDOW slabs from `first` on (bit j = slab first + j), fetched ONCE per block,
// ahead of the block's metadata, made wave-uniform and claimed there: nothing of it is in flight when the slab loop starts (a
// scalar load in flight there turns the gather's counted lgkmcnt waits into lgkmcnt(0), a vector load is followed by vmcnt(0), a
// wait for the LDS-DMA just issued: profiles/HISTORY.md section 3.2); the slab loop walks it in SGPRs (scn_keep_bits.h).  The host
// hands a workgroup at most KEEP_WINDOW slabs.
constexpr int KEEP_WINDOW = 64;
// FORM: the form of the 16-wave forwards, an OR of these bits (fwd_c16_w16_kernel: FWD_EXT0 and FWD_KEEP); the kernels' first lines
// name them and assert which combinations exist.
enum : unsigned { FWD_EXT0 = 1, FWD_ACCUM = 2, FWD_FROMY = 4, FWD_KEEP = 8 };
__device__ __forceinline__ uint64_t keep_window(const KeepMask km, int b, int first) {
    const uint64_t win = keep_window_lane(km, b, first);      // (scn_window_scan.inc: three loads, no branch; the one copy of the rule)
    uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)win), hi = __builtin_amdgcn_readfirstlane((uint32_t)(win >> 32));   // wave-uniform
    asm volatile("" : "+s"(lo), "+s"(hi));                    // the loads are waited for HERE
    return ((uint64_t)hi << 32) | lo;
}
template <int ACT, unsigned FORM = 0>
__global__ __launch_bounds__(W16_THREADS, 4) void fwd_c32_w16_kernel(PlanDev P, const float* __restrict__ X,
                                                                     const float* __restrict__ X0,
                                                                     const float* __restrict__ W0,
                                                                     const float* __restrict__ W1,
                                                                     const float* __restrict__ W2,
                                                                     float* __restrict__ out, int n_rows, int n_cols,
                                                                     int n_slabs, WorkList wl, FirstW fw, KeepMask km, UnitList ul) {
    constexpr bool EXT0 = (FORM & FWD_EXT0) != 0, ACCUM = (FORM & FWD_ACCUM) != 0, FROMY = (FORM & FWD_FROMY) != 0, KEEP = (FORM & FWD_KEEP) != 0;
    static_assert(!FROMY || (!EXT0 && !ACCUM), "the from-y form exists for the plain kernel");
    static_assert(!KEEP || (!EXT0 && !ACCUM), "the keep mask exists for the plain and the from-y kernel");
    static_assert(!(EXT0 && ACCUM), "the accumulate form exists for the plain kernel");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PIECE = 512, CPP = 32, NDMA = BK_SRC * CPP / W16_THREADS;   // 4 LDS-DMA instructions per wave
    const SmemC32 sm = carve_c32(smem);
    const uint32_t lds0 = lds_addr_of(smem);                  // LDS byte address of staging buffer 0
    char* wfrag = smem + smem_bytes_c32();
    uint8_t* tws = (uint8_t*)(wfrag + W16_WFRAG_BYTES);
    uint32_t* wred = (uint32_t*)(tws + 16);
    float* fwl = (float*)(smem + smem_bytes_c32(W16_EXTRA_BYTES));   // FROMY only (the launch adds W16_FIRSTW_BYTES)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the wave's four rows are a QUAD of its 8-row group (rows {0,3,5,6} / {1,2,4,7}: the row sets the backward's lane groups
    // hold) and the point index is trajectory-major, so that every ds_read_b128 lane group holds the quad's four rows with all
    // four trajectories: conflict-free whenever the four sources differ in slot & 3 (scn_blk_layout.inc arranges that)
    const int pt = lane & 15, kq = lane >> 4, n = pt >> 2, rt = quad_row(wave, pt & 3);
    STAMP_DECL;
    // split the weights once, under ONE power-of-two scale for the three matrices (their products share an accumulator):
    // fragment (g, ct, part, lane) = W_g[8*kq' + j][16*ct + i] * sW, i = lane&15, kq' = lane>>4
    float invW;
    static_assert(3 * 2 * 64 <= W16_THREADS, "one fragment per thread");
    float w[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (tid < 3 * 2 * 64) {
        const int g = tid / 128, ct = (tid >> 6) & 1, l = tid & 63;
        const float* Wg = g == 0 ? W0 : (g == 1 ? W1 : W2);
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = Wg[(8 * (l >> 4) + j) * 32 + 16 * ct + (l & 15)];
    }
    bool w_bad;                                               // a weight is NaN / Inf: no zero-tile early-out (above block_abs_max)
    bool fw_bad = false;                                      // FROMY: the first layer's weights count too (0 * Inf: no zero-record short cut)
    if (FROMY && tid < 96) {
        const float v = fw.w[tid >> 5][tid & 31];
        fwl[tid] = v;                                         // (visible after block_abs_max's barrier)
        fw_bad = not_finite(v);
    }
    const float sW = pow2_scale(block_abs_max<W16_THREADS>(amax3(amax3(amax3(amax3(0.f, w[0], w[1]), w[2], w[3]), w[4], w[5]), w[6], w[7]),
                                                           any_not_finite(w) || fw_bad, wred, w_bad), invW);
    if (tid < 3 * 2 * 64) {
        const int f = tid;
        const int g = f / 128, ct = (f >> 6) & 1, l = f & 63;
        const Split2 sp = split2(w, sW);
        char* base = wfrag + ((g * 2 + ct) * 2) * 1024 + l * 16;
        *(f16x8*)(base) = sp.hi;
        *(f16x8*)(base + 1024) = sp.lo;
    }
    SCN_UNIT_RANGE();
    if (!listed && slab0 >= slab1) return;
    SCN_WINDOW_WALK(KEEP, km, smem + smem_bytes_c32(W16_EXTRA_BYTES + (FROMY ? W16_FIRSTW_BYTES : 0)), ul);
#if SCN_FWD_PRIO == 2
    if (wave >= 12) __builtin_amdgcn_s_setprio(3); else if (wave >= 8) __builtin_amdgcn_s_setprio(2); else if (wave >= 4) __builtin_amdgcn_s_setprio(1);
#elif SCN_FWD_PRIO == 3
    if (wave >= 8) __builtin_amdgcn_s_setprio(1);
#endif
    f32x4 pend[2];
    float* pend_ptr = nullptr;
    bool pend_valid = false;
    // chunk index of this lane's two 16-byte chunks inside a piece: n*8 + kq*2 + q, swizzled like the 8-wave kernels
    uint32_t cqs[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) cqs[q] = (uint32_t)((n * 8 + kq * 2 + q) ^ (n >> 1)) << 4;
    const size_t slab_bytes = (size_t)n_cols * PIECE;
    const int lane_out = (rt * BK_NS + n) * 32 + 4 * kq;      // this lane's first output float inside the block's rows of a slab
    // The whole block loop exists TWICE, for the early and the late half of the waves (see STAGGER below): with `late` a
    // compile-time constant each half is one straight-line path, and the values that live across the phases (the gathered z, the
    // pending tile) keep their registers -- as one path the compiler paid ~20 register moves per visit to reconcile the two roles.
    auto run = [&](auto late_c) {
    constexpr int late = decltype(late_c)::value;
    // KEEP: the units are the blocks of this workgroup that have a kept slab, with their windows cut to its slab range (the bits
    // above n_it are other workgroups' slabs), from the batched scan ahead of the loop (scn_window_scan.inc): a block without a kept
    // slab never enters the loop -- its metadata is not touched, no barrier, no LDS write; a tile pending from an earlier block
    // stays pending.  The table is the same in all sixteen waves.  (dense launches only: k0 = slab0)
    SCN_UNIT_BEGIN_MASKED(KEEP)
        const uint64_t keep = win_;
        const int n_vis = KEEP ? keep_count(keep) : n_it;             // visits of this block: visit i = the slab of the i-th set bit
        wait_all_and_barrier();
        BlockMeta m;
        {
            m.row0 = P.blk_row0[b];
            m.rows = P.blk_rows[b];
            const int sp0 = P.src_ptr[b];
            m.nsrc = P.src_ptr[b + 1] - sp0;
            m.w = P.width[b];
            const int ep = P.ell_ptr[b];
            for (int i = tid; i < m.nsrc; i += W16_THREADS) sm.srcrows[i] = P.src_rows[sp0 + i];
            for (int i = tid; i < m.w * m.rows; i += W16_THREADS) {
                sm.enc[i] = P.ell_enc[ep + i];
                sm.v[i] = P.ell_v[ep + i];
            }
            if (tid < BK_R) sm.self[tid] = P.self_slot[(size_t)b * BK_R + tid];
            if (tid < W16_WAVES) tws[tid] = P.tile_w4[b * W16_WAVES + tid];
        }
        __syncthreads();
        const int tw = tws[wave];                    // width of this wave's own quad
        const int twu = EXT0 ? 0 : P.tile_wu4[b * W16_WAVES + wave];
        const int rtc = rt < m.rows ? rt : m.rows - 1;
        // LDS-DMA instruction k of this wave moves chunks c = (k * 16 + wave) * 64 + lane: slot = 2 * (k * 16 + wave) + (lane >> 5),
        // position lane & 31; the swizzled source chunk depends on slot & 3 = ((wave & 1) << 1) | (lane >> 5) only: ONE lane
        // constant for every k, the slot's source row comes from LDS at a lane constant + 128 * k bytes
        const int total = m.nsrc * CPP;
        const uint32_t dchunk = (uint32_t)swz32(((wave & 1) << 1) | (lane >> 5), lane & 31) * 16;
        const int32_t* my_src = sm.srcrows + 2 * wave + (lane >> 5);          // + 32 * k
        auto dma = [&](int k, const char* Xs, int bufi) {
            if (FROMY) return;                                     // staged by y_load / y_expand below
#if defined(SCN_FWD_FLOOR) && SCN_FWD_FLOOR == 2                 // diagnostic build (results wrong by design): no staging, gather + contraction + stores only
            return;
#endif
            const int base = (k * W16_WAVES + wave) * 64;
            if (base + lane < total) lds_dma16(Xs, (uint32_t)my_src[32 * k] * PIECE + dchunk, lds0 + (uint32_t)(bufi * (BK_SRC * 512) + base * 16));
        };
        // slab indices are wave-uniform; saying so BEFORE the address arithmetic keeps the 64-bit multiplies on the scalar unit (the
        // listed form loads them with a vector load: left to itself the compiler does slab * slab_bytes in quarter-rate v_mul_*_u32)
        auto slab_at = [&](int it) { return SLAB_AT_U(it); };
        // KEEP: the visits are the set bits of `keep`, consumed in ascending order.  Each consumer holds a CURSOR, a copy of the
        // window whose lowest set bit is the visit it handles next (keep_first), and drops that bit when done (keep_next): two
        // SGPRs and a few scalar instructions per visit, no table and no memory operation inside the slab loop (see keep_window).
        // slab_of(w, it): the slab of visit `it`, `w` being a cursor that stands at it.  The visit INDEX still counts 0, 1, 2, ...:
        // buffer parity, the stagger and the vdma guards run on it as in the other forms.
        auto slab_of = [&](uint64_t w, int it) { return KEEP ? k0 + keep_first(w) : slab_at(it); };
        uint64_t cw = keep;                                           // the contraction's cursor
        uint64_t yw = keep_next(keep);                                // FROMY: the record loads' cursor, one visit ahead
        auto slab_base = [&](int slab) { return (const char*)X + (size_t)slab * slab_bytes; };   // SGPR base + 32-bit lane offset in the LDS-DMA
        // FROMY staging: this thread's four records of a slab (slots ys_slot + 32 i, trajectory ys_n), then their channel quad ys_cq
        // of H1 into the image: piece chunk ys_n * 8 + ys_cq of slot s lives at s * 512 + swz32(s, chunk) * 16 (what the LDS-DMA builds)
        const int ys_cq = tid & 7, ys_n = (tid >> 3) & 3, ys_slot = tid >> 5;
        typedef float f32x3 __attribute__((ext_vector_type(3)));   // (the record's fourth float is padding: 12 registers, not 16)
        f32x3 yr[NDMA];
        auto y_load = [&](int slab) {
            const char* Ys = (const char*)X + (size_t)slab * n_cols * (BK_NS * Y_STRIDE * 4);
#pragma unroll
            for (int i = 0; i < NDMA; ++i) {
                const int s = ys_slot + 32 * i;
                if (s < m.nsrc) yr[i] = *(const f32x3*)(Ys + ((size_t)(uint32_t)sm.srcrows[s] * BK_NS + ys_n) * (Y_STRIDE * 4));
            }
        };
        auto y_expand = [&](int bufi) {
            const f32x4 f0 = *(const f32x4*)(fwl + 4 * ys_cq), f1 = *(const f32x4*)(fwl + 32 + 4 * ys_cq),
                        f2 = *(const f32x4*)(fwl + 64 + 4 * ys_cq);
#pragma unroll
            for (int i = 0; i < NDMA; ++i) {
                const int s = ys_slot + 32 * i;
                const bool live = s < m.nsrc;                       // (s is uniform over 32 lanes: half-wave granular)
                const uint32_t bits = live ? (__float_as_uint(yr[i][0]) | __float_as_uint(yr[i][1]) | __float_as_uint(yr[i][2])) : 0u;
                // records that are all zero BITS expand to zeros without the FMAs and the activation (decided per wave; -0, NaN and Inf
                // are not zero bits, and a non-finite first-layer weight turns the short cut off: 0 * Inf is NaN)
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (w_bad || __builtin_amdgcn_ballot_w64(bits != 0u) != 0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = first_layer_value(ACT, yr[i][0], yr[i][1], yr[i][2], f0[j], f1[j], f2[j]);
                }
                if (live) *(f32x4*)(sm.buf(bufi) + s * PIECE + swz32(s, ys_n * 8 + ys_cq) * 16) = v;
            }
        };
        if (FROMY) {
            y_load(slab_of(keep, 0));
            y_expand(0);
        } else {
            const char* Xs = slab_base(slab_of(keep, 0));
#pragma unroll
            for (int i = 0; i < NDMA; ++i) dma(i, Xs, 0);
        }
        // STAGGER.  A slab visit has two phases per wave: GATHER (LDS reads + FMAs -- with all sixteen waves in it at once the
        // LDS pipe is the limit) and CONTRACT (split + MFMA + activation: matrix pipe and VALU).  Waves 8-15 run half a visit
        // behind waves 0-7 (every SIMD hosts two of each): while one half gathers slab v the other contracts slab v - 1, between
        // the same two slab barriers.  A late wave carries its gathered z across the barrier; its share of the next LDS-DMA is one
        // visit further ahead (slab v + 2), the early waves' as before (slab v + 1).
        if (!FROMY && late && n_vis > 1) {             // the late waves' share of visit 1 has no contraction to ride in
            const char* Xs = slab_base(slab_of(keep_next(keep), 1));
#pragma unroll
            for (int i = 0; i < NDMA; ++i) dma(i, Xs, 1);
        }
        f32x4 z[3][2];                                 // [segment][chunk q]: channels 8*kq + 4*q .. +3 of this lane's point
        f32x4 addv[2];                                 // accumulate form: the partial pre-activations of this lane's eight outputs
        constexpr bool accumulate = ACCUM;
        auto tile_of = [&](int slab) { return ((size_t)slab * n_rows + m.row0) * (BK_NS * 32); };   // (scalar) first float of the block's rows in a slab
        // ---------------- GATHER of slab `it` (staged in buffer it & 1) into z
        auto gather_phase = [&](int it) {
#if defined(SCN_FWD_FLOOR) && SCN_FWD_FLOOR == 1                 // diagnostic build (results wrong by design): staging + barriers + stores only
            return;
#endif
            // hipcc counts an LDS-DMA as a possible LGKM operation that returns out of order, and while one may be pending every
            // LDS wait becomes lgkmcnt(0) (see lds_dma16); a compiler-visible lgkmcnt(0) here -- nothing of this wave's is in the
            // LDS queue at this point -- keeps the gather's waits counted whatever the staging is written with
            __builtin_amdgcn_s_waitcnt(0xC07F);
            const uint32_t cb[2] = {cqs[0] | (uint32_t)((it & 1) << 16), cqs[1] | (uint32_t)((it & 1) << 16)};
            if (EXT0) {
                const float* x0 = X0 + tile_of(slab_at(it)) + ((rtc * BK_NS + n) * 32 + 8 * kq);
                z[0][0] = *(const f32x4*)(x0);           // requested before the gather: its latency hides under it
                z[0][1] = *(const f32x4*)(x0 + 4);
                f32x4 unused[2];
                gather_c32<2, false>(sm, rtc, m.w, tw, 0, cb, z[1], z[2], unused);
            } else {
                if (accumulate) {                          // requested before the gather, like the EXT0 operand
                    const float* pa = X0 + tile_of(slab_at(it)) + ((rtc * BK_NS + n) * 32 + 4 * kq);
                    addv[0] = *(const f32x4*)(pa);
                    addv[1] = *(const f32x4*)(pa + 16);
                }
                gather_c32<2>(sm, rtc, m.w, tw, twu, cb, z[0], z[1], z[2]);
            }
            STAMP_ADD(2);
        };
        // ---------------- CONTRACT of slab `it` from z: out^T tile (16 channels x 16 points) x 2 channel tiles; the LDS-DMA of the
        // slab this wave stages next and the previous tile's two 16-byte stores ride inside the chains
        auto contract_phase = [&](int it) {
            const int slab = slab_of(cw, it);
            const size_t tile0 = tile_of(slab);
            const int vdma = it + 1 + late;
            const bool more = vdma < n_vis;
            const uint64_t cw1 = keep_next(cw), cwd = late ? keep_next(cw1) : cw1;   // KEEP: the cursor at visit it + 1 and at visit vdma
            const char* Xn = slab_base(more ? slab_of(cwd, vdma) : slab);
            if (KEEP) cw = cw1;
            const int nbuf = vdma & 1;
#if defined(SCN_FWD_FLOOR) && SCN_FWD_FLOOR == 1
            if (more) {
#pragma unroll
                for (int k = 0; k < NDMA; ++k) dma(k, Xn, nbuf);
            }
            if (rt < m.rows) {
                float* op = out + tile0 + lane_out;
                *(f32x4*)(op) = f32x4{0.f, 0.f, 0.f, 0.f};
                *(f32x4*)(op + 16) = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            return;
#endif
            {
                const f32x4 prev0 = pend[0], prev1 = pend[1];
                float* const prev_ptr = pend_ptr;
                const bool prev_valid = pend_valid && pend_ptr != nullptr;
                f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
                // (claimed HERE: a vector-memory wait is in issue order, so the compiler's wait for these two loads must come before
                // this visit's LDS-DMA instructions, which it cannot see, are issued)
                if (accumulate) asm volatile("" : "+v"(addv[0]), "+v"(addv[1]));
                // the point's scale: largest magnitude among its 96 gathered values (this lane's 24 and its three partner lanes')
                float inv;
                float sz;
                const float m = amaxn_2x4(amaxn_4x4(0.f, z[0][0], z[0][1], z[1][0], z[1][1]), z[2][0], z[2][1]);   // (NaN counts)
                // ZERO-TILE EARLY-OUT.  No layer of this path has a bias and act(0) = 0, so a tile whose gathered values are all exactly
                // zero has the output act(partial) -- exactly what the contraction would produce; its split, MFMAs and un-scaling are
                // skipped (wave-uniform branch), its share of the staging and its pending stores are not.  A trajectory's activations
                // are supported on the k-hop neighbourhood of its edges after k layers, so most tiles of a real batch are of this kind;
                // `roofline.dense_random_*` in the bench line is measured on tensors without zeros.
                const bool tile_zero = !w_bad && __builtin_amdgcn_ballot_w64(m != 0.f) == 0;
                if (tile_zero) {
#pragma unroll
                    for (int k = 0; k < NDMA; ++k)
                        if (more) dma(k, Xn, nbuf);
                    if (prev_valid) {
                        *(f32x4*)(prev_ptr) = prev0;
                        *(f32x4*)(prev_ptr + 16) = prev1;
                    }
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                        for (int r = 0; r < 4; ++r) pend[ct][r] = accumulate ? act_apply_fast(ACT, addv[ct][r]) : 0.f;
                } else {
                {
                    sz = pow2_scale(max_over_rows(__float_as_uint(m)), inv);
                    inv *= invW;
                }
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    SCN_FWD_PRIO_CONTRACT(g);
                    float x8[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) x8[j] = z[g][j >> 2][j & 3];
                    const Split2 zs = split2(x8, sz);
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) {
                        const char* wb = wfrag + ((g * 2 + ct) * 2) * 1024 + lane * 16;
                        const f16x8 wh = *(const f16x8*)(wb), wl = *(const f16x8*)(wb + 1024);
                        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, zs.hi, acc[ct], 0, 0, 0);      // small terms first
                        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, zs.lo, acc[ct], 0, 0, 0);
                        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, zs.hi, acc[ct], 0, 0, 0);
                        const int k = g * 2 + ct;                         // 6 side slots: 4 DMA + 2 stores
                        if (k < NDMA) {
                            if (more) dma(k, Xn, nbuf);
                        } else if (prev_valid) {
                            *(f32x4*)(prev_ptr + 16 * (k - NDMA)) = (k - NDMA) == 0 ? prev0 : prev1;
                        }
                    }
                }
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) pend[ct][r] = act_apply_fast(ACT, accumulate ? __builtin_fmaf(acc[ct][r], inv, addv[ct][r]) : acc[ct][r] * inv);
                }
            }
            // D: column = lane&15 = point, row = 4*kq + r = channel within the 16-channel tile
            pend_ptr = out + tile0 + lane_out;
            pend_valid = rt < m.rows;                                // decided by the visit that made the tile, never again at store time (KEEP: every visit that runs is kept)
            STAMP_ADD(3);
        };
        // One barrier interval per slab (+ one for the late waves' last contraction).  Early waves: gather(v), contract(v); late
        // waves: contract(v - 1), gather(v).
        for (int v = 0; v <= n_vis; ++v) {
            STAMP_START();
#ifndef SCN_FWD_FREERUN               // (diagnostic build, results WRONG by design: no slab barrier at all -- the no-synchronisation floor)
            // FROMY: the image of slab v was WRITTEN by this workgroup's waves (and every LDS read of the buffer it replaces has
            // returned): wait for the LDS queue; stores and record loads stay in flight across the barrier
            if (FROMY) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            STAMP_ADD(0);
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
#endif
            STAMP_ADD(1);
            const bool stage = FROMY && v + 1 < n_vis;         // both halves stage visit v + 1 during interval v
            if (stage) {
                y_load(slab_of(yw, v + 1));
                if (KEEP) yw = keep_next(yw);
            }
            if (!late) {
                if (v < n_vis) {
                    SCN_FWD_PRIO_GATHER();
                    gather_phase(v);
                    if (stage) y_expand((v + 1) & 1);
                    contract_phase(v);
                }
            } else {
                if (v > 0) contract_phase(v - 1);
                if (stage) y_expand((v + 1) & 1);
                SCN_FWD_PRIO_GATHER();
                if (v < n_vis) gather_phase(v);
            }
        }
    }
    SCN_UNIT_END_MASKED(KEEP);
    };
#ifndef SCN_FWD_NO_STAGGER
    if (wave >> 3) run(std::integral_constant<int, 1>{});
    else run(std::integral_constant<int, 0>{});
#else
    run(std::integral_constant<int, 0>{});
#endif
    STAMP_FLUSH();
    if (pend_ptr && pend_valid) {
        *(f32x4*)(pend_ptr) = pend[0];
        *(f32x4*)(pend_ptr + 16) = pend[1];
    }
}

// The forms of fwd_c32_w16_kernel by name (one function-pointer type; the dispatch never spells FORM).  The
// static_asserts inside the kernel say which combinations exist; here is what X, X0 and fw carry in each:
template <int ACT> constexpr auto fwd_c32_plain = fwd_c32_w16_kernel<ACT>;                        // X = the layer's input; X0 null, fw null
template <int ACT> constexpr auto fwd_c32_power = fwd_c32_w16_kernel<ACT, FWD_EXT0>;              // X = x, X0 = x0 of act(x0 W0 + x W1 + (S x) W2)
template <int ACT> constexpr auto fwd_c32_accum = fwd_c32_w16_kernel<ACT, FWD_ACCUM>;             // X0 = partial pre-activation, added before act
template <int ACT> constexpr auto fwd_c32_from_y = fwd_c32_w16_kernel<ACT, FWD_FROMY>;            // X = the first layer's records y, fw = its weight rows
template <int ACT> constexpr auto fwd_c32_plain_keep = fwd_c32_w16_kernel<ACT, FWD_KEEP>;         // plain, visits by km
template <int ACT> constexpr auto fwd_c32_from_y_keep = fwd_c32_w16_kernel<ACT, FWD_FROMY | FWD_KEEP>;   // from y, visits by km

// ------------------------------------------------------------------------------------------------
// forward, C_in = C_out = 16, sixteen waves, f16 hi + lo split -- the C=32 machinery on TWO slabs at a time:
// a staged 512-byte piece is [slab A: 4 trajectories x 16 channels | slab B: the same], so the plan, the LDS image, the
// XOR addressing and gather_c32 are shared with the C=32 kernels (the LDS-DMA takes a per-lane source address, which is
// all the pairing needs).  wave = 4 rows; lane = (point = lane&15 -> row, trajectory n; channel quad g = lane>>4) holds
// chunk q = the same point of slab A (q=0) and slab B (q=1): two 16-point MFMA tiles, each point with its own scale.
//   per tile: v_mfma_f32_16x16x32_f16 over K = [segment 0 | segment 1] (4 + 4 channels per lane) and
//             v_mfma_f32_16x16x16_f16 over segment 2, each as the three products of the split; weights stay in registers.
// ------------------------------------------------------------------------------------------------
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
// four values: x[j] * s -> hi[j] + lo[j] (see split2)
__device__ __forceinline__ void split2_4(const f32x4 x, float s, f16x4& hi, f16x4& lo) {
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    u32x2 h, l;
    asm("v_fma_mixlo_f16 %0, %4, %8, 0\n\tv_fma_mixlo_f16 %1, %6, %8, 0\n\tv_fma_mixhi_f16 %0, %5, %8, 0\n\tv_fma_mixhi_f16 %1, %7, %8, 0\n\t"
        "v_fma_mixlo_f16 %2, %4, %8, -%0 op_sel_hi:[0,0,1]\n\tv_fma_mixlo_f16 %3, %6, %8, -%1 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %2, %5, %8, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\tv_fma_mixhi_f16 %3, %7, %8, -%1 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\ts_nop 0"
        : "=&v"(h[0]), "=&v"(h[1]), "=&v"(l[0]), "=&v"(l[1]) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(s));
    hi = __builtin_bit_cast(f16x4, h);
    lo = __builtin_bit_cast(f16x4, l);
}

// EXT0 (the power form, see fwd_c32_w16_kernel): act(X0 W0 + X W1 + (S X) W2), segment 0 = the point's own channels of X0 in
// slab A / slab B straight from HBM, the operator has one value array.
// KEEP (plain form, dense launches): see fwd_c32_w16_kernel; each slab of a pair has its own bit.
template <int ACT, unsigned FORM = 0>
__global__ __launch_bounds__(W16_THREADS, 4) void fwd_c16_w16_kernel(PlanDev P, const float* __restrict__ X,
                                                                     const float* __restrict__ X0,
                                                                     const float* __restrict__ W0,
                                                                     const float* __restrict__ W1,
                                                                     const float* __restrict__ W2,
                                                                     float* __restrict__ out, int n_rows, int n_cols,
                                                                     int n_slabs, WorkList wl, KeepMask km) {
    constexpr bool EXT0 = (FORM & FWD_EXT0) != 0, KEEP = (FORM & FWD_KEEP) != 0;
    static_assert((FORM & ~(FWD_EXT0 | FWD_KEEP)) == 0 && (!KEEP || !EXT0), "the slab-pair forward has the power form and the keep mask, on the plain kernel");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int CPP = 32, NDMA = BK_SRC * CPP / W16_THREADS;   // 4 LDS-DMA instructions per wave and slab pair
    const SmemC32 sm = carve_c32(smem);
    const uint32_t lds0 = lds_addr_of(smem);                  // LDS byte address of staging buffer 0
    uint8_t* tws = (uint8_t*)(smem + smem_bytes_c32());
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pt = lane & 15, g = lane >> 4, n = pt >> 2, rt = quad_row(wave, pt & 3);     // quads: see fwd_c32_w16_kernel
    // A fragments: lane (out channel i = lane&15, k-group g): K=32 block = W0 rows 4g..4g+3 then W1 rows 4g..4g+3; K=16: W2 -- all three
    // under one power-of-two scale (their products are added)
    Split2 wa;
    f16x4 wbh, wbl;
    float invW;
    bool w_bad;                                               // a weight is NaN / Inf: no zero-tile early-out (above block_abs_max)
    {
        float w[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            w[j] = W0[(4 * g + j) * 16 + pt];
            w[4 + j] = W1[(4 * g + j) * 16 + pt];
        }
        f32x4 w2;
#pragma unroll
        for (int j = 0; j < 4; ++j) w2[j] = W2[(4 * g + j) * 16 + pt];
        // (the 64 lanes of a wave hold all 3 x 256 weights between them: the largest is a wave reduction, no barrier, no second read)
        const float mw = amax_f4(amax3(amax3(amax3(amax3(0.f, w[0], w[1]), w[2], w[3]), w[4], w[5]), w[6], w[7]), w2);
        const float sW = pow2_scale(max_over_wave(__float_as_uint(mw)), invW);
        w_bad = __builtin_amdgcn_ballot_w64(any_not_finite(w) || not_finite(w2[0]) || not_finite(w2[1]) || not_finite(w2[2]) ||
                                            not_finite(w2[3])) != 0;
        wa = split2(w, sW);
        split2_4(w2, sW, wbh, wbl);
    }
    SCN_UNIT_RANGE();
    if (!listed && slab0 >= slab1) return;
    f32x4 pend[2];
    float* pend_ptr[2] = {nullptr, nullptr};
    // chunk of tile q inside a piece: q*16 + n*4 + g, swizzled like the DMA image (swz32: pos ^ bit 4 of the chunk ^ slot part)
    uint32_t cqs[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) cqs[q] = (uint32_t)((q * 16 + n * 4 + g) ^ q) << 4;
    const size_t slab_bytes = (size_t)n_cols * 256;
    SCN_UNIT_BEGIN()
        wait_all_and_barrier();
        BlockMeta m;
        {
            m.row0 = P.blk_row0[b];
            m.rows = P.blk_rows[b];
            const int sp0 = P.src_ptr[b];
            m.nsrc = P.src_ptr[b + 1] - sp0;
            m.w = P.width[b];
            const int ep = P.ell_ptr[b];
            for (int i = tid; i < m.nsrc; i += W16_THREADS) sm.srcrows[i] = P.src_rows[sp0 + i];
            for (int i = tid; i < m.w * m.rows; i += W16_THREADS) {
                sm.enc[i] = P.ell_enc[ep + i];
                sm.v[i] = P.ell_v[ep + i];
            }
            if (tid < BK_R) sm.self[tid] = P.self_slot[(size_t)b * BK_R + tid];
            if (tid < W16_WAVES) tws[tid] = P.tile_w4[b * W16_WAVES + tid];
        }
        const uint64_t keep = KEEP ? keep_window(km, b, k0) : ~0ull;   // bit `it` = slab k0 + it of this block is stored (dense launches only)
        __syncthreads();
        const int tw = tws[wave];
        const int twu = EXT0 ? 0 : P.tile_wu4[b * W16_WAVES + wave];
        const int rtc = rt < m.rows ? rt : m.rows - 1;
        uint32_t goff[NDMA];
        const bool second = (lane >> 4) & 1;          // this lane's chunks come from slab B: bit 4 of d = bit 4 of pos = lane bit 4
        const int total = m.nsrc * CPP;
#pragma unroll
        for (int i = 0; i < NDMA; ++i) {
            const int c = (i * W16_WAVES + wave) * 64 + lane;
            const int slot = c / CPP, d = swz32(slot, c % CPP);
            goff[i] = c < total ? (uint32_t)sm.srcrows[slot] * 256 + (d & 15) * 16 : 0u;
        }
        auto dma = [&](int k, const char* XA, const char* XB, int bufi) {
            const int base = (k * W16_WAVES + wave) * 64;
            if (base + lane < total) lds_dma16_v((second ? XB : XA) + goff[k], lds0 + (uint32_t)(bufi * (BK_SRC * 512) + base * 16));
        };
        const int n_pairs = (n_it + 1) >> 1;
        {
            const char* XA = (const char*)X + (size_t)SLAB_AT(0) * slab_bytes;
            const char* XB = n_it > 1 ? (const char*)X + (size_t)SLAB_AT(1) * slab_bytes : XA;
#pragma unroll
            for (int i = 0; i < NDMA; ++i) dma(i, XA, XB, 0);
        }
        for (int ip = 0; ip < n_pairs; ++ip) {
            const bool has_b = 2 * ip + 1 < n_it;
            const int slab_a = SLAB_AT(2 * ip), slab_b = has_b ? SLAB_AT(2 * ip + 1) : slab_a;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            const bool more = ip + 1 < n_pairs;
            const char* XnA = (const char*)X + (size_t)(more ? SLAB_AT(2 * ip + 2) : slab_a) * slab_bytes;
            const char* XnB = (more && 2 * ip + 3 < n_it) ? (const char*)X + (size_t)SLAB_AT(2 * ip + 3) * slab_bytes : XnA;
            const int nbuf = (ip + 1) & 1;
            f32x4 z[3][2];                 // [segment][tile q]: channels 4g..4g+3 of this lane's point in slab A / B
            {
                __builtin_amdgcn_s_waitcnt(0xC07F);                     // (see fwd_c32_w16_kernel: lets the compiler count the gather's LDS reads)
                const uint32_t cb[2] = {cqs[0] | (uint32_t)((ip & 1) << 16), cqs[1] | (uint32_t)((ip & 1) << 16)};
                if (EXT0) {                                             // requested before the gather: the latency hides under it
                    const size_t xo = ((size_t)(m.row0 + rtc) * BK_NS + n) * 16 + 4 * g;
                    z[0][0] = *(const f32x4*)(X0 + (size_t)slab_a * n_rows * (BK_NS * 16) + xo);
                    z[0][1] = *(const f32x4*)(X0 + (size_t)slab_b * n_rows * (BK_NS * 16) + xo);
                    f32x4 unused[2];
                    gather_c32<2, false>(sm, rtc, m.w, tw, 0, cb, z[1], z[2], unused);
                } else {
                    gather_c32<2>(sm, rtc, m.w, tw, twu, cb, z[0], z[1], z[2]);
                }
            }
#pragma unroll
            for (int q = 0; q < 2; ++q)                        // the previous pair's results: a whole gather phase old by the
                if (pend_ptr[q]) *(f32x4*)(pend_ptr[q]) = pend[q];   // time the next vmcnt(0) comes
            // the two points' scales: largest magnitude among a point's 48 gathered values (this lane's 12 and its three partner
            // lanes'), both tiles' maxima reduced side by side as the upper halves of their bit patterns (exponent + 7 mantissa bits)
            float sz[2], inv[2];
            const float m0 = amaxn3(amaxn_2x4(0.f, z[0][0], z[1][0]), z[2][0][0], z[2][0][1]);    // (NaN counts)
            const float m1 = amaxn3(amaxn_2x4(0.f, z[0][1], z[1][1]), z[2][1][0], z[2][1][1]);
            const float m0b = amaxn3(m0, z[2][0][2], z[2][0][3]), m1b = amaxn3(m1, z[2][1][2], z[2][1][3]);
            const bool tile_zero = !w_bad && __builtin_amdgcn_ballot_w64(m0b != 0.f || m1b != 0.f) == 0;   // zero-tile early-out (see fwd_c32_w16_kernel)
            if (tile_zero) {
                if (more) {
#pragma unroll
                    for (int k = 0; k < NDMA; ++k) dma(k, XnA, XnB, nbuf);
                }
                pend[0] = pend[1] = f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
            {
                uint32_t mm = __builtin_amdgcn_perm(__float_as_uint(m1b), __float_as_uint(m0b), 0x07060302u);   // (hi16 of m0 | hi16 of m1 << 16)
                {
                    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
                    const auto r = __builtin_amdgcn_permlane16_swap(mm, mm, false, false);
                    u16x2 a = __builtin_bit_cast(u16x2, (uint32_t)r[0]), b = __builtin_bit_cast(u16x2, (uint32_t)r[1]);
                    a = __builtin_elementwise_max(a, b);
                    mm = __builtin_bit_cast(uint32_t, a);
                    const auto q2 = __builtin_amdgcn_permlane32_swap(mm, mm, false, false);
                    a = __builtin_bit_cast(u16x2, (uint32_t)q2[0]);
                    b = __builtin_bit_cast(u16x2, (uint32_t)q2[1]);
                    a = __builtin_elementwise_max(a, b);
                    mm = __builtin_bit_cast(uint32_t, a);
                }
                sz[0] = pow2_scale(mm << 16, inv[0]);
                sz[1] = pow2_scale(mm & 0xffff0000u, inv[1]);
                inv[0] *= invW;
                inv[1] *= invW;
            }
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                float x8[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) { x8[j] = z[0][q][j]; x8[4 + j] = z[1][q][j]; }
                const Split2 za = split2(x8, sz[q]);
                f16x4 zbh, zbl;
                split2_4(z[2][q], sz[q], zbh, zbl);
                // two accumulators: a chain of dependent MFMAs stays within one instruction shape
                f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acb = acc;
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa.lo, za.hi, acc, 0, 0, 0);     // small terms first
                acb = __builtin_amdgcn_mfma_f32_16x16x16f16(wbl, zbh, acb, 0, 0, 0);
                if (more) dma(2 * q, XnA, XnB, nbuf);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa.hi, za.lo, acc, 0, 0, 0);
                acb = __builtin_amdgcn_mfma_f32_16x16x16f16(wbh, zbl, acb, 0, 0, 0);
                if (more) dma(2 * q + 1, XnA, XnB, nbuf);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa.hi, za.hi, acc, 0, 0, 0);
                acb = __builtin_amdgcn_mfma_f32_16x16x16f16(wbh, zbh, acb, 0, 0, 0);
                acc += acb;
#pragma unroll
                for (int r = 0; r < 4; ++r) pend[q][r] = act_apply_fast(ACT, acc[r] * inv[q]);
            }
            }
            // D: column = lane&15 = point, row = 4*g + r = output channel
            const bool valid = rt < m.rows;
            const bool keep_a = !KEEP || ((keep >> (2 * ip)) & 1) != 0, keep_b = !KEEP || ((keep >> (2 * ip + 1)) & 1) != 0;
            pend_ptr[0] = valid && keep_a ? out + (((size_t)slab_a * n_rows + m.row0 + rt) * BK_NS + n) * 16 + 4 * g : nullptr;
            pend_ptr[1] = valid && has_b && keep_b ? out + (((size_t)slab_b * n_rows + m.row0 + rt) * BK_NS + n) * 16 + 4 * g : nullptr;
        }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
        if (pend_ptr[q]) *(f32x4*)(pend_ptr[q]) = pend[q];
}

// The forms of fwd_c16_w16_kernel by name (one function-pointer type; the dispatch never spells FORM):
template <int ACT> constexpr auto fwd_c16_plain = fwd_c16_w16_kernel<ACT>;            // X = the layer's input, X0 unused (null)
template <int ACT> constexpr auto fwd_c16_power = fwd_c16_w16_kernel<ACT, FWD_EXT0>;  // X = x, X0 = x0 of act(x0 W0 + x W1 + (S x) W2)
template <int ACT> constexpr auto fwd_c16_plain_keep = fwd_c16_w16_kernel<ACT, FWD_KEEP>;   // plain, stores by km

// ------------------------------------------------------------------------------------------------
// forward, C_in = 1 -> C_out = C (first layer, TE:143-147 with flow (E,1)): three gathered scalars per point,
// then out = act(x*w0 + lo*w1 + up*w2) written as coalesced float4.
// ------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(BK_THREADS, 6) void fwd_c1_kernel(PlanDev P, const float* __restrict__ X,
                                                               const float* __restrict__ W0,
                                                               const float* __restrict__ W1,
                                                               const float* __restrict__ W2,
                                                               float* __restrict__ out, float* __restrict__ Yout,
                                                               int n_rows, int n_cols, int n_slabs, int act, WorkList wl) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PIECE = 16, CQ = C / 4;
    const Smem sm = carve(smem, PIECE);
    float* Z = (float*)(smem + smem_bytes(PIECE));                    // [2][BK_R*BK_NS][3]
    const int tid = threadIdx.x;
    const int cq = tid % CQ;                                          // constant per thread: 512 % CQ == 0
    const f32x4 w0 = *(const f32x4*)(W0 + cq * 4), w1 = *(const f32x4*)(W1 + cq * 4), w2 = *(const f32x4*)(W2 + cq * 4);
    SCN_UNIT_RANGE();
    if (!listed && slab0 >= slab1) return;
    SCN_UNIT_BEGIN()
        wait_all_and_barrier();
        const BlockMeta m = load_block(P, b, sm);
        __syncthreads();
        // (loaded here, not in the slab loop: a vector load there is followed by s_waitcnt vmcnt(0), i.e. by a wait for the
        // next slab's LDS-DMA that has just been issued)
        const int tw = tid < m.rows * BK_NS ? P.tile_w[b * BK_WAVES + (tid >> 5)] : 0;
        dma_stage<PIECE, 0>((const char*)X + (size_t)SLAB_AT_U(0) * n_cols * PIECE, sm.buf(0), sm, m.nsrc);
        for (int it = 0; it < n_it; ++it) {
            const int slab = SLAB_AT_U(it);
            const float* st = (const float*)sm.buf(it & 1);
            float* Zs = Z + (it & 1) * (BK_R * BK_NS * 3);
            wait_vm_and_barrier();
            if (it + 1 < n_it)
                dma_stage<PIECE, 0>((const char*)X + (size_t)SLAB_AT_U(it + 1) * n_cols * PIECE, sm.buf((it + 1) & 1), sm,
                                    m.nsrc);
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
                Zs[tid * 3] = zs; Zs[tid * 3 + 1] = zl; Zs[tid * 3 + 2] = zu;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // Z visible: LDS writes only -- the next slab's LDS-DMA stays in flight
            __builtin_amdgcn_s_barrier();                        // (__syncthreads() would wait vmcnt(0) as well)
            asm volatile("" ::: "memory");
            if (Yout) {        // the shifted input (x, S_lo x, S_up x, 0) per point, as the first-layer weight gradient takes it
                float* yb = Yout + ((size_t)slab * n_rows + m.row0) * (BK_NS * Y_STRIDE);
                for (int i = tid; i < m.rows * BK_NS; i += BK_THREADS)
                    *(f32x4*)(yb + 4 * i) = f32x4{Zs[3 * i], Zs[3 * i + 1], Zs[3 * i + 2], 0.f};
            }
            float* o = out + ((size_t)slab * n_rows + m.row0) * (BK_NS * C);
            const int total = m.rows * BK_NS * CQ;
            for (int idx = tid; idx < total; idx += BK_THREADS) {
                const int pt = idx / CQ;
                const float zs = Zs[pt * 3], zl = Zs[pt * 3 + 1], zu = Zs[pt * 3 + 2];
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = first_layer_value(act, zs, zl, zu, w0[j], w1[j], w2[j]);
                __builtin_nontemporal_store(v, (f32x4*)(o + (size_t)idx * 4));   // streamed out: keep the L2 for the gathered input
            }
        }
    }
}
