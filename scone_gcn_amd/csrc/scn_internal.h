// Internal declarations shared by the translation units of libscone_hip.so (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <map>
#include <type_traits>
#include <vector>

#include "scone_hip.h"
#include "scn_blk_record.h"

namespace scn {

void set_hip_error(hipError_t e, const char* where);

#define SCN_HIP_TRY(expr)                                   \
    do {                                                    \
        hipError_t _e = (expr);                             \
        if (_e != hipSuccess) {                             \
            ::scn::set_hip_error(_e, #expr);                \
            return SCN_ERR_HIP;                             \
        }                                                   \
    } while (0)

#define SCN_LAUNCH_CHECK()                                  \
    do {                                                    \
        hipError_t _e = hipGetLastError();                  \
        if (_e != hipSuccess) {                             \
            ::scn::set_hip_error(_e, "kernel launch");      \
            return SCN_ERR_HIP;                             \
        }                                                   \
    } while (0)

// The runtime activation code as a compile-time constant: calls f(std::integral_constant<int, SCN_ACT_x>{}) and returns its status.
// Kernels take the activation as a template parameter; this is the one switch that picks the instantiation.  A code outside the
// four runs as SCN_ACT_NONE (an entry point that refuses such a code checks it before the call).  SCN_HIP_TRY / SCN_LAUNCH_CHECK
// inside f return out of f: it returns int, and the caller hands that on.
template <class F>
static inline int with_act(int act, F&& f) {
    switch (act) {
        case SCN_ACT_TANH: return f(std::integral_constant<int, SCN_ACT_TANH>{});
        case SCN_ACT_RELU: return f(std::integral_constant<int, SCN_ACT_RELU>{});
        case SCN_ACT_LEAKY_RELU: return f(std::integral_constant<int, SCN_ACT_LEAKY_RELU>{});
        default: return f(std::integral_constant<int, SCN_ACT_NONE>{});
    }
}

// One checked launch of the kernel (form) k: dynamic LDS above 64 KB is opted into per kernel (160 KB is what a CU has:
// SCN_ERR_UNSUPPORTED beyond), a launch error becomes SCN_ERR_HIP.  The arguments convert to k's parameter types (nullptr included).
template <class... KA, class... A>
static inline int launch_checked(void (*k)(KA...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A&&... a) {
    static_assert(sizeof...(KA) == sizeof...(A), "one argument per kernel parameter");
    if (lds > 160 * 1024) return SCN_ERR_UNSUPPORTED;
    if (lds > 64 * 1024)
        SCN_HIP_TRY(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, grid, block, lds, st, static_cast<KA>(a)...);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

// relu and its negative-part twin that keep a NaN a NaN, like the reference's np.maximum (fmaxf(z, 0.f) returns 0 for a NaN z)
__device__ __forceinline__ float relu_nan(float z) { return z <= 0.f ? 0.f : z; }
__device__ __forceinline__ float neg_part_nan(float z) { return z >= 0.f ? 0.f : z; }

// activation and its derivative expressed through the OUTPUT value y (what the backward has at hand)
// tanh to ~3e-7 absolute: odd Taylor polynomial below 1/8, 1 - 2/(e^{2|x|}+1) on v_exp_f32 / v_rcp_f32 above
__device__ __forceinline__ float fast_tanh(float x) {
    const float ax = fabsf(x), x2 = x * x;
    const float poly = x * fmaf(x2, fmaf(x2, fmaf(x2, -17.f / 315.f, 2.f / 15.f), -1.f / 3.f), 1.f);
    const float t = __builtin_amdgcn_exp2f(ax * 2.885390081777927f);
    const float r = 1.f - 2.f * __builtin_amdgcn_rcpf(t + 1.f);
    return ax < 0.125f ? poly : copysignf(r, x);
}
__device__ __forceinline__ float act_apply_fast(int act, float z) {
    switch (act) {
        case SCN_ACT_TANH: return fast_tanh(z);
        case SCN_ACT_RELU: return relu_nan(z);
        case SCN_ACT_LEAKY_RELU: return z >= 0.f ? z : 0.01f * z;
        default: return z;
    }
}
// One value of the first layer's output (1 -> C channels): H1[p][c] = act(x w0[c] + (S_lo x) w1[c] + (S_up x) w2[c]) from the point's
// shifted-input record y[p] = (ys, yl, yu, 0).  The ONE definition: fwd_c1_kernel writes it, the from-y forward and the aux-free
// fused-first backward rebuild it instead of reading it back, and all three must round alike -- every multiply-add spelled out
// (see adam_update for what contraction does otherwise).
__device__ __forceinline__ float first_layer_value(int act, float ys, float yl, float yu, float w0, float w1, float w2) {
    return act_apply_fast(act, __builtin_fmaf(yu, w2, __builtin_fmaf(yl, w1, ys * w0)));
}
// first-layer weight rows handed to the kernels that rebuild H1 (by value; all null elsewhere)
struct FirstW { const float* w[3]; };
__device__ __forceinline__ float act_apply(int act, float z) {
    switch (act) {
        case SCN_ACT_TANH: return tanhf(z);
        case SCN_ACT_RELU: return relu_nan(z);
        case SCN_ACT_LEAKY_RELU: return z >= 0.f ? z : 0.01f * z;
        default: return z;
    }
}
__device__ __forceinline__ float act_grad_from_output(int act, float y) {
    switch (act) {
        case SCN_ACT_TANH: return 1.f - y * y;
        case SCN_ACT_RELU: return y > 0.f ? 1.f : 0.f;
        case SCN_ACT_LEAKY_RELU: return y >= 0.f ? 1.f : 0.01f;
        default: return 1.f;
    }
}

// One parameter's ridge + Adam update (scn_adam_step, STM:300-326), every multiply-add spelled out: all kernels that apply it must round
// alike (left to the compiler's contraction, `a * b + c * d` became fma(a, b, c * d) in one kernel and fma(c, d, a * b) in another).
// c1 = 1 - b1^(i+1), c2 = 1 - b2^(i+1) (adam_corrections); wd2 = 2 * weight_decay.
__device__ __forceinline__ void adam_update(float* __restrict__ w, float g_raw, float* __restrict__ m, float* __restrict__ v, float lr,
                                            float b1, float b2, float eps, float c1, float c2, float wd2, float g_scale) {
#pragma clang fp contract(off)
    const float wi = *w;
    const float gi = fmaf(g_raw, g_scale, wd2 * wi);
    const float mi = fmaf(1.f - b1, gi, b1 * *m);
    const float vi = fmaf((1.f - b2) * gi, gi, b2 * *v);
    *m = mi;
    *v = vi;
    *w = wi - lr * (mi / c1) / (sqrtf(vi / c2) + eps);
}
__host__ __device__ __forceinline__ void adam_corrections(float b1, float b2, int i, float& c1, float& c2) {
    c1 = 1.f - (float)pow((double)b1, (double)(i + 1));
    c2 = 1.f - (float)pow((double)b2, (double)(i + 1));
}

// Philox4x32-10 (Salmon et al., SC'11): the counter-based generator behind the sampled multi-hop decoder, one definition for the
// host entry point (scn_sample_uniform) and the kernels.  out = the block function of (counter, key).
__host__ __device__ __forceinline__ void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}
// The uniform of (seed, root, sample, hop) in [0, 1), 24 bits: keyed by these four and by nothing else (not the launch, the chunk or
// the entry the sample sits in).
__host__ __device__ __forceinline__ float sample_uniform(uint64_t seed, int32_t root, int32_t sample, int32_t hop) {
    const uint32_t ctr[4] = {(uint32_t)root, (uint32_t)sample, (uint32_t)hop, 0u};
    const uint32_t key[2] = {(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)};
    uint32_t out[4];
    philox4x32_10(ctr, key, out);
    return (float)(out[0] >> 8) * 5.9604644775390625e-8f;     // 2^-24: exact
}

// Row r of slab s of a tree level's input: the root columns of its ns = 4 leaves 4 s .. 4 s + 3 (0 past the last leaf and for a leaf
// without a root), as the one 16-byte store the slab builders of scn_hops.hip and scn_field.hip make of them.
__device__ __forceinline__ float4 root_columns(int64_t s, int r, int n_leaves, const int32_t* __restrict__ root, int n_roots,
                                               const float* __restrict__ root_x, int n_rows) {
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t l = s * 4 + q;
        const int rt = l < n_leaves ? root[l] : -1;
        v[q] = (rt >= 0 && rt < n_roots) ? root_x[((size_t)(rt >> 2) * n_rows + r) * 4 + (rt & 3)] : 0.f;
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}

struct Group {
    int32_t n_cols = 0, identity = 0, n_vals = 0;
    int64_t nnz = 0;
    int32_t slot_base = 0, n_slots = 0;
    // device copies
    int32_t* d_rowptr = nullptr;
    int32_t* d_col = nullptr;
    float* d_val0 = nullptr;
    float* d_val1 = nullptr;
    // host copies (plan building)
    std::vector<int32_t> h_rowptr, h_col;
    std::vector<float> h_val0, h_val1;
};

// ---- LDS-blocked execution plan of a single-group operator (scn_blocked.hip) ----
constexpr int BK_WAVES = 8;
constexpr int BK_R = 8 * BK_WAVES;   // output rows per block (upper bound; 8 per wave)
constexpr int BK_SRC = 128;     // staged source pieces per block (upper bound)
constexpr int BK_NS = 4;        // trajectories per slab the blocked kernels are built for
constexpr int BK_THREADS = 64 * BK_WAVES;
constexpr int BK_ELL_CAP = 1152;  // ELL entries (rows-in-block x padded width) a block may carry (64 rows x 18; 4 % of the blocks of the
                                  // benchmark complex are cut a few rows short by it: the 2 KB go to the backward's selection fragments)

// device view passed to kernels by value
struct PlanDev {
    int32_t n_blocks, ell_w_max;
    const int32_t* blk_row0;    // [n_blocks] first output row
    const uint8_t* blk_rows;    // [n_blocks] rows in block (<= BK_R)
    const int32_t* src_ptr;     // [n_blocks+1]
    const int32_t* src_rows;    // staged source rows by slot (slot & 3 = the LDS bank class of the source: scn_blk_layout.inc)
    const int32_t* ell_ptr;     // [n_blocks] entry offset (entries are [t][BK_R])
    const uint8_t* width;       // [n_blocks] padded entries per row
    const uint8_t* tile_w;      // [n_blocks][BK_WAVES] entries needed by each wave's 8 rows
    const uint8_t* tile_w4;     // [n_blocks][2*BK_WAVES] the same per QUAD: rows {0,3,5,6} / {1,2,4,7} of an 8-row group (16-wave kernels)
    const uint8_t* tile_wu;     // [n_blocks][BK_WAVES] leading entries that carry a non-zero val1 (rows are ordered that way)
    const int32_t* assign;      // optional [n_blocks]: visit position -> block (cost-balanced static assignment, per launch grid)
    const uint8_t* tile_wu4;    // [n_blocks][2*BK_WAVES]
    const uint8_t* ell_slot;    // local slot of entry
    const uint16_t* ell_enc;    // the same for 512-byte pieces, ready to XOR into an LDS address: slot*512 | (slot&3)*32
    const float2* ell_v;        // (val0, val1) of entry
    const uint8_t* self_slot;   // [n_blocks][BK_R] slot of the row itself (identity shift)
};
static_assert(BLK_REC_WAVES == BK_WAVES, "a record carries the tile widths of the 8-wave kernels");

// optional (block, slab) work list of the zero-skipping mode (scn_work_list); block == nullptr: every block, every slab
struct WorkList {
    int32_t n_work;
    const int32_t* block;   // [n_work] plan block index
    const int32_t* ptr;     // [n_work + 1] offsets into slab
    const int32_t* slab;    // active slabs of each listed block, ascending
};

// optional keep mask of a last layer's forward (scn_keep_mask): bit s & 31 of bits[b * words + (s >> 5)] = (block b, slab s) is
// stored; bits == nullptr: everything is
struct KeepMask {
    const uint32_t* bits;
    int32_t words;          // words per block = ceil(n_slabs / 32)
};

// optional unit list of a keep mask (scn_keep_mask_units / scn_mask_hop_units): entry = block * words + word of every non-empty word
// of the mask, each once, in any order; units == nullptr: the workgroups walk their static units
struct UnitList {
    const uint32_t* units;
    const uint32_t* count;  // the number of entries (device)
};

// extra plan arrays of a "terms" operator (fused Bunch layer, scn_terms.inc); the common part lives in BlockPlan
struct TermsPlan {
    bool built = false;
    int group_rows = 0;                 // rows per wave of the kernel the plan was cut for (4: forward, 8: backward)
    int32_t bins[3] = {0, 0, 0};        // rows of each level a block can hold
    const int32_t* blk_row0 = nullptr;  // [n_blocks][3]
    const uint8_t* blk_rows = nullptr;  // [n_blocks][4]
    const uint8_t* blk_w = nullptr;     // [n_blocks][4]
    const uint8_t* grp = nullptr;       // [n_blocks][16][5]
    int32_t lvl_row0[4] = {0, 0, 0, 0};
};

struct BlockPlan {
    bool built = false;
    PlanDev dev{};
    const BlockRec* blk_rec = nullptr;   // [n_blocks] the header fields of `dev` and tile_w / tile_wu, packed: 32 bytes per block (scn_blk_record.h);
                                         // not part of PlanDev: only the visiting backwards read it, as a kernel argument of their own
    double mean_src_per_row = 0.0;
    int64_t gather_positions = 0, gather_cycles = 0;   // simulated lane-group reads of one gather pass and their LDS cycles (scn_blk_layout.inc)
    std::vector<int32_t> h_row0;   // first row of every block (+ n_rows): scn_conv_plan_blocks
    std::vector<float> h_cost;     // relative cost of one slab of every block (balanced_assignment)
    std::map<int, const int32_t*> assign_by_grid;   // grid.x -> device table, built with the plan
    std::vector<void*> allocs;
};

}  // namespace scn

struct scn_conv_s {
    int32_t n_rows = 0, n_groups = 0, n_slots = 0;
    scn::Group g[SCN_MAX_GROUPS];
    int32_t slot_group[SCN_MAX_SLOTS] = {0, 0, 0, 0};
    int32_t slot_kind[SCN_MAX_SLOTS] = {0, 0, 0, 0};   // 0 identity, 1 val0, 2 val1
    scn::BlockPlan plan;
    scn::TermsPlan terms;
    void* small_pack = nullptr;         // (col, val0, val1, 0) per entry for scn_small_step, built by scn_conv_create* (small_prepare; owned through plan.allocs)
    void* small_ell = nullptr;          // the first twelve entries of every row at a fixed stride, columns as LDS offsets: [n_rows][12] float4 (same owner)
    void* small_ovf = nullptr;          // the entries past the twelfth of each row in the same form, small_n_ovf of them,
    int32_t* small_ovf_ptr = nullptr;   // [n_rows + 1] a row's range among them
    int32_t small_n_ovf = 0;
    std::vector<uint8_t> block_start;   // optional layout hint: 1 where a block of the plan must start (see scn_plan_refine_order)
};

namespace scn {
int small_prepare(scn_conv_s* c);      // scn_small.hip: the entry pack + LDS limit of scn_small_step, at create time

// ---- scn_blocked.hip as scn_conv.hip calls it: the ONE declaration of each ----
constexpr WorkList NO_LIST{0, nullptr, nullptr, nullptr};

// What a launch of a fused layer kernel is given, one record per family.  The leading fields are what every launch of the family has
// (aggregate-initialised, in this order); the ones with a default are options, absent unless a call site sets them BY NAME.
struct FwdLaunch {                          // blocked_forward (and blocked_shifted_input_keep: src, y_out, keep, units)
    int n_slabs;
    const float* src;                       // the layer's input, c_in channels
    int c_in;
    const float* const* W;
    int c_out, act;
    float* out;                             // null (c_in = 1): the first layer's shifted input only, into y_out
    hipStream_t st;
    float* y_out = nullptr;                 // c_in = 1: the shifted-input records, beside out
    WorkList wl = NO_LIST;                  // zero-skipping work list
    const float* partial = nullptr;         // 32 -> 32: out = act(partial + ...), see fwd_c32_w16_kernel
    const uint32_t* keep = nullptr;         // 32 -> 32 and 16 -> 16, dense, no partial: only the mask's items are stored (32 -> 32: visited)
    const uint32_t* units = nullptr;        // the mask's unit list and its count (32 -> 32 and the shifted input; unit_list_of)
    const uint32_t* unit_count = nullptr;
};
struct FromYLaunch {                        // blocked_forward_from_y: 32 channels, dense
    int n_slabs;
    const float* y;                         // the first layer's shifted-input records
    const float* const* W_first;
    const float* const* W;
    int act;
    float* out;
    hipStream_t st;
    const uint32_t* keep = nullptr;         // visits and stores by the mask, as FwdLaunch
    const uint32_t* units = nullptr;
    const uint32_t* unit_count = nullptr;
};
struct BwdLaunch {                          // blocked_backward
    int n_slabs;
    const float* dz;
    int c_dz;
    const float* const* W;
    const float* aux;
    int c_aux, act;
    float* dx;                              // null: weight gradients only
    float* const* dW;
    void* ws;                               // blocked_backward_workspace bytes
    hipStream_t st;
    WorkList wl = NO_LIST;
    const float* dx_partial = nullptr;      // 32 -> 32: dx = dx_partial + (...) act', see bwd_c32_bf16_kernel
    const uint32_t* dzmask = nullptr;       // 32 -> 32, dense, no partial: dz is staged by the source mask, see there
    const uint32_t* visit = nullptr;        // the same shapes, no dzmask: only the mask's items are visited, see there
    int32_t* defer_n_wg = nullptr;          // given: no reduce launch -- the partials [n_wg][c_aux][3 c_dz] stay at the head of ws for the step
                                            // epilogue (scn_step_epilogue), and n_wg is written here
};
struct BwdFirstLaunch {                     // blocked_backward_first: the layer behind the first one, fused with dW_first
    int n_slabs;
    const float* dz;
    const float* const* W;
    int ch, act;
    const float* y;                         // the first layer's shifted-input records
    float* const* dW;
    float* const* dW_first;
    void* ws;                               // blocked_backward_first_workspace bytes
    hipStream_t st;
    const float* aux = nullptr;             // the first layer's output; absent with W_first
    const float* const* W_first = nullptr;  // 32 channels: aux is rebuilt from y, not read
    WorkList wl = NO_LIST;
    const uint32_t* visit = nullptr;        // with W_first, dense: only the mask's items are visited
    int32_t* defer_n_wg = nullptr;          // given: neither reduce is launched -- ws keeps [n_wg][3 ch ch] and behind it [n_wg][96], n_wg is written here
};

int build_block_plan(scn_conv_s* c);
void free_block_plan(scn_conv_s* c);
bool blocked_forward_supported(const scn_conv_s* c, int ns, const int32_t* c_in, int c_out);
int blocked_forward(scn_conv_s* c, const FwdLaunch& a);
int blocked_shifted_input_keep(scn_conv_s* c, const FwdLaunch& a);
bool blocked_forward_from_y_supported(const scn_conv_s* c, int ns, int ch);
int blocked_forward_from_y(scn_conv_s* c, const FromYLaunch& a);
bool blocked_backward_supported(const scn_conv_s* c, int ns, const int32_t* c_dz, int c_aux);
size_t blocked_backward_workspace(const scn_conv_s* c, int n_slabs, int ns, const int32_t* c_dz, int c_aux);
int blocked_backward(scn_conv_s* c, const BwdLaunch& a);
bool blocked_backward_first_supported(const scn_conv_s* c, int ns, int ch);
size_t blocked_backward_first_workspace(const scn_conv_s* c, int n_slabs, int ns, int ch);
int blocked_backward_first(scn_conv_s* c, const BwdFirstLaunch& a);
bool blocked_power_supported(const scn_conv_s* c, int ns, int ch);
size_t blocked_power_backward_workspace(const scn_conv_s* c, int n_slabs, int ns, int ch);
int blocked_power_forward(scn_conv_s* c, int n_slabs, const float* x0, const float* x, const float* const* W, int ch, int act,
                          float* out, hipStream_t st);
int blocked_power_backward(scn_conv_s* c, int n_slabs, const float* dz, const float* g1, const float* const* W,
                           const float* aux, int ch, int act, float* dx, float* const* dW, void* ws, hipStream_t st);
bool blocked_dw_first_supported(const scn_conv_s* c, int ns, int cd);
size_t blocked_dw_first_workspace(const scn_conv_s* c, int n_slabs, int ns, int cd);
int blocked_dw_first(scn_conv_s* c, int n_slabs, const float* x, const float* y, const float* dz, int cd,
                     float* const* dW, void* ws, const WorkList* wl, hipStream_t st);
int blocked_clear_list(scn_conv_s* c, int ns, int ch, float* t, const WorkList* wl, hipStream_t st);
int blocked_clear_mask(scn_conv_s* c, int n_slabs, int ns, int ch, float* t, const uint32_t* mask, hipStream_t st);
int blocked_step_epilogue(scn_conv_s* c, const scn_step_epilogue_desc& d, hipStream_t st);
int blocked_dw_reduce_alone(const float* partial, int n_wg, int c_aux, int cd, float* const* dW, hipStream_t st);
int blocked_dw_first_reduce_alone(const float* partial, int n_wg, int form, float* const* dW, hipStream_t st);
bool blocked_spmm_supported(const scn_conv_s* c, int k);
int blocked_spmm(scn_conv_s* c, int n_slabs, int k, const float* x, float* ya, float* yb, hipStream_t st);
int blocked_window_scan_probe(scn_conv_s* c, int n_slabs, const uint32_t* mask, int gx, int slab0, int n_it, int cap, int32_t* out_block,
                              uint64_t* out_window, int32_t* out_count, int32_t* unit_block, hipStream_t st);
int build_terms_plan(scn_conv_s* c, const uint8_t* term, const int32_t* lvl_row0, const uint8_t* merged, const int32_t* bins,
                     int group_rows);
int terms_forward(scn_conv_s* c, int n_slabs, const float* const* x, const float* const* W, int act, float* const* out,
                  hipStream_t st);
size_t terms_backward_workspace(const scn_conv_s* c, int n_slabs);
int terms_backward(scn_conv_s* c, int n_slabs, const float* const* dz, const float* const* W, const float* const* aux, int act,
                   float* const* dx, float* const* dW, const float* const* y, float* const* dW_first, void* ws, hipStream_t st);
}
