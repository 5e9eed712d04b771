// Teacher-forced scoring of whole node paths (Scone_GCN.path_step_log_probs): the device steps around the batched forwards.  A path
// of n nodes has n - 1 steps; item (path, k) asks for the model's log-probability of node k given the first k nodes.  scn_path_steps
// turns every step into (slot, device row, value of that edge's flow after the step, next step on the same edge) once per call;
// scn_path_slabs writes the flow of any prefix from those records with one writer per word; scn_path_score reads the forward's
// output at the slot actually taken.  No float atomics anywhere: the same inputs give the same bytes.
// Training on whole paths (Scone_GCN.path_grad_step) stages its micro-batches with scn_path_stage: the flows of scn_path_slabs plus
// the items' last nodes and weighted one-hot target rows, into buffers that are kept from step to step.  The dense zero fill of x was
// 34.8 % of the scoring call's kernel time at |E| ~ 1M (profiles/path_scores.txt), so a restage clears only the words the buffer's
// previous items wrote.  The reset is ordered before the writes by SEPARATE LAUNCHES on the one stream (reset, then stage), not by a
// fence inside one wave.
#include "scn_internal.h"

#include <climits>

namespace {

constexpr int WAVE = 64;

struct StepTab {
    const int32_t* deg;
    const int32_t* node;
    const int32_t* edge;
    const float* sign;
    int n_nodes, d, n_rows;
    __device__ __forceinline__ bool has(int v) const { return v >= 0 && v < n_nodes; }
    // the slots of the node v in [0, n_nodes) that hold a neighbour: deg[v] clamped to [0, d]
    __device__ __forceinline__ int live_deg(int v) const {
        const int dv = deg[v];
        return dv < 0 ? 0 : (dv > d ? d : dv);
    }
};

// One wave per path.  Pass 1 looks every step up (slot, row) and writes both; pass 2 takes 64 steps at a time and walks the path's
// steps in tiles of 64 staged in LDS: the running sum of the signs on the own row up to the own step (in step order), and the first
// later step on that row.  Any length: a tile pair costs 64 x 64 LDS compares.  slot / row are read back by the workgroup that wrote
// them, behind a barrier.
__global__ __launch_bounds__(WAVE) void path_steps_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ nodes, StepTab tab,
                                                          int32_t* slot, int32_t* row, float* __restrict__ run,
                                                          int32_t* __restrict__ next_same, int32_t* err) {
    __shared__ int s_row[WAVE];
    __shared__ float s_sign[WAVE];
    const int p = blockIdx.x, lane = threadIdx.x, d = tab.d;
    const int t0 = ptr[p], len = ptr[p + 1] - t0;
    if (len <= 0) return;
    const int n_steps = len - 1;
    if (lane == 0) {                                                 // the path's last position is no step
        const int t = t0 + n_steps;
        slot[t] = -1;
        row[t] = -1;
        run[t] = 0.f;
        next_same[t] = INT_MAX;
    }
    for (int q = lane; q < n_steps; q += WAVE) {
        const int t = t0 + q;
        const int v = nodes[t], u = nodes[t + 1];
        int j = -1, r = -1;
        if (tab.has(v) && tab.has(u)) {                              // nothing is read through an id out of range
            const int dv = tab.live_deg(v);
            const int32_t* nb = tab.node + (size_t)v * d;
            for (int c = 0; c < dv; ++c)
                if (nb[c] == u) {
                    j = c;
                    break;
                }
            if (j >= 0) r = tab.edge[(size_t)v * d + j];
            if (r < 0 || r >= tab.n_rows) j = r = -1;
        }
        if (j < 0) atomicMin(err, t);
        slot[t] = j;
        row[t] = r;
    }
    __syncthreads();
    for (int base = 0; base < n_steps; base += WAVE) {
        const int q = base + lane;
        const bool own = q < n_steps;
        const int r = own ? row[t0 + q] : -1;
        float sum = 0.f;
        int nxt = INT_MAX;
        for (int tb = 0; tb < n_steps; tb += WAVE) {
            const bool open = r >= 0 && nxt == INT_MAX;
            if (tb > base && !__any(open)) break;                    // (wave-uniform) every lane has its next step, the sums are complete
            __syncthreads();
            {
                const int qq = tb + lane;
                int rr = -1;
                float sg = 0.f;
                if (qq < n_steps) {
                    rr = row[t0 + qq];
                    if (rr >= 0) sg = tab.sign[(size_t)nodes[t0 + qq] * d + slot[t0 + qq]];
                }
                s_row[lane] = rr;
                s_sign[lane] = sg;
            }
            __syncthreads();
            if (r >= 0) {
                const int lim = min(WAVE, n_steps - tb);
                for (int c = 0; c < lim; ++c) {
                    if (s_row[c] != r) continue;
                    const int qc = tb + c;
                    if (qc <= q)
                        sum += s_sign[c];
                    else if (nxt == INT_MAX)
                        nxt = t0 + qc;
                }
            }
        }
        if (own) {
            run[t0 + q] = sum;
            next_same[t0 + q] = nxt;
        }
    }
}

// one thread per (slab, row): 16 bytes of zeros
__global__ __launch_bounds__(256) void path_zero_kernel(int64_t n_items, float* __restrict__ x) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_items; t += (int64_t)gridDim.x * blockDim.x)
        *reinterpret_cast<float4*>(x + (size_t)t * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// The prefix of item i: path p and its k nodes, held to the path (a path outside [0, n_paths) or k < 1 is a caller's error that is
// only guarded against: the item is empty).  Returns false for such an item.
__device__ __forceinline__ bool item_prefix(int i, const int32_t* __restrict__ item_path, const int32_t* __restrict__ item_len,
                                            int n_paths, const int32_t* __restrict__ ptr, int& t0, int& k) {
    const int p = item_path[i];
    if (p < 0 || p >= n_paths) return false;
    t0 = ptr[p];
    const int len = ptr[p + 1] - t0;
    k = item_len[i];
    return k >= 1 && k <= len;
}

// one wave per item: step t of the prefix writes its edge's value iff no later step of the prefix crosses that edge again
__global__ __launch_bounds__(WAVE) void path_scatter_kernel(const int32_t* __restrict__ item_path, const int32_t* __restrict__ item_len,
                                                            int n_paths, const int32_t* __restrict__ ptr, const int32_t* __restrict__ row,
                                                            const float* __restrict__ run, const int32_t* __restrict__ next_same,
                                                            int n_rows, float* __restrict__ x) {
    const int i = blockIdx.x, lane = threadIdx.x;
    int t0, k;
    if (!item_prefix(i, item_path, item_len, n_paths, ptr, t0, k)) return;
    const int end = t0 + k - 1;                                      // the prefix's last node: its steps are t0 .. end - 1
    for (int t = t0 + lane; t < end; t += WAVE) {
        const int r = row[t];
        if (r >= 0 && r < n_rows && next_same[t] >= end) x[((size_t)(i >> 2) * n_rows + r) * 4 + (i & 3)] = run[t];
    }
}

// scn_path_stage, launch 1 of the sparse form: one wave per item the buffer held.  The words path_scatter_kernel wrote for that item
// in column i -- the same predicate -- go back to +0; nothing else is touched, so the cost is the prefixes' lengths, not the buffer's.
__global__ __launch_bounds__(WAVE) void path_reset_kernel(const int32_t* __restrict__ item_path, const int32_t* __restrict__ item_len,
                                                          int n_paths, const int32_t* __restrict__ ptr, const int32_t* __restrict__ row,
                                                          const int32_t* __restrict__ next_same, int n_rows, float* __restrict__ x) {
    const int i = blockIdx.x, lane = threadIdx.x;
    int t0, k;
    if (!item_prefix(i, item_path, item_len, n_paths, ptr, t0, k)) return;
    const int end = t0 + k - 1;
    for (int t = t0 + lane; t < end; t += WAVE) {
        const int r = row[t];
        if (r >= 0 && r < n_rows && next_same[t] >= end) x[((size_t)(i >> 2) * n_rows + r) * 4 + (i & 3)] = 0.f;
    }
}

// scn_path_stage, the last launch: one wave per column i < 4 n_slabs.  A valid item scatters its prefix's flow as path_scatter_kernel
// does, and every column writes its last node and its whole target row (zero but for the weight at the slot the path takes next).
__global__ __launch_bounds__(WAVE) void path_stage_kernel(int n_items, const int32_t* __restrict__ item_path,
                                                          const int32_t* __restrict__ item_len, const float* __restrict__ item_weight,
                                                          int n_paths, const int32_t* __restrict__ ptr, const int32_t* __restrict__ nodes,
                                                          const int32_t* __restrict__ slot, const int32_t* __restrict__ row,
                                                          const float* __restrict__ run, const int32_t* __restrict__ next_same,
                                                          int n_rows, int d, float* __restrict__ x, int32_t* __restrict__ last_nodes,
                                                          float* __restrict__ y) {
    const int i = blockIdx.x, lane = threadIdx.x;
    int t0 = 0, k = 0;
    const bool valid = i < n_items && item_prefix(i, item_path, item_len, n_paths, ptr, t0, k);
    const int end = t0 + k - 1;                                      // the prefix's last node: its steps are t0 .. end - 1
    int js = -1;
    float w = 0.f;
    if (valid) {
        for (int t = t0 + lane; t < end; t += WAVE) {
            const int r = row[t];
            if (r >= 0 && r < n_rows && next_same[t] >= end) x[((size_t)(i >> 2) * n_rows + r) * 4 + (i & 3)] = run[t];
        }
        js = slot[end];                                              // -1 where the prefix ends its path
        w = item_weight ? item_weight[i] : 1.f;
    }
    if (lane == 0) last_nodes[i] = valid ? nodes[end] : 0;
    for (int j = lane; j < d; j += WAVE) y[(size_t)i * d + j] = j == js ? w : 0.f;
}

// slot j comes before slot b in the order of scn_beam_step / scn_hop_select: a NaN before every number, then the higher value, then
// the lower slot
__device__ __forceinline__ bool comes_before(float a, int j, float b, int jb) {
    if (isnan(a)) return isnan(b) ? j < jb : true;
    if (isnan(b)) return false;
    return a > b || (a == b && j < jb);
}

// one thread per item
__global__ __launch_bounds__(256) void path_score_kernel(int n_items, const int32_t* __restrict__ item_path,
                                                         const int32_t* __restrict__ item_len, int n_paths,
                                                         const int32_t* __restrict__ ptr, const int32_t* __restrict__ nodes,
                                                         const int32_t* __restrict__ slot, StepTab tab, const float* __restrict__ logp,
                                                         float* __restrict__ step_logp, int32_t* __restrict__ step_rank,
                                                         float* __restrict__ step_mass) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    const int d = tab.d;
    int t0, k, js = -1, lim = 0;
    if (item_prefix(i, item_path, item_len, n_paths, ptr, t0, k)) {
        const int t = t0 + k - 1;
        const int v = nodes[t];
        if (tab.has(v)) {
            lim = tab.live_deg(v);
            js = slot[t];
        }
    }
    if (js < 0 || js >= lim) {
        step_logp[i] = __builtin_nanf("");
        step_rank[i] = -1;
        step_mass[i] = __builtin_nanf("");
        return;
    }
    const float* __restrict__ lp = logp + (size_t)i * d;
    const float own = lp[js];
    int rank = 0, best = 0;
    for (int j = 0; j < lim; ++j) {
        if (j != js && comes_before(lp[j], j, own, js)) ++rank;
        if (j > 0 && comes_before(lp[j], j, lp[best], best)) best = j;
    }
    const float m = lp[best];
    float mass = m;
    if (isfinite(m)) {
        float sum = 0.f;
        for (int j = 0; j < lim; ++j) sum += expf(lp[j] - m);
        mass = m + logf(sum);
    }
    step_logp[i] = own;
    step_rank[i] = rank;
    step_mass[i] = mass;
}

}  // namespace

extern "C" {

int scn_path_steps(int32_t n_paths, const int32_t* path_ptr, const int32_t* path_nodes, int32_t n_nodes, int32_t d, const int32_t* deg,
                   const int32_t* step_node, const int32_t* step_edge, const float* step_sign, int32_t n_rows, int32_t* slot,
                   int32_t* row, float* run, int32_t* next_same, int32_t* err, void* stream) {
    if (n_paths < 0 || n_nodes <= 0 || d <= 0 || n_rows <= 0) return SCN_ERR_BAD_SHAPE;
    if (n_paths == 0) return SCN_OK;
    if (!path_ptr || !path_nodes || !deg || !step_node || !step_edge || !step_sign || !slot || !row || !run || !next_same || !err)
        return SCN_ERR_BAD_ARG;
    return scn::launch_checked(path_steps_kernel, dim3((unsigned)n_paths), dim3(WAVE), 0, (hipStream_t)stream, path_ptr, path_nodes,
                               StepTab{deg, step_node, step_edge, step_sign, n_nodes, d, n_rows}, slot, row, run, next_same, err);
}

int scn_path_slabs(int32_t n_items, int32_t n_slabs, const int32_t* item_path, const int32_t* item_len, int32_t n_paths,
                   const int32_t* path_ptr, const int32_t* row, const float* run, const int32_t* next_same, int32_t n_rows, int32_t ns,
                   float* x, void* stream) {
    if (n_items < 0 || n_slabs < 0 || n_paths < 0 || n_rows <= 0) return SCN_ERR_BAD_SHAPE;
    if (ns != 4) return SCN_ERR_UNSUPPORTED;
    if ((int64_t)n_items > (int64_t)n_slabs * ns) return SCN_ERR_BAD_SHAPE;
    if (n_items == 0) return SCN_OK;
    if (!x || (reinterpret_cast<uintptr_t>(x) & 15) != 0) return SCN_ERR_BAD_ARG;
    if (!item_path || !item_len || !path_ptr || !row || !run || !next_same) return SCN_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t words = (int64_t)n_slabs * n_rows;
    const int64_t blocks = (words + 255) / 256;
    const int status = scn::launch_checked(path_zero_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, words, x);
    if (status != SCN_OK) return status;
    return scn::launch_checked(path_scatter_kernel, dim3((unsigned)n_items), dim3(WAVE), 0, st, item_path, item_len, n_paths, path_ptr,
                               row, run, next_same, n_rows, x);
}

int scn_path_stage(int32_t n_items, int32_t n_slabs, const int32_t* item_path, const int32_t* item_len, const float* item_weight,
                   int32_t n_prev, const int32_t* prev_item_path, const int32_t* prev_item_len, int32_t n_paths, const int32_t* path_ptr,
                   const int32_t* path_nodes, const int32_t* slot, const int32_t* row, const float* run, const int32_t* next_same,
                   int32_t n_rows, int32_t ns, int32_t d, float* x, int32_t* last_nodes, float* y, void* stream) {
    if (n_items < 0 || n_slabs < 0 || n_paths < 0 || n_rows <= 0 || d < 1) return SCN_ERR_BAD_SHAPE;
    if (ns != 4) return SCN_ERR_UNSUPPORTED;
    if ((int64_t)n_items > (int64_t)n_slabs * ns || (int64_t)n_prev > (int64_t)n_slabs * ns) return SCN_ERR_BAD_SHAPE;
    if ((int64_t)n_slabs * ns >= INT_MAX) return SCN_ERR_UNSUPPORTED;      // a column is an int and a grid index
    if (n_slabs == 0) return SCN_OK;
    if (!x || (reinterpret_cast<uintptr_t>(x) & 15) != 0 || !last_nodes || !y) return SCN_ERR_BAD_ARG;
    if (n_items > 0 && (!item_path || !item_len || !path_nodes || !slot || !run)) return SCN_ERR_BAD_ARG;
    if (n_prev > 0 && (!prev_item_path || !prev_item_len)) return SCN_ERR_BAD_ARG;
    if ((n_items > 0 || n_prev > 0) && (!path_ptr || !row || !next_same)) return SCN_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    int status = SCN_OK;
    if (n_prev < 0) {
        const int64_t words = (int64_t)n_slabs * n_rows;
        const int64_t blocks = (words + 255) / 256;
        status = scn::launch_checked(path_zero_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, words, x);
    } else if (n_prev > 0) {
        status = scn::launch_checked(path_reset_kernel, dim3((unsigned)n_prev), dim3(WAVE), 0, st, prev_item_path, prev_item_len, n_paths,
                                     path_ptr, row, next_same, n_rows, x);
    }
    if (status != SCN_OK) return status;
    return scn::launch_checked(path_stage_kernel, dim3((unsigned)(n_slabs * ns)), dim3(WAVE), 0, st, n_items, item_path, item_len,
                               item_weight, n_paths, path_ptr, path_nodes, slot, row, run, next_same, n_rows, d, x, last_nodes, y);
}

int scn_path_score(int32_t n_items, int32_t d, const int32_t* item_path, const int32_t* item_len, int32_t n_paths,
                   const int32_t* path_ptr, const int32_t* path_nodes, const int32_t* slot, const int32_t* deg, int32_t n_nodes,
                   const float* logp, float* step_logp, int32_t* step_rank, float* step_mass, void* stream) {
    if (n_items < 0 || d <= 0 || n_paths < 0 || n_nodes <= 0) return SCN_ERR_BAD_SHAPE;
    if ((int64_t)n_items * d >= INT_MAX) return SCN_ERR_UNSUPPORTED;
    if (n_items == 0) return SCN_OK;
    if (!item_path || !item_len || !path_ptr || !path_nodes || !slot || !deg || !logp || !step_logp || !step_rank || !step_mass)
        return SCN_ERR_BAD_ARG;
    return scn::launch_checked(path_score_kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_items,
                               item_path, item_len, n_paths, path_ptr, path_nodes, slot,
                               StepTab{deg, nullptr, nullptr, nullptr, n_nodes, d, 0}, logp, step_logp, step_rank, step_mass);
}

}  // extern "C"
