// Field-of-view work lists of multi-hop prediction, built on the device.  The leaves of a level exist on
// the device only and change at every hop, so the (block, slab) lists the *_list forwards take cannot come from the host: from the
// leaves' nodes and two block-level CSR tables (node -> blocks the readout reads, block -> blocks a block's rows stage) these
// kernels mark, hop and compact the lists of every layer, and scn_tree_slabs_list fills only the listed items of a level's input.
// Integer work only; every racing store writes the same value; nothing here allocates or synchronises.
#include "scn_internal.h"

#include <climits>

namespace {

using namespace scn;

constexpr int FL_THREADS = 256;
constexpr int FL_SCAN = 256;          // threads of the one workgroup that scans a level's blocks

// marks are bytes [level][block][slab]: one thread per leaf stores a 1 for every block of T(node) in the leaf's slab
__global__ __launch_bounds__(FL_THREADS) void field_mark_kernel(int n, int ns, const int32_t* __restrict__ node, int n_nodes,
                                                                const int32_t* __restrict__ top_ptr, const int32_t* __restrict__ top_blk,
                                                                int n_blocks, int n_slabs, uint8_t* __restrict__ mark) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int v = node[i];
    if (v < 0 || v >= n_nodes) return;
    const int s = i / ns;
    for (int k = top_ptr[v]; k < top_ptr[v + 1]; ++k) {
        const int b = top_blk[k];
        if (b >= 0 && b < n_blocks) mark[(size_t)b * n_slabs + s] = 1;
    }
}

// one level down: every marked (b, s) of the upper level marks (b', s) for b' in A(b); slabs run fastest over the threads
__global__ __launch_bounds__(FL_THREADS) void field_hop_kernel(int n_blocks, int n_slabs, const int32_t* __restrict__ adj_ptr,
                                                               const int32_t* __restrict__ adj_blk, const uint8_t* __restrict__ upper,
                                                               uint8_t* __restrict__ lower) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)n_blocks * n_slabs) return;
    if (!upper[t]) return;
    const int b = (int)(t / n_slabs), s = (int)(t - (int64_t)b * n_slabs);
    for (int k = adj_ptr[b]; k < adj_ptr[b + 1]; ++k) {
        const int b2 = adj_blk[k];
        if (b2 >= 0 && b2 < n_blocks) lower[(size_t)b2 * n_slabs + s] = 1;
    }
}

// one wave per (level, block): the number of marked slabs
__global__ __launch_bounds__(FL_THREADS) void field_count_kernel(int n_items, int n_slabs, const uint8_t* __restrict__ mark,
                                                                 int32_t* __restrict__ cnt) {
    const int w = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (w >= n_items) return;                                                // (wave-uniform)
    const uint8_t* __restrict__ m = mark + (size_t)w * n_slabs;
    int c = 0;
    for (int s = lane; s < n_slabs; s += 64) c += m[s] != 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) cnt[w] = c;
}

// one workgroup per level: exclusive scans over the blocks of (cnt > 0) and of cnt.  Thread t owns a contiguous run of blocks; the
// FL_SCAN run totals are scanned in LDS.  Writes the level's counts, and -- when its items fit cap -- block, ptr and every block's
// slab offset (off, workspace) for the fill pass.
__global__ __launch_bounds__(FL_SCAN) void field_scan_kernel(int n_blocks, int64_t cap, const int32_t* __restrict__ cnt,
                                                             int32_t* __restrict__ off, int32_t* __restrict__ block,
                                                             int32_t* __restrict__ ptr, int32_t* __restrict__ counts) {
    __shared__ int s_nw[FL_SCAN], s_it[FL_SCAN];
    const int level = blockIdx.x, tid = threadIdx.x;
    const int32_t* __restrict__ c_l = cnt + (size_t)level * n_blocks;
    int32_t* __restrict__ off_l = off + (size_t)level * n_blocks;
    int32_t* __restrict__ block_l = block + (size_t)level * n_blocks;
    int32_t* __restrict__ ptr_l = ptr + (size_t)level * (n_blocks + 1);
    const int per = (n_blocks + FL_SCAN - 1) / FL_SCAN;
    const int b0 = min(n_blocks, tid * per), b1 = min(n_blocks, b0 + per);
    int nw = 0, it = 0;
    for (int b = b0; b < b1; ++b) {
        const int c = c_l[b];
        nw += c > 0;
        it += c;
    }
    s_nw[tid] = nw;
    s_it[tid] = it;
    __syncthreads();
    for (int o = 1; o < FL_SCAN; o <<= 1) {                                  // inclusive scan of the run totals
        const int a = tid >= o ? s_nw[tid - o] : 0, d = tid >= o ? s_it[tid - o] : 0;
        __syncthreads();
        s_nw[tid] += a;
        s_it[tid] += d;
        __syncthreads();
    }
    const int total_nw = s_nw[FL_SCAN - 1], total_it = s_it[FL_SCAN - 1];
    if (tid == 0) {
        counts[2 * level] = total_nw;
        counts[2 * level + 1] = total_it;
    }
    if ((int64_t)total_it > cap) return;                                      // counts only: the caller sizes up or runs dense
    int u = s_nw[tid] - nw, k = s_it[tid] - it;
    for (int b = b0; b < b1; ++b) {
        const int c = c_l[b];
        off_l[b] = k;
        if (c > 0) {
            block_l[u] = b;
            ptr_l[u] = k;
            ++u;
            k += c;
        }
    }
    if (tid == 0 && total_nw > 0) ptr_l[total_nw] = total_it;           // (an empty level writes its counts and nothing else)
}

// one wave per (level, block): the marked slabs in ascending order from the block's offset, 64 slabs per ballot
__global__ __launch_bounds__(FL_THREADS) void field_fill_kernel(int n_items, int n_blocks, int n_slabs, int64_t cap,
                                                                const uint8_t* __restrict__ mark, const int32_t* __restrict__ cnt,
                                                                const int32_t* __restrict__ off, const int32_t* __restrict__ counts,
                                                                int32_t* __restrict__ slab) {
    const int w = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (w >= n_items) return;                                                // (wave-uniform, as are the two below)
    if (cnt[w] == 0) return;
    const int level = w / n_blocks;
    if ((int64_t)counts[2 * level + 1] > cap) return;
    const uint8_t* __restrict__ m = mark + (size_t)w * n_slabs;
    int32_t* __restrict__ out = slab + (size_t)level * cap + off[w];
    int k = 0;
    for (int base = 0; base < n_slabs; base += 64) {
        const int s = base + lane;
        const bool on = s < n_slabs && m[s] != 0;
        const unsigned long long mask = __ballot(on);
        if (on) out[k + __popcll(mask & ((1ull << lane) - 1ull))] = s;
        k += __popcll(mask);
    }
}

// scn_tree_slabs over the listed items only: one workgroup walks listed blocks, a thread one (slab, row) of the block at a time
__global__ __launch_bounds__(FL_THREADS) void tree_copy_list_kernel(PlanDev P, WorkList wl, int n_leaves, int n_slabs,
                                                                    const int32_t* __restrict__ root, int n_roots,
                                                                    const float* __restrict__ root_x, int n_rows, float* __restrict__ x) {
    for (int u = blockIdx.x; u < wl.n_work; u += gridDim.x) {
        const int b = wl.block[u];
        if (b < 0 || b >= P.n_blocks) continue;
        const int row0 = P.blk_row0[b], rows = P.blk_rows[b];
        const int k0 = wl.ptr[u], total = (wl.ptr[u + 1] - k0) * rows;
        for (int i = threadIdx.x; i < total; i += FL_THREADS) {
            const int s = wl.slab[k0 + i / rows], r = row0 + i % rows;
            if (s < 0 || s >= n_slabs || r >= n_rows) continue;
            *reinterpret_cast<float4*>(x + ((size_t)s * n_rows + r) * 4) = scn::root_columns(s, r, n_leaves, root, n_roots, root_x, n_rows);
        }
    }
}

// index of the last element <= key of an ascending array (-1: none)
__device__ __forceinline__ int last_le(const int32_t* __restrict__ a, int n, int key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// one thread per leaf, its path entries in level order (the last write wins); an entry is set only where (block of the row, the
// leaf's slab) is listed: three binary searches over ascending arrays (blk_row0, the listed blocks, the block's slabs)
__global__ __launch_bounds__(FL_THREADS) void tree_patch_list_kernel(PlanDev P, WorkList wl, int n_leaves, int h,
                                                                     const int32_t* __restrict__ path_row,
                                                                     const float* __restrict__ path_sign, int n_rows, float* __restrict__ x) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_leaves) return;
    const int s = l >> 2;
    for (int q = 0; q < h; ++q) {
        const int r = path_row[(size_t)l * h + q];
        if (r < 0 || r >= n_rows) continue;
        const int b = last_le(P.blk_row0, P.n_blocks, r);
        if (b < 0 || r >= P.blk_row0[b] + P.blk_rows[b]) continue;
        const int u = last_le(wl.block, wl.n_work, b);
        if (u < 0 || wl.block[u] != b) continue;
        const int k0 = wl.ptr[u], k = last_le(wl.slab + k0, wl.ptr[u + 1] - k0, s);
        if (k < 0 || wl.slab[k0 + k] != s) continue;
        x[((size_t)s * n_rows + r) * 4 + (l & 3)] = path_sign[(size_t)l * h + q];
    }
}

size_t mark_bytes(int64_t n_blocks, int64_t n_slabs, int64_t n_levels) {
    return (size_t)((n_blocks * n_slabs * n_levels + 15) / 16 * 16);
}

}  // namespace

extern "C" {

size_t scn_field_lists_workspace(int32_t n_blocks, int32_t n_slabs, int32_t n_levels) {
    if (n_blocks <= 0 || n_slabs <= 0 || n_levels <= 0) return 0;
    if ((int64_t)n_blocks * n_slabs * n_levels >= INT_MAX / 16) return 0;     // (int32 item counts, one wave per (level, block))
    return mark_bytes(n_blocks, n_slabs, n_levels) + 2 * sizeof(int32_t) * (size_t)n_blocks * n_levels;
}

int scn_field_lists(int32_t n, int32_t ns, const int32_t* node, int32_t n_nodes, const int32_t* top_ptr, const int32_t* top_blk,
                    int32_t n_blocks, const int32_t* adj_ptr, const int32_t* adj_blk, int32_t n_levels, int32_t* block, int32_t* ptr,
                    int32_t* slab, int64_t cap, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (n < 0 || ns <= 0 || n_nodes <= 0 || n_blocks <= 0 || n_levels <= 0 || cap < 0) return SCN_ERR_BAD_SHAPE;
    if ((n > 0 && !node) || !top_ptr || !top_blk || !adj_ptr || !adj_blk || !block || !ptr || (!slab && cap > 0) || !counts || !workspace)
        return SCN_ERR_BAD_ARG;
    const int n_slabs = n > 0 ? (n + ns - 1) / ns : 1;
    const size_t need = scn_field_lists_workspace(n_blocks, n_slabs, n_levels);
    if (need == 0) return SCN_ERR_UNSUPPORTED;
    if (workspace_bytes < need) return SCN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t level_marks = (size_t)n_blocks * n_slabs;
    uint8_t* mark = static_cast<uint8_t*>(workspace);
    int32_t* cnt = reinterpret_cast<int32_t*>(mark + mark_bytes(n_blocks, n_slabs, n_levels));
    int32_t* off = cnt + (size_t)n_blocks * n_levels;
    SCN_HIP_TRY(hipMemsetAsync(mark, 0, level_marks * n_levels, st));
    if (n > 0) {
        hipLaunchKernelGGL(field_mark_kernel, dim3((unsigned)((n + FL_THREADS - 1) / FL_THREADS)), dim3(FL_THREADS), 0, st, n, ns, node,
                           n_nodes, top_ptr, top_blk, n_blocks, n_slabs, mark + level_marks * (n_levels - 1));
        SCN_LAUNCH_CHECK();
        const unsigned hop_grid = (unsigned)((level_marks + FL_THREADS - 1) / FL_THREADS);
        for (int l = n_levels - 2; l >= 0; --l) {
            hipLaunchKernelGGL(field_hop_kernel, dim3(hop_grid), dim3(FL_THREADS), 0, st, n_blocks, n_slabs, adj_ptr, adj_blk,
                               mark + level_marks * (l + 1), mark + level_marks * l);
            SCN_LAUNCH_CHECK();
        }
    }
    const int n_items = n_blocks * n_levels;
    const unsigned wave_grid = (unsigned)(((int64_t)n_items * 64 + FL_THREADS - 1) / FL_THREADS);
    hipLaunchKernelGGL(field_count_kernel, dim3(wave_grid), dim3(FL_THREADS), 0, st, n_items, n_slabs, mark, cnt);
    SCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(field_scan_kernel, dim3((unsigned)n_levels), dim3(FL_SCAN), 0, st, n_blocks, cap, cnt, off, block, ptr, counts);
    SCN_LAUNCH_CHECK();
    if (n > 0 && cap > 0) {
        hipLaunchKernelGGL(field_fill_kernel, dim3(wave_grid), dim3(FL_THREADS), 0, st, n_items, n_blocks, n_slabs, cap, mark, cnt, off,
                           counts, slab);
        SCN_LAUNCH_CHECK();
    }
    return SCN_OK;
}

int scn_tree_slabs_list(scn_conv_t c, int32_t n_leaves, int32_t n_slabs, int32_t h, const int32_t* root, const int32_t* path_row,
                        const float* path_sign, int32_t n_roots, const float* root_x, int32_t n_rows, int32_t ns, float* x,
                        const scn_work_list* wl, void* stream) {
    if (!c || !wl || wl->n_work < 0 || !wl->block || !wl->ptr || (!wl->slab && wl->n_work > 0)) return SCN_ERR_BAD_ARG;
    if (n_leaves < 0 || n_slabs <= 0 || h < 0 || n_roots <= 0 || n_rows <= 0) return SCN_ERR_BAD_SHAPE;
    if (ns != 4 || !c->plan.built || n_rows != c->n_rows) return SCN_ERR_UNSUPPORTED;
    if ((int64_t)n_leaves > (int64_t)n_slabs * ns) return SCN_ERR_BAD_SHAPE;
    if (!x || !root_x || (n_leaves > 0 && !root) || (h > 0 && n_leaves > 0 && (!path_row || !path_sign))) return SCN_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(x) & 15) != 0) return SCN_ERR_BAD_ARG;
    if (wl->n_work == 0) return SCN_OK;
    hipStream_t st = (hipStream_t)stream;
    const WorkList list{wl->n_work, wl->block, wl->ptr, wl->slab};
    hipLaunchKernelGGL(tree_copy_list_kernel, dim3((unsigned)(wl->n_work < 4096 ? wl->n_work : 4096)), dim3(FL_THREADS), 0, st,
                       c->plan.dev, list, n_leaves, n_slabs, root, n_roots, root_x, n_rows, x);
    SCN_LAUNCH_CHECK();
    if (h > 0 && n_leaves > 0) {
        hipLaunchKernelGGL(tree_patch_list_kernel, dim3((unsigned)((n_leaves + FL_THREADS - 1) / FL_THREADS)), dim3(FL_THREADS), 0, st,
                           c->plan.dev, list, n_leaves, h, path_row, path_sign, n_rows, x);
        SCN_LAUNCH_CHECK();
    }
    return SCN_OK;
}

}  // extern "C"
