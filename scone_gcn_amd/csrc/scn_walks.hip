// Synthetic trajectories on the device (the reference's synthetic_data_gen.generate_random_walks, SDG:178-243): many single-source
// shortest-path problems on one sparse graph in one launch, and the assembly of a walk from three of their paths.
//
// scn_sssp_paths: one 256-thread workgroup owns one job at a time in a slot of the caller's workspace (tentative distances, queue
// stamps, two queues) and relaxes its frontier generation by generation.  A tentative distance is the bit pattern of a non-negative
// fp64, which orders like an unsigned 64-bit integer: lowering it is one 64-bit atomicMin, and the fixed point
//     dist[v] = min over neighbours u of fl(dist[u] + w(u, v))
// has one solution whatever order the relaxations ran in.  Predecessors are NOT taken from the relaxation that happened to win: after
// convergence pred[v] is the smallest-index neighbour u with fl(dist[u] + w(u, v)) == dist[v], so the tree and the paths depend on the
// graph alone.  No workgroup waits on another and nothing synchronises across the grid.
#include "scn_internal.h"

namespace {

constexpr int WG = 256, WAVE = 64;
constexpr int SUB = 8;                                         // lanes that share one frontier entry (a Delaunay row has ~6 neighbours)
constexpr unsigned long long INF_BITS = 0x7FF0000000000000ull; // +inf

// one slot: dist u64[n] | stamp i32[n] | queue i32[2][n], rounded up to 16 bytes
__host__ __device__ inline size_t slot_bytes(int64_t n) { return ((size_t)n * 20 + 15) & ~(size_t)15; }

// A distance as the workgroup last left it in the slot.  The slot is lowered by atomics, which act in L2: reads go there too.
__device__ __forceinline__ unsigned long long ld_dist(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct SsspArgs {
    int n_nodes;
    const int32_t* adj_ptr;
    const int32_t* adj;
    const double* adj_w;      // null: unit weights
    int n_jobs;
    const int32_t* source;
    const int32_t* target;
    int n_targets, path_cap;
    int32_t* path;
    int32_t* path_len;
    double* dist_out;         // optional
    double* dist_all;         // optional
    int32_t* pred_all;        // optional
    int32_t* n_gen;           // optional
    unsigned char* ws;
};

__device__ __forceinline__ unsigned long long relaxed_bits(unsigned long long du, const double* adj_w, int k) {
    return (unsigned long long)__double_as_longlong(__longlong_as_double((long long)du) + (adj_w ? adj_w[k] : 1.0));
}

__global__ __launch_bounds__(WG) void sssp_paths_kernel(SsspArgs a) {
    __shared__ int s_cnt[2];
    __shared__ int s_stop;
    __shared__ unsigned long long s_front;                     // the smallest distance written in this generation
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int n = a.n_nodes;
    unsigned char* base = a.ws + (size_t)blockIdx.x * slot_bytes(n);
    unsigned long long* dist = (unsigned long long*)base;
    int32_t* stamp = (int32_t*)(base + (size_t)n * 8);
    int32_t* qs[2] = {stamp + n, stamp + 2 * (size_t)n};
    const bool want_tree = a.dist_all || a.pred_all;
    const int eff_cap = a.path_cap < n ? a.path_cap : n;       // a simple path has at most n nodes

    for (int job = blockIdx.x; job < a.n_jobs; job += gridDim.x) {
        const int src_in = a.source[job];
        const int src = (src_in >= 0 && src_in < n) ? src_in : -1;
        int tg[SCN_SSSP_MAX_TARGETS];
#pragma unroll
        for (int t = 0; t < SCN_SSSP_MAX_TARGETS; ++t) {
            const int v = t < a.n_targets ? a.target[(size_t)job * a.n_targets + t] : -1;
            tg[t] = (v >= 0 && v < n) ? v : -1;
        }
        // the slot's last job leaves nothing behind: distances, stamps and both queue heads start over
        for (int v = tid; v < n; v += WG) {
            dist[v] = INF_BITS;
            stamp[v] = 0;
        }
        if (tid == 0) {
            s_cnt[0] = 0;
            s_cnt[1] = 0;
            s_stop = 0;
        }
        __threadfence();                                       // the plain stores are in L2 before an atomic of another wave meets them
        __syncthreads();
        if (tid == 0 && src >= 0) {
            dist[src] = 0ull;
            stamp[src] = 1;
            qs[1][0] = src;                                    // generation g reads queue g & 1
            s_cnt[1] = 1;
            __threadfence();
        }
        int gen = 0;
        bool capped = false;
        for (;;) {
            __syncthreads();
            const int cur = (gen + 1) & 1;
            int cnt = s_cnt[cur];                              // the exit is decided from LDS words every thread reads after the barrier
            const int stop = s_stop;
            if (cnt == 0 || stop) break;
            if (gen == n) {                                    // no shortest path has more hops
                capped = true;
                break;
            }
            ++gen;
            cnt = cnt < n ? cnt : n;
            if (tid == 0) {
                s_cnt[cur ^ 1] = 0;
                s_front = ~0ull;
            }
            __syncthreads();
            const int32_t* q = qs[cur];
            int32_t* qn = qs[cur ^ 1];
            for (int e = tid / SUB; e < cnt; e += WG / SUB) {
                const int u = q[e];
                const unsigned long long du = ld_dist(dist + u);
                const int r1 = a.adj_ptr[u + 1];
                for (int k = a.adj_ptr[u] + (tid % SUB); k < r1; k += SUB) {
                    const int v = a.adj[k];
                    if ((unsigned)v >= (unsigned)n) continue;
                    const unsigned long long nb = relaxed_bits(du, a.adj_w, k);   // a NaN or a negative sum orders above +inf: never taken
                    if (nb >= ld_dist(dist + v)) continue;
                    const unsigned long long old = atomicMin(dist + v, nb);
                    if (nb < old) {
                        atomicMin(&s_front, nb);
                        if (atomicExch(stamp + v, gen + 1) != gen + 1) {          // once per generation
                            const int p = atomicAdd(&s_cnt[cur ^ 1], 1);
                            if (p < n) qn[p] = v;
                        }
                    }
                }
            }
            __syncthreads();
            // Early end when only paths are asked for: every target is reached and nothing still queued can lower a node at or below
            // the farthest target (unit weights: a level is final once reached).  The nodes a walk back visits are final then.
            if (tid == 0 && !want_tree) {
                bool all = true;
                unsigned long long far = 0ull;
#pragma unroll
                for (int t = 0; t < SCN_SSSP_MAX_TARGETS; ++t)
                    if (tg[t] >= 0) {
                        const unsigned long long d = ld_dist(dist + tg[t]);
                        all = all && d != INF_BITS;
                        far = d > far ? d : far;
                    }
                if (all && (!a.adj_w || s_front > far)) s_stop = 1;
            }
        }
        if (tid == 0 && a.n_gen) a.n_gen[job] = gen;

        if (want_tree) {
            for (int v = tid; v < n; v += WG) {
                const unsigned long long dv = ld_dist(dist + v);
                int p = -1;
                if (dv != INF_BITS && v != src) {
                    const int r1 = a.adj_ptr[v + 1];
                    for (int k = a.adj_ptr[v]; k < r1; ++k) {
                        const int u = a.adj[k];
                        if ((unsigned)u >= (unsigned)n) continue;
                        const unsigned long long du = ld_dist(dist + u);
                        if (du != INF_BITS && relaxed_bits(du, a.adj_w, k) == dv) {
                            p = u;
                            break;
                        }
                    }
                }
                if (a.dist_all) a.dist_all[(size_t)job * n + v] = __longlong_as_double((long long)dv);
                if (a.pred_all) a.pred_all[(size_t)job * n + v] = p;
            }
        }

        // One wave per target walks back along the smallest tight neighbours into a queue (both are free now), target first.
        int len = 0;
        if (wave < a.n_targets) {
            const int tgt = tg[wave];
            int32_t* rq = qs[wave];
            if (capped) {
                len = -3;
            } else if (tgt < 0) {
                len = 0;
            } else if (ld_dist(dist + tgt) == INF_BITS) {
                len = -1;
            } else {
                int cur = tgt;
                for (;;) {
                    if (lane == 0) rq[len] = cur;
                    ++len;
                    if (cur == src) break;
                    if (len >= eff_cap) {
                        len = -2;
                        break;
                    }
                    const unsigned long long dv = ld_dist(dist + cur);
                    const int r0 = a.adj_ptr[cur], r1 = a.adj_ptr[cur + 1];
                    int p = -1;
                    for (int b = r0; b < r1 && p < 0; b += WAVE) {
                        const int k = b + lane;
                        int u = -1;
                        bool tight = false;
                        if (k < r1) {
                            u = a.adj[k];
                            if ((unsigned)u < (unsigned)n) {
                                const unsigned long long du = ld_dist(dist + u);
                                tight = du != INF_BITS && relaxed_bits(du, a.adj_w, k) == dv;
                            }
                        }
                        const unsigned long long m = __ballot(tight);
                        if (m) p = __shfl(u, __ffsll((long long)m) - 1, WAVE);   // columns ascend: the first tight lane is the smallest
                    }
                    if (p < 0) {                               // not at a fixed point (cannot happen after convergence)
                        len = -1;
                        break;
                    }
                    cur = p;
                }
            }
        }
        __syncthreads();
        if (wave < a.n_targets) {
            const size_t o = (size_t)job * a.n_targets + wave;
            const int32_t* rq = qs[wave];
            for (int i = lane; i < len; i += WAVE) a.path[o * a.path_cap + i] = rq[len - 1 - i];
            if (lane == 0) {
                a.path_len[o] = len;
                if (a.dist_out)
                    a.dist_out[o] = __longlong_as_double((long long)(tg[wave] >= 0 && !capped ? ld_dist(dist + tg[wave]) : INF_BITS));
            }
        }
        __syncthreads();                                       // the queues are read to here; the next job writes them
    }
}

__device__ __forceinline__ unsigned hash_id(int v) {
    unsigned x = (unsigned)v * 0x9E3779B1u;
    return x ^ (x >> 15);
}

// One workgroup per attempt: job 2 a = (v_1 -> v_begin, v_1 -> v_2), job 2 a + 1 = (v_2 -> v_end, none).
__global__ __launch_bounds__(WG) void walk_assemble_kernel(const int32_t* __restrict__ path, const int32_t* __restrict__ path_len, int path_cap,
                                                           int32_t* __restrict__ walk, int32_t* __restrict__ walk_len, int walk_cap,
                                                           int tab_mask) {
    extern __shared__ int32_t s_tab[];                         // open-addressed set of the walk's ids, tab_mask + 1 >= 2 walk_cap entries
    __shared__ int s_dup;
    const int a = blockIdx.x, tid = threadIdx.x;
    const int la = path_len[(size_t)a * 4], lb = path_len[(size_t)a * 4 + 1], lc = path_len[(size_t)a * 4 + 2];
    int len = 0;
    if (la > 0 && lb > 0 && lc > 0 && la <= path_cap && lb <= path_cap && lc <= path_cap) {
        const long long L = (long long)la + lb + lc - 2;
        if (L <= walk_cap) len = (int)L;
    }
    if (len == 0) {                                            // uniform: every thread read the same three lengths
        if (tid == 0) walk_len[a] = 0;
        return;
    }
    for (int i = tid; i <= tab_mask; i += WG) s_tab[i] = -1;
    if (tid == 0) s_dup = 0;
    __syncthreads();
    const int32_t* pa = path + (size_t)a * 4 * path_cap;
    const int32_t* pb = pa + path_cap;
    const int32_t* pc = pa + 2 * (size_t)path_cap;
    int32_t* w = walk + (size_t)a * walk_cap;
    for (int i = tid; i < len; i += WG) {
        int v;
        if (i < la - 1) v = pa[la - 1 - i];                    // reverse(path(v_1 -> v_begin))[:-1]
        else if (i < la + lb - 2) v = pb[i - (la - 1)];        // path(v_1 -> v_2)[:-1]
        else v = pc[i - (la + lb - 2)];                        // path(v_2 -> v_end)
        w[i] = v;
        unsigned h = hash_id(v) & (unsigned)tab_mask;
        for (int probe = 0; probe <= tab_mask; ++probe) {
            const int old = atomicCAS(&s_tab[h], -1, v);
            if (old == -1) break;
            if (old == v) {
                s_dup = 1;
                break;
            }
            h = (h + 1) & (unsigned)tab_mask;
        }
    }
    __syncthreads();
    if (tid == 0) walk_len[a] = s_dup ? 0 : len;
}

}  // namespace

extern "C" {

size_t scn_sssp_slot_bytes(int32_t n_nodes) { return n_nodes > 0 ? slot_bytes(n_nodes) : 0; }

int scn_sssp_paths(int32_t n_nodes, const int32_t* adj_ptr, const int32_t* adj, const double* adj_w, int32_t n_jobs, const int32_t* source,
                   const int32_t* target, int32_t n_targets, int32_t path_cap, int32_t* path, int32_t* path_len, double* dist_out,
                   double* dist_all, int32_t* pred_all, int32_t* n_gen, void* workspace, size_t workspace_bytes, int32_t n_slots,
                   void* stream) {
    if (n_nodes <= 0 || n_jobs < 0) return SCN_ERR_BAD_SHAPE;
    if (n_targets < 1 || n_targets > SCN_SSSP_MAX_TARGETS || path_cap < 1 || n_slots < 1) return SCN_ERR_BAD_ARG;
    if (n_jobs == 0) return SCN_OK;
    if (!adj_ptr || !adj || !source || !target || !path || !path_len || !workspace) return SCN_ERR_BAD_ARG;
    if (((uintptr_t)workspace & 7u) != 0) return SCN_ERR_BAD_ARG;
    if (workspace_bytes / slot_bytes(n_nodes) < (size_t)n_slots) return SCN_ERR_WORKSPACE;
    const int grid = n_jobs < n_slots ? n_jobs : n_slots;
    SsspArgs a{n_nodes, adj_ptr, adj, adj_w, n_jobs, source, target, n_targets, path_cap, path, path_len, dist_out, dist_all, pred_all,
               n_gen, (unsigned char*)workspace};
    return scn::launch_checked(sssp_paths_kernel, dim3((unsigned)grid), dim3(WG), 0, (hipStream_t)stream, a);
}

int scn_walk_assemble(int32_t n, const int32_t* path, const int32_t* path_len, int32_t path_cap, int32_t* walk, int32_t* walk_len,
                      int32_t walk_cap, void* stream) {
    if (n < 0) return SCN_ERR_BAD_SHAPE;
    if (path_cap < 1 || walk_cap < 1) return SCN_ERR_BAD_ARG;
    if (walk_cap > SCN_WALK_MAX) return SCN_ERR_UNSUPPORTED;
    if (n == 0) return SCN_OK;
    if (!path || !path_len || !walk || !walk_len) return SCN_ERR_BAD_ARG;
    int tab = 64;
    while (tab < 2 * walk_cap) tab *= 2;
    return scn::launch_checked(walk_assemble_kernel, dim3((unsigned)n), dim3(WG), (size_t)tab * sizeof(int32_t), (hipStream_t)stream, path,
                               path_len, path_cap, walk, walk_len, walk_cap, tab - 1);
}

}  // extern "C"
