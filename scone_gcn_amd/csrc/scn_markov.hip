// The k-th order Markov baseline (the reference's markov_model.py, MM:9-112) on direct-addressed integer count tables: one launch
// counts every window of every training walk, one launch rolls a whole multi-hop test out.  A walk of `order` nodes is the state
//     s = ((v0 * D + slot(v0, v1)) * D + slot(v1, v2)) ... * D + slot(v_{k-2}, v_{k-1}),
// slot(a, b) = the position of b among the neighbours of a (nbr[a][0 .. deg[a]), ascending, left-aligned); counts[s][j] = how often
// the walk was followed by the neighbour in slot j of its last node.  Nothing is hashed or sorted, every sum is an integer (no float
// atomics), every random choice is the Philox uniform of (seed, row, ...): the same inputs give the same bytes.
#include "scn_internal.h"
#include "scn_markov_common.h"

#include <climits>

namespace {

using scn_markov::Graph;
using scn_markov::smoothed_weight;
using scn_markov::uniform_u24;

constexpr int WAVE = 64;

// The window of a prefix: its last `order` nodes w[0 .. order) and the order - 1 slots between them.  false (and *err lowered to the
// flat position of the first offending pair, or of the node itself at order 1) when a pair is no edge or an id is out of range; false
// without an error for a prefix shorter than `order` (*is_short set).  Every lane of a wave may call it with the same arguments.
__device__ __forceinline__ bool load_window(const Graph& g, const int32_t* __restrict__ ptr, const int32_t* __restrict__ nodes, int i,
                                            int order, int w[SCN_MARKOV_MAX_ORDER], int sl[SCN_MARKOV_MAX_ORDER], int32_t* err,
                                            bool* is_short) {
    const int t0 = ptr[i], len = ptr[i + 1] - t0;
    *is_short = len < order;
    if (len < order) return false;
    const int base = t0 + len - order;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < SCN_MARKOV_MAX_ORDER; ++k) w[k] = k < order ? nodes[base + k] : -1;
    if (order == 1 && !g.has(w[0])) {
        atomicMin(err, base);
        return false;
    }
#pragma unroll
    for (int k = 0; k + 1 < SCN_MARKOV_MAX_ORDER; ++k) {
        sl[k] = 0;
        if (k + 1 < order && ok) {
            sl[k] = g.slot(w[k], w[k + 1]);
            if (sl[k] < 0) {
                atomicMin(err, base + k);
                ok = false;
            }
        }
    }
    return ok;
}

__device__ __forceinline__ size_t window_state(const int w[SCN_MARKOV_MAX_ORDER], const int sl[SCN_MARKOV_MAX_ORDER], int order, int d) {
    size_t s = (size_t)w[0];
#pragma unroll
    for (int k = 0; k + 1 < SCN_MARKOV_MAX_ORDER; ++k)
        if (k + 1 < order) s = s * d + sl[k];
    return s;
}

// One wave per walk.  A pass takes 64 windows: the slots of the 64 + order - 1 pairs they span go to LDS once, then lane l composes
// window l from order - 1 of them and adds one to its (state, next slot).  Longer walks loop.
__global__ __launch_bounds__(WAVE) void markov_count_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ nodes, int order,
                                                            Graph g, int32_t* counts, int32_t* err) {
    __shared__ int s_slot[WAVE + SCN_MARKOV_MAX_ORDER];
    const int p = blockIdx.x, lane = threadIdx.x;
    const int t0 = ptr[p], len = ptr[p + 1] - t0;
    const int n_win = len - order;                                   // windows of the walk (each has a node after it)
    for (int w0 = 0; w0 < n_win; w0 += WAVE) {
        const int nw = min(WAVE, n_win - w0), n_pairs = nw + order - 1;   // pairs w0 .. w0 + n_pairs - 1 <= len - 2
        for (int q = lane; q < n_pairs; q += WAVE) {
            const int t = t0 + w0 + q;
            const int sl = g.slot(nodes[t], nodes[t + 1]);
            if (sl < 0) atomicMin(err, t);
            s_slot[q] = sl;
        }
        __syncthreads();
        if (lane < nw) {
            size_t s = (size_t)(uint32_t)nodes[t0 + w0 + lane];     // in range whenever the window's first pair is an edge
            bool ok = true;
            for (int k = 0; k + 1 < order; ++k) {
                const int sl = s_slot[lane + k];
                ok = ok && sl >= 0;
                s = s * g.d + (sl < 0 ? 0 : sl);
            }
            const int nx = s_slot[lane + order - 1];
            if (ok && nx >= 0) atomicAdd(&counts[s * g.d + nx], 1);  // a window over a bad pair counts nothing
        }
        __syncthreads();
    }
}

// One wave per prefix, all hops: the lanes loop over the slots of the row (neighbourhoods wider than a wave included)
__global__ __launch_bounds__(WAVE) void markov_rollout_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ nodes,
                                                              int order, int hops, uint64_t seed, Graph g,
                                                              const int32_t* __restrict__ counts, int32_t* __restrict__ pred,
                                                              int32_t* __restrict__ n_tied, int32_t* err) {
    const int i = blockIdx.x, lane = threadIdx.x;
    int w[SCN_MARKOV_MAX_ORDER], sl[SCN_MARKOV_MAX_ORDER];
    bool is_short;
    bool live = load_window(g, ptr, nodes, i, order, w, sl, err, &is_short);
    for (int h = 0; h < hops; ++h) {
        int v = -1;
#pragma unroll
        for (int k = 0; k < SCN_MARKOV_MAX_ORDER; ++k)
            if (k == order - 1) v = w[k];
        const int dv = live ? g.live_deg(v) : 0;
        if (dv == 0) {                                               // short or bad prefix, or a node without neighbours: ends here
            for (int q = h + lane; q < hops; q += WAVE) {
                pred[(size_t)i * hops + q] = -1;
                n_tied[(size_t)i * hops + q] = 0;
            }
            return;
        }
        const int32_t* row = counts + window_state(w, sl, order, g.d) * g.d;
        int mx = INT_MIN;
        for (int j = lane; j < dv; j += WAVE) mx = max(mx, row[j]);
        for (int o = WAVE / 2; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, WAVE));
        int m = 0;
        for (int b = 0; b < dv; b += WAVE) m += __popcll(__ballot(b + lane < dv && row[b + lane] == mx));
        const int k = (int)(((uint64_t)uniform_u24(seed, i, 0, h) * (uint64_t)m) >> 24);     // < m
        int pick = -1, run = 0;
        for (int b = 0; b < dv && pick < 0; b += WAVE) {
            const bool is = b + lane < dv && row[b + lane] == mx;
            const unsigned long long mask = __ballot(is);
            const int c = __popcll(mask);
            if (k < run + c) {
                const bool mine = is && __popcll(mask & ((1ull << lane) - 1ull)) == k - run;
                pick = b + __ffsll((long long)__ballot(mine)) - 1;
            }
            run += c;
        }
        const int u = g.nbr[(size_t)v * g.d + pick];
        if (lane == 0) {
            pred[(size_t)i * hops + h] = u;
            n_tied[(size_t)i * hops + h] = m;
        }
        // the window moves on by one node
#pragma unroll
        for (int q = 0; q + 1 < SCN_MARKOV_MAX_ORDER; ++q) {
            if (q + 1 < order) w[q] = w[q + 1];
            if (q + 2 < order) sl[q] = sl[q + 1];
        }
#pragma unroll
        for (int q = 0; q < SCN_MARKOV_MAX_ORDER; ++q) {
            if (q == order - 1) w[q] = u;
            if (q == order - 2) sl[q] = pick;
        }
        live = g.has(u);                                             // a table entry outside the graph ends the walk
    }
}

__global__ __launch_bounds__(256) void markov_two_target_kernel(int n, const int32_t* __restrict__ ptr, const int32_t* __restrict__ nodes,
                                                                int order, uint64_t seed, const int32_t* __restrict__ target, Graph g,
                                                                const int32_t* __restrict__ counts, float* __restrict__ score,
                                                                int32_t* __restrict__ other, int32_t* err, int32_t* err_target) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int w[SCN_MARKOV_MAX_ORDER], sl[SCN_MARKOV_MAX_ORDER];
    bool is_short;
    float sc = 0.f;
    int ot = -1;
    if (load_window(g, ptr, nodes, i, order, w, sl, err, &is_short)) {
        int v = -1;
#pragma unroll
        for (int k = 0; k < SCN_MARKOV_MAX_ORDER; ++k)
            if (k == order - 1) v = w[k];
        const int dv = g.live_deg(v);
        const int t = g.slot(v, target[i]);
        if (t < 0) {
            atomicMin(err_target, i);
        } else if (dv > 1) {
            const int o = (int)(((uint64_t)uniform_u24(seed, i, 1, 0) * (uint64_t)(dv - 1)) >> 24);
            const int j = o + (o >= t ? 1 : 0);
            const int32_t* row = counts + window_state(w, sl, order, g.d) * g.d;
            const int ct = row[t], co = row[j];
            sc = ct == co ? 0.5f : (ct > co ? 1.f : 0.f);
            ot = g.nbr[(size_t)v * g.d + j];
        }
    }
    score[i] = sc;
    other[i] = ot;
}

__global__ __launch_bounds__(WAVE) void markov_probs_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ nodes, int order,
                                                            Graph g, const int32_t* __restrict__ counts, double* __restrict__ probs,
                                                            int32_t* err) {
    const int i = blockIdx.x, lane = threadIdx.x;
    int w[SCN_MARKOV_MAX_ORDER], sl[SCN_MARKOV_MAX_ORDER];
    bool is_short;
    const bool live = load_window(g, ptr, nodes, i, order, w, sl, err, &is_short);
    int v = -1;
#pragma unroll
    for (int k = 0; k < SCN_MARKOV_MAX_ORDER; ++k)
        if (k == order - 1) v = w[k];
    const int dv = live ? g.live_deg(v) : 0;
    const int32_t* row = counts + (live ? window_state(w, sl, order, g.d) * g.d : 0);
    long long sum = 0;
    for (int j = lane; j < dv; j += WAVE) sum += row[j];
    for (int o = WAVE / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o, WAVE);
    for (int j = lane; j < g.d; j += WAVE)
        probs[(size_t)i * g.d + j] = (j < dv && sum > 0) ? (double)row[j] / (double)sum : 0.0;
}

// One wave per path, the walk of markov_count_kernel with a read where counting has an add.  A pass takes 64 node positions q0 ..
// q0 + 63: the slots of the 63 + order pairs q0 - order .. q0 + 62 go to LDS once (s_slot[i] = pair q0 - order + i; -2 where the path
// has no such pair), then lane l finishes the record of position q0 + l from order of them: its window is the pairs q - order .. q - 1
// that exist, the last of them the step the record predicts.  The quotient is smoothed_weight's: the bits of the C expression
// whatever alpha is.
__global__ __launch_bounds__(WAVE) void markov_path_scores_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ nodes,
                                                                  int order, double alpha, Graph g, const int32_t* __restrict__ counts,
                                                                  double* __restrict__ prob, int32_t* __restrict__ rank,
                                                                  int32_t* __restrict__ total, int32_t* err) {
    __shared__ int s_slot[WAVE + SCN_MARKOV_MAX_ORDER];
    const int p = blockIdx.x, lane = threadIdx.x;
    const int t0 = ptr[p], len = ptr[p + 1] - t0;
    for (int q0 = 0; q0 < len; q0 += WAVE) {
        for (int i = lane; i < WAVE - 1 + order; i += WAVE) {
            const int r = q0 - order + i;                            // the pair (r, r + 1) of the path
            int sl = -2;
            if (r >= 0 && r + 1 < len) {
                sl = g.slot(nodes[t0 + r], nodes[t0 + r + 1]);
                if (sl < 0 && r + 1 >= q0) atomicMin(err, t0 + r);   // (the pairs before q0 were the previous pass's)
            }
            s_slot[i] = sl;
        }
        __syncthreads();
        const int q = q0 + lane;
        if (q < len) {
            double pr = 0.0;
            int rk = -1, tot = 0;
            bool ok = q >= 1;
            for (int m = 0; m < order; ++m) ok = ok && s_slot[lane + m] != -1;
            if (ok) {
                const int t = t0 + q, v = nodes[t - 1], j = s_slot[lane + order - 1], dv = g.live_deg(v);
                long long sum = 0;
                int cj = 0, before = j;                              // the all-zero row of a short prefix: every lower slot ties
                if (q >= order) {
                    size_t s = (size_t)(uint32_t)nodes[t - order];
                    for (int m = 0; m + 1 < order; ++m) s = s * g.d + s_slot[lane + m];
                    const int32_t* row = counts + s * g.d;
                    cj = row[j];
                    before = 0;
                    for (int x = 0; x < dv; ++x) {
                        const int c = row[x];
                        sum += c;
                        before += (c > cj || (c == cj && x < j)) ? 1 : 0;
                    }
                }
                pr = smoothed_weight((double)cj, alpha, (double)sum, (double)dv);
                rk = before;
                tot = (int)sum;
            }
            prob[t0 + q] = pr;
            rank[t0 + q] = rk;
            total[t0 + q] = tot;
        }
        __syncthreads();
    }
}

// the checks every entry point shares: shapes, then what is served, before anything is launched
int check_table(int32_t n, int32_t n_nodes, int32_t d, int32_t order) {
    if (n < 0 || n_nodes <= 0 || d <= 0) return SCN_ERR_BAD_SHAPE;
    const int rows = scn_markov_table_rows(n_nodes, d, order);
    return rows < 0 ? rows : SCN_OK;
}

}  // namespace

extern "C" {

int scn_markov_table_rows(int32_t n_nodes, int32_t d, int32_t order) {
    if (n_nodes <= 0 || d <= 0) return SCN_ERR_BAD_SHAPE;
    if (order < 1 || order > SCN_MARKOV_MAX_ORDER) return SCN_ERR_UNSUPPORTED;
    int64_t rows = n_nodes;
    for (int k = 1; k < order; ++k) {
        rows *= d;
        if (rows * d >= INT_MAX) return SCN_ERR_UNSUPPORTED;
    }
    if (rows * d >= INT_MAX) return SCN_ERR_UNSUPPORTED;
    return (int)rows;
}

int scn_markov_count(int32_t n_paths, const int32_t* path_ptr, const int32_t* path_nodes, int32_t order, int32_t n_nodes, int32_t d,
                     const int32_t* nbr, const int32_t* deg, int32_t* counts, int32_t* err, void* stream) {
    const int st = check_table(n_paths, n_nodes, d, order);
    if (st != SCN_OK) return st;
    if (n_paths == 0) return SCN_OK;
    if (!path_ptr || !path_nodes || !nbr || !deg || !counts || !err) return SCN_ERR_BAD_ARG;
    return scn::launch_checked(markov_count_kernel, dim3((unsigned)n_paths), dim3(WAVE), 0, (hipStream_t)stream, path_ptr, path_nodes,
                               order, Graph{nbr, deg, n_nodes, d}, counts, err);
}

int scn_markov_rollout(int32_t n, const int32_t* prefix_ptr, const int32_t* prefix_nodes, int32_t order, int32_t hops, uint64_t seed,
                       int32_t n_nodes, int32_t d, const int32_t* nbr, const int32_t* deg, const int32_t* counts, int32_t* pred,
                       int32_t* n_tied, int32_t* err, void* stream) {
    if (hops <= 0) return SCN_ERR_BAD_SHAPE;
    const int st = check_table(n, n_nodes, d, order);
    if (st != SCN_OK) return st;
    if (n == 0) return SCN_OK;
    if (!prefix_ptr || !prefix_nodes || !nbr || !deg || !counts || !pred || !n_tied || !err) return SCN_ERR_BAD_ARG;
    return scn::launch_checked(markov_rollout_kernel, dim3((unsigned)n), dim3(WAVE), 0, (hipStream_t)stream, prefix_ptr, prefix_nodes,
                               order, hops, seed, Graph{nbr, deg, n_nodes, d}, counts, pred, n_tied, err);
}

int scn_markov_two_target(int32_t n, const int32_t* prefix_ptr, const int32_t* prefix_nodes, int32_t order, uint64_t seed,
                          const int32_t* target, int32_t n_nodes, int32_t d, const int32_t* nbr, const int32_t* deg,
                          const int32_t* counts, float* score, int32_t* other, int32_t* err, int32_t* err_target, void* stream) {
    const int st = check_table(n, n_nodes, d, order);
    if (st != SCN_OK) return st;
    if (n == 0) return SCN_OK;
    if (!prefix_ptr || !prefix_nodes || !target || !nbr || !deg || !counts || !score || !other || !err || !err_target)
        return SCN_ERR_BAD_ARG;
    return scn::launch_checked(markov_two_target_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                               prefix_ptr, prefix_nodes, order, seed, target, Graph{nbr, deg, n_nodes, d}, counts, score, other, err,
                               err_target);
}

int scn_markov_probs(int32_t n, const int32_t* prefix_ptr, const int32_t* prefix_nodes, int32_t order, int32_t n_nodes, int32_t d,
                     const int32_t* nbr, const int32_t* deg, const int32_t* counts, double* probs, int32_t* err, void* stream) {
    const int st = check_table(n, n_nodes, d, order);
    if (st != SCN_OK) return st;
    if (n == 0) return SCN_OK;
    if (!prefix_ptr || !prefix_nodes || !nbr || !deg || !counts || !probs || !err) return SCN_ERR_BAD_ARG;
    return scn::launch_checked(markov_probs_kernel, dim3((unsigned)n), dim3(WAVE), 0, (hipStream_t)stream, prefix_ptr, prefix_nodes, order,
                               Graph{nbr, deg, n_nodes, d}, counts, probs, err);
}

int scn_markov_path_scores(int32_t n_paths, const int32_t* path_ptr, const int32_t* path_nodes, int32_t order, double alpha,
                           int32_t n_nodes, int32_t d, const int32_t* nbr, const int32_t* deg, const int32_t* counts, double* prob,
                           int32_t* rank, int32_t* total, int32_t* err, void* stream) {
    const int st = check_table(n_paths, n_nodes, d, order);
    if (st != SCN_OK) return st;
    if (!(alpha >= 0.0)) return SCN_ERR_BAD_ARG;                     // negative or NaN
    if (n_paths == 0) return SCN_OK;
    if (!path_ptr || !nbr || !deg || !counts || !err) return SCN_ERR_BAD_ARG;
    if (!path_nodes && !prob && !rank && !total) return SCN_OK;      // paths without a node: T == 0, nothing to write
    if (!path_nodes || !prob || !rank || !total) return SCN_ERR_BAD_ARG;
    return scn::launch_checked(markov_path_scores_kernel, dim3((unsigned)n_paths), dim3(WAVE), 0, (hipStream_t)stream, path_ptr,
                               path_nodes, order, alpha, Graph{nbr, deg, n_nodes, d}, counts, prob, rank, total, err);
}

}  // extern "C"
