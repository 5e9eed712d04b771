// The variable-order Markov baseline: the count rows of every order 1 .. K of scn_markov.hip's states in one open-addressed hash
// table, and readers that back off to the longest context the table holds (the PPM rule).  A walk of k nodes is the state s of
// scn_markov.hip; its key is (k - 1) << 59 | s, all-ones the empty slot.  keys[capacity] (capacity a power of two) is probed linearly
// from mix(key); row_of[slot] names the key's row of counts[n_states][d].
//
// The table is built by three launches, none of which waits for another thread: insert claims a slot per distinct key (a 64-bit
// compare-and-swap on a slot that read empty, a step on where the slot holds another key -- a claimed slot never changes again, so
// nothing is ever re-read until it changes), number gives every claimed slot a row, count looks the keys up and adds.  Every loop is
// bounded by the capacity.  Row numbers depend on the order the atomics land in; no output of a reader does.
#include "scn_internal.h"
#include "scn_markov_common.h"

#include <climits>

namespace {

using scn_markov::Graph;
using scn_markov::smoothed_weight;
using scn_markov::uniform_u24;

constexpr int WAVE = 64;
constexpr int MAXO = SCN_MARKOV_HASH_MAX_ORDER;
constexpr uint64_t EMPTY = ~0ull;
constexpr int KEY_SHIFT = 59;

__device__ __forceinline__ uint64_t make_key(int k, uint64_t s) { return ((uint64_t)(k - 1) << KEY_SHIFT) | s; }

// the finaliser of splitmix64
__device__ __forceinline__ uint64_t mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

struct Table {
    const uint64_t* keys;      // [capacity]
    const int32_t* row_of;     // [capacity]
    const int32_t* counts;     // [n_states][d]
    uint64_t capacity;
    // the row of key, -1 when the table does not hold it: at most `capacity` slots are read
    __device__ __forceinline__ int row(uint64_t key) const {
        uint64_t h = mix(key) & (capacity - 1);
        for (uint64_t probe = 0; probe < capacity; ++probe) {
            const uint64_t at = keys[h];
            if (at == key) return row_of[h];
            if (at == EMPTY) return -1;
            h = (h + 1) & (capacity - 1);
        }
        return -1;
    }
};

// ---- the build ----

// One wave per walk, 64 window starts a pass (markov_count_kernel's walk): the slots of the pairs the pass spans go to LDS once, then
// lane l grows the window that starts at node w0 + l order by order and hands fn(k, state, next slot) every window of k nodes that has
// a node after it and no offending pair in or behind it.
template <class Fn>
__device__ __forceinline__ void for_each_window(const int32_t* __restrict__ ptr, const int32_t* __restrict__ nodes, int max_order,
                                                const Graph& g, int32_t* err, int* s_slot, Fn fn) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int t0 = ptr[p], len = ptr[p + 1] - t0;
    const int n_pairs_all = len - 1;                                 // pair q is (node q, node q + 1); a window starts at every q
    for (int w0 = 0; w0 < n_pairs_all; w0 += WAVE) {
        const int nw = min(WAVE, n_pairs_all - w0), n_pairs = min(nw + max_order - 1, n_pairs_all - w0);
        for (int q = lane; q < n_pairs; q += WAVE) {
            const int t = t0 + w0 + q;
            const int sl = g.slot(nodes[t], nodes[t + 1]);
            if (sl < 0) atomicMin(err, t);
            s_slot[q] = sl;
        }
        __syncthreads();
        if (lane < nw) {
            uint64_t s = (uint64_t)(uint32_t)nodes[t0 + w0 + lane];  // in range whenever the window's first pair is an edge
            for (int k = 1; k <= max_order && lane + k - 1 < n_pairs; ++k) {
                const int nx = s_slot[lane + k - 1];
                if (nx < 0) break;                                   // every longer window holds the pair too
                fn(k, s, nx);
                s = s * (uint64_t)g.d + (uint64_t)nx;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(WAVE) void hash_insert_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ nodes,
                                                           int max_order, Graph g, unsigned long long* keys, uint64_t capacity,
                                                           int32_t* err, int32_t* overflow) {
    __shared__ int s_slot[WAVE + MAXO];
    const int p = blockIdx.x;
    for_each_window(ptr, nodes, max_order, g, err, s_slot, [&](int k, uint64_t s, int) {
        const uint64_t key = make_key(k, s);
        uint64_t h = mix(key) & (capacity - 1);
        for (uint64_t probe = 0; probe < capacity; ++probe) {
            uint64_t at = keys[h];                                   // a slot that holds a key keeps it: no need to ask again
            if (at == EMPTY) at = atomicCAS(&keys[h], (unsigned long long)EMPTY, (unsigned long long)key);
            if (at == EMPTY || at == key) return;
            h = (h + 1) & (capacity - 1);
        }
        atomicMin(overflow, p);                                      // every slot holds another key
    });
}

__global__ __launch_bounds__(256) void hash_number_kernel(const uint64_t* __restrict__ keys, uint64_t capacity, int max_order,
                                                          int32_t* __restrict__ row_of, int32_t* n_states,
                                                          int32_t* n_states_per_order) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= capacity) return;
    const uint64_t key = keys[i];
    int row = -1;
    if (key != EMPTY) {
        row = atomicAdd(n_states, 1);
        const int k = (int)(key >> KEY_SHIFT);                       // order - 1 < max_order for every key insert wrote
        if (k < max_order) atomicAdd(&n_states_per_order[k], 1);
    }
    row_of[i] = row;
}

__global__ __launch_bounds__(WAVE) void hash_count_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ nodes,
                                                          int max_order, Graph g, Table tab, int32_t n_states, int32_t* counts,
                                                          int32_t* err) {
    __shared__ int s_slot[WAVE + MAXO];
    for_each_window(ptr, nodes, max_order, g, err, s_slot, [&](int k, uint64_t s, int nx) {
        const int row = tab.row(make_key(k, s));
        if (row >= 0 && row < n_states) atomicAdd(&counts[(size_t)row * g.d + nx], 1);
    });
}

// ---- the readers ----

// The last nodes of a prefix, right-aligned: w[MAXO - 1] is the last node, sl[q] = slot(w[q], w[q + 1]); m of them are held.
struct Context {
    int w[MAXO], sl[MAXO];
    int m;
    // the state of the last k <= m nodes
    __device__ __forceinline__ uint64_t state(int k, int d) const {
        uint64_t s = 0;
#pragma unroll
        for (int q = 0; q < MAXO; ++q) {
            if (q == MAXO - k) s = (uint64_t)(uint32_t)w[q];
            else if (q > MAXO - k) s = s * (uint64_t)d + (uint64_t)sl[q - 1];
        }
        return s;
    }
    __device__ __forceinline__ void push(int u, int pick, int max_order) {
#pragma unroll
        for (int q = 0; q + 1 < MAXO; ++q) {
            w[q] = w[q + 1];
            sl[q] = sl[q + 1];
        }
        w[MAXO - 1] = u;
        sl[MAXO - 2] = pick;
        m = min(m + 1, max_order);
    }
};

// The last min(len, max_order) nodes of prefix i.  false for an empty prefix, for a prefix shorter than max_order without back-off
// (neither is an error) and for a pair that is no edge or an id outside the graph, which lowers *err to the flat position of the
// first such pair (of the node itself for a window of one node).  Every lane of a wave may call it with the same arguments.
__device__ __forceinline__ bool load_context(const Graph& g, const int32_t* __restrict__ ptr, const int32_t* __restrict__ nodes, int i,
                                             int max_order, int backoff, Context& c, int32_t* err) {
    const int t0 = ptr[i], len = ptr[i + 1] - t0;
    const int m = min(len, max_order);
    c.m = m;
#pragma unroll
    for (int q = 0; q < MAXO; ++q) {
        c.w[q] = -1;
        c.sl[q] = 0;
    }
    if (m == 0 || (!backoff && len < max_order)) return false;
    const int base = t0 + len - m;
#pragma unroll
    for (int q = 0; q < MAXO; ++q)
        if (q >= MAXO - m) c.w[q] = nodes[base + q - (MAXO - m)];
    if (m == 1 && !g.has(c.w[MAXO - 1])) {
        atomicMin(err, base);
        return false;
    }
    bool ok = true;
#pragma unroll
    for (int q = 0; q + 1 < MAXO; ++q) {
        if (q >= MAXO - m && ok) {
            c.sl[q] = g.slot(c.w[q], c.w[q + 1]);
            if (c.sl[q] < 0) {
                atomicMin(err, base + q - (MAXO - m));
                c.sl[q] = 0;
                ok = false;
            }
        }
    }
    return ok;
}

// the orders a context of m nodes tries, longest first: k_hi down to k_lo (none when k_hi < k_lo)
__device__ __forceinline__ void order_range(int m, int max_order, int backoff, int* k_hi, int* k_lo) {
    *k_hi = min(m, max_order);
    *k_lo = backoff ? 1 : max_order;
}

// One lane's choice: the longest order whose state is in the table with a row total >= min_count over the dv slots; 0 and row -1
// when there is none.
__device__ __forceinline__ int choose_order_lane(const Context& c, const Table& tab, int max_order, int backoff, int min_count, int d,
                                                 int dv, int* row_out, long long* sum_out) {
    int k_hi, k_lo;
    order_range(c.m, max_order, backoff, &k_hi, &k_lo);
    for (int k = k_hi; k >= k_lo; --k) {
        const int row = tab.row(make_key(k, c.state(k, d)));
        if (row < 0) continue;
        const int32_t* r = tab.counts + (size_t)row * d;
        long long sum = 0;
        for (int j = 0; j < dv; ++j) sum += r[j];
        if (sum >= min_count) {
            *row_out = row;
            *sum_out = sum;
            return k;
        }
    }
    *row_out = -1;
    *sum_out = 0;
    return 0;
}

// The same for a whole wave: one key, every lane; the lanes share the row's sum.
__device__ __forceinline__ int choose_order_wave(const Context& c, const Table& tab, int max_order, int backoff, int min_count, int d,
                                                 int dv, int lane, int* row_out, long long* sum_out) {
    int k_hi, k_lo;
    order_range(c.m, max_order, backoff, &k_hi, &k_lo);
    for (int k = k_hi; k >= k_lo; --k) {
        const int row = tab.row(make_key(k, c.state(k, d)));
        if (row < 0) continue;
        const int32_t* r = tab.counts + (size_t)row * d;
        long long sum = 0;
        for (int j = lane; j < dv; j += WAVE) sum += r[j];
        for (int o = WAVE / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o, WAVE);
        if (sum >= min_count) {
            *row_out = row;
            *sum_out = sum;
            return k;
        }
    }
    *row_out = -1;
    *sum_out = 0;
    return 0;
}

// One wave per prefix, all hops (markov_rollout_kernel with the order chosen anew at every hop)
__global__ __launch_bounds__(WAVE) void hash_rollout_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ nodes,
                                                            int max_order, int backoff, int min_count, int hops, uint64_t seed, Graph g,
                                                            Table tab, int32_t* __restrict__ pred, int32_t* __restrict__ n_tied,
                                                            int32_t* __restrict__ used_order, int32_t* err) {
    const int i = blockIdx.x, lane = threadIdx.x;
    Context c;
    bool live = load_context(g, ptr, nodes, i, max_order, backoff, c, err);
    for (int h = 0; h < hops; ++h) {
        const int v = c.w[MAXO - 1];
        const int dv = live ? g.live_deg(v) : 0;
        if (dv == 0) {                                               // no context, an offending one, or a node without neighbours
            for (int q = h + lane; q < hops; q += WAVE) {
                pred[(size_t)i * hops + q] = -1;
                n_tied[(size_t)i * hops + q] = 0;
                used_order[(size_t)i * hops + q] = 0;
            }
            return;
        }
        int r;
        long long sum;
        const int used = choose_order_wave(c, tab, max_order, backoff, min_count, g.d, dv, lane, &r, &sum);
        const int32_t* row = tab.counts + (size_t)(r < 0 ? 0 : r) * g.d;
        const bool none = r < 0;                                     // the all-zero row: every neighbour ties
        int mx = INT_MIN;
        for (int j = lane; j < dv; j += WAVE) mx = max(mx, none ? 0 : row[j]);
        for (int o = WAVE / 2; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, WAVE));
        int m = 0;
        for (int b = 0; b < dv; b += WAVE) m += __popcll(__ballot(b + lane < dv && (none ? 0 : row[b + lane]) == mx));
        const int k = (int)(((uint64_t)uniform_u24(seed, i, 0, h) * (uint64_t)m) >> 24);     // < m
        int pick = -1, run = 0;
        for (int b = 0; b < dv && pick < 0; b += WAVE) {
            const bool is = b + lane < dv && (none ? 0 : row[b + lane]) == mx;
            const unsigned long long mask = __ballot(is);
            const int cnt = __popcll(mask);
            if (k < run + cnt) {
                const bool mine = is && __popcll(mask & ((1ull << lane) - 1ull)) == k - run;
                pick = b + __ffsll((long long)__ballot(mine)) - 1;
            }
            run += cnt;
        }
        const int u = g.nbr[(size_t)v * g.d + pick];
        if (lane == 0) {
            pred[(size_t)i * hops + h] = u;
            n_tied[(size_t)i * hops + h] = m;
            used_order[(size_t)i * hops + h] = used;
        }
        c.push(u, pick, max_order);
        live = g.has(u);                                             // a table entry outside the graph ends the walk
    }
}

__global__ __launch_bounds__(256) void hash_two_target_kernel(int n, const int32_t* __restrict__ ptr, const int32_t* __restrict__ nodes,
                                                              int max_order, int backoff, int min_count, uint64_t seed,
                                                              const int32_t* __restrict__ target, Graph g, Table tab,
                                                              float* __restrict__ score, int32_t* __restrict__ other,
                                                              int32_t* __restrict__ used_order, int32_t* err, int32_t* err_target) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Context c;
    float sc = 0.f;
    int ot = -1, used = 0;
    if (load_context(g, ptr, nodes, i, max_order, backoff, c, err)) {
        const int v = c.w[MAXO - 1];
        const int dv = g.live_deg(v);
        const int t = g.slot(v, target[i]);
        if (t < 0) {
            atomicMin(err_target, i);
        } else if (dv > 1) {
            const int o = (int)(((uint64_t)uniform_u24(seed, i, 1, 0) * (uint64_t)(dv - 1)) >> 24);
            const int j = o + (o >= t ? 1 : 0);
            int r;
            long long sum;
            used = choose_order_lane(c, tab, max_order, backoff, min_count, g.d, dv, &r, &sum);
            const int32_t* row = tab.counts + (size_t)(r < 0 ? 0 : r) * g.d;
            const int ct = r < 0 ? 0 : row[t], co = r < 0 ? 0 : row[j];
            sc = ct == co ? 0.5f : (ct > co ? 1.f : 0.f);
            ot = g.nbr[(size_t)v * g.d + j];
        }
    }
    score[i] = sc;
    other[i] = ot;
    used_order[i] = used;
}

__global__ __launch_bounds__(WAVE) void hash_probs_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ nodes,
                                                          int max_order, int backoff, int min_count, Graph g, Table tab,
                                                          double* __restrict__ probs, int32_t* __restrict__ used_order, int32_t* err) {
    const int i = blockIdx.x, lane = threadIdx.x;
    Context c;
    const bool live = load_context(g, ptr, nodes, i, max_order, backoff, c, err);
    const int dv = live ? g.live_deg(c.w[MAXO - 1]) : 0;
    int r = -1, used = 0;
    long long sum = 0;
    if (dv > 0) used = choose_order_wave(c, tab, max_order, backoff, min_count, g.d, dv, lane, &r, &sum);
    const int32_t* row = tab.counts + (size_t)(r < 0 ? 0 : r) * g.d;
    for (int j = lane; j < g.d; j += WAVE)
        probs[(size_t)i * g.d + j] = (j < dv && r >= 0 && sum > 0) ? (double)row[j] / (double)sum : 0.0;
    if (lane == 0) used_order[i] = used;
}

// One wave per path, markov_path_scores_kernel's passes: s_slot[i] = the slot of pair q0 - K + i (-2 where the path has no such pair),
// lane l finishes the record of position q0 + l, looking its own keys up longest first.
__global__ __launch_bounds__(WAVE) void hash_path_scores_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ nodes,
                                                                int max_order, int backoff, int min_count, double alpha, Graph g,
                                                                Table tab, double* __restrict__ prob, int32_t* __restrict__ rank,
                                                                int32_t* __restrict__ total, int32_t* __restrict__ used_order,
                                                                int32_t* err) {
    __shared__ int s_slot[WAVE + MAXO];
    const int p = blockIdx.x, lane = threadIdx.x, K = max_order;
    const int t0 = ptr[p], len = ptr[p + 1] - t0;
    for (int q0 = 0; q0 < len; q0 += WAVE) {
        for (int i = lane; i < WAVE - 1 + K; i += WAVE) {
            const int r = q0 - K + i;                                // the pair (r, r + 1) of the path
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
            int rk = -1, tot = 0, used = 0;
            bool ok = q >= 1;
            for (int m = 0; m < K; ++m) ok = ok && s_slot[lane + m] != -1;
            if (ok) {
                const int t = t0 + q, v = nodes[t - 1], j = s_slot[lane + K - 1], dv = g.live_deg(v);
                long long sum = 0;
                int cj = 0, before = j;                              // the all-zero row: every lower slot ties
                const int k_hi = min(q, K), k_lo = backoff ? 1 : K;
                for (int k = k_hi; k >= k_lo && used == 0; --k) {
                    uint64_t s = (uint64_t)(uint32_t)nodes[t - k];
                    for (int m = 0; m + 1 < k; ++m) s = s * (uint64_t)g.d + (uint64_t)s_slot[lane + K - k + m];
                    const int r = tab.row(make_key(k, s));
                    if (r < 0) continue;
                    const int32_t* row = tab.counts + (size_t)r * g.d;
                    long long rs = 0;
                    for (int x = 0; x < dv; ++x) rs += row[x];
                    if (rs < min_count) continue;
                    used = k;
                    sum = rs;
                    cj = row[j];
                    before = 0;
                    for (int x = 0; x < dv; ++x) {
                        const int cx = row[x];
                        before += (cx > cj || (cx == cj && x < j)) ? 1 : 0;
                    }
                }
                pr = smoothed_weight((double)cj, alpha, (double)sum, (double)dv);
                rk = before;
                tot = (int)sum;
            }
            prob[t0 + q] = pr;
            rank[t0 + q] = rk;
            total[t0 + q] = tot;
            used_order[t0 + q] = used;
        }
        __syncthreads();
    }
}

int check_reader(int32_t n, int32_t n_nodes, int32_t d, int32_t max_order, int64_t capacity, int32_t backoff, int32_t min_count) {
    if (n < 0) return SCN_ERR_BAD_SHAPE;
    const int st = scn_markov_hash_check(n_nodes, d, max_order, capacity);
    if (st != SCN_OK) return st;
    if ((backoff != 0 && backoff != 1) || min_count < 1) return SCN_ERR_BAD_ARG;
    return SCN_OK;
}

}  // namespace

extern "C" {

int scn_markov_hash_check(int32_t n_nodes, int32_t d, int32_t max_order, int64_t capacity) {
    if (n_nodes <= 0 || d <= 0) return SCN_ERR_BAD_SHAPE;
    if (max_order < 1 || max_order > SCN_MARKOV_HASH_MAX_ORDER) return SCN_ERR_UNSUPPORTED;
    const uint64_t limit = 1ull << KEY_SHIFT;
    uint64_t states = (uint64_t)n_nodes;                             // < 2^31 < limit
    for (int k = 1; k < max_order; ++k) {
        if (states > (limit - 1) / (uint64_t)d) return SCN_ERR_UNSUPPORTED;      // states * d >= limit, asked before the product can wrap
        states *= (uint64_t)d;
    }
    if (capacity < 1 || (capacity & (capacity - 1)) != 0) return SCN_ERR_BAD_ARG;
    return SCN_OK;
}

int scn_markov_hash_insert(int32_t n_paths, const int32_t* path_ptr, const int32_t* path_nodes, int32_t max_order, int32_t n_nodes,
                           int32_t d, const int32_t* nbr, const int32_t* deg, uint64_t* keys, int64_t capacity, int32_t* err,
                           int32_t* overflow, void* stream) {
    if (n_paths < 0) return SCN_ERR_BAD_SHAPE;
    const int st = scn_markov_hash_check(n_nodes, d, max_order, capacity);
    if (st != SCN_OK) return st;
    if (n_paths == 0) return SCN_OK;
    if (!path_ptr || !path_nodes || !nbr || !deg || !keys || !err || !overflow) return SCN_ERR_BAD_ARG;
    return scn::launch_checked(hash_insert_kernel, dim3((unsigned)n_paths), dim3(WAVE), 0, (hipStream_t)stream, path_ptr, path_nodes,
                               max_order, Graph{nbr, deg, n_nodes, d}, (unsigned long long*)keys, (uint64_t)capacity, err, overflow);
}

int scn_markov_hash_number(const uint64_t* keys, int64_t capacity, int32_t max_order, int32_t* row_of, int32_t* n_states,
                           int32_t* n_states_per_order, void* stream) {
    const int st = scn_markov_hash_check(1, 1, max_order, capacity);
    if (st != SCN_OK) return st;
    if (capacity > (int64_t)INT_MAX) return SCN_ERR_UNSUPPORTED;     // a row number is an int32
    if (!keys || !row_of || !n_states || !n_states_per_order) return SCN_ERR_BAD_ARG;
    return scn::launch_checked(hash_number_kernel, dim3((unsigned)((capacity + 255) / 256)), dim3(256), 0, (hipStream_t)stream, keys,
                               (uint64_t)capacity, max_order, row_of, n_states, n_states_per_order);
}

int scn_markov_hash_count(int32_t n_paths, const int32_t* path_ptr, const int32_t* path_nodes, int32_t max_order, int32_t n_nodes,
                          int32_t d, const int32_t* nbr, const int32_t* deg, const uint64_t* keys, const int32_t* row_of,
                          int64_t capacity, int32_t n_states, int32_t* counts, int32_t* err, void* stream) {
    if (n_paths < 0 || n_states < 0) return SCN_ERR_BAD_SHAPE;
    const int st = scn_markov_hash_check(n_nodes, d, max_order, capacity);
    if (st != SCN_OK) return st;
    if (n_paths == 0 || n_states == 0) return SCN_OK;
    if (!path_ptr || !path_nodes || !nbr || !deg || !keys || !row_of || !counts || !err) return SCN_ERR_BAD_ARG;
    return scn::launch_checked(hash_count_kernel, dim3((unsigned)n_paths), dim3(WAVE), 0, (hipStream_t)stream, path_ptr, path_nodes,
                               max_order, Graph{nbr, deg, n_nodes, d}, Table{keys, row_of, counts, (uint64_t)capacity}, n_states, counts,
                               err);
}

int scn_markov_hash_rollout(int32_t n, const int32_t* prefix_ptr, const int32_t* prefix_nodes, int32_t max_order, int32_t backoff,
                            int32_t min_count, int32_t hops, uint64_t seed, int32_t n_nodes, int32_t d, const int32_t* nbr,
                            const int32_t* deg, const uint64_t* keys, const int32_t* row_of, int64_t capacity, const int32_t* counts,
                            int32_t* pred, int32_t* n_tied, int32_t* used_order, int32_t* err, void* stream) {
    if (hops <= 0) return SCN_ERR_BAD_SHAPE;
    const int st = check_reader(n, n_nodes, d, max_order, capacity, backoff, min_count);
    if (st != SCN_OK) return st;
    if (n == 0) return SCN_OK;
    if (!prefix_ptr || !prefix_nodes || !nbr || !deg || !keys || !row_of || !counts || !pred || !n_tied || !used_order || !err)
        return SCN_ERR_BAD_ARG;
    return scn::launch_checked(hash_rollout_kernel, dim3((unsigned)n), dim3(WAVE), 0, (hipStream_t)stream, prefix_ptr, prefix_nodes,
                               max_order, backoff, min_count, hops, seed, Graph{nbr, deg, n_nodes, d},
                               Table{keys, row_of, counts, (uint64_t)capacity}, pred, n_tied, used_order, err);
}

int scn_markov_hash_two_target(int32_t n, const int32_t* prefix_ptr, const int32_t* prefix_nodes, int32_t max_order, int32_t backoff,
                               int32_t min_count, uint64_t seed, const int32_t* target, int32_t n_nodes, int32_t d, const int32_t* nbr,
                               const int32_t* deg, const uint64_t* keys, const int32_t* row_of, int64_t capacity, const int32_t* counts,
                               float* score, int32_t* other, int32_t* used_order, int32_t* err, int32_t* err_target, void* stream) {
    const int st = check_reader(n, n_nodes, d, max_order, capacity, backoff, min_count);
    if (st != SCN_OK) return st;
    if (n == 0) return SCN_OK;
    if (!prefix_ptr || !prefix_nodes || !target || !nbr || !deg || !keys || !row_of || !counts || !score || !other || !used_order ||
        !err || !err_target)
        return SCN_ERR_BAD_ARG;
    return scn::launch_checked(hash_two_target_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                               prefix_ptr, prefix_nodes, max_order, backoff, min_count, seed, target, Graph{nbr, deg, n_nodes, d},
                               Table{keys, row_of, counts, (uint64_t)capacity}, score, other, used_order, err, err_target);
}

int scn_markov_hash_probs(int32_t n, const int32_t* prefix_ptr, const int32_t* prefix_nodes, int32_t max_order, int32_t backoff,
                          int32_t min_count, int32_t n_nodes, int32_t d, const int32_t* nbr, const int32_t* deg, const uint64_t* keys,
                          const int32_t* row_of, int64_t capacity, const int32_t* counts, double* probs, int32_t* used_order,
                          int32_t* err, void* stream) {
    const int st = check_reader(n, n_nodes, d, max_order, capacity, backoff, min_count);
    if (st != SCN_OK) return st;
    if (n == 0) return SCN_OK;
    if (!prefix_ptr || !prefix_nodes || !nbr || !deg || !keys || !row_of || !counts || !probs || !used_order || !err)
        return SCN_ERR_BAD_ARG;
    return scn::launch_checked(hash_probs_kernel, dim3((unsigned)n), dim3(WAVE), 0, (hipStream_t)stream, prefix_ptr, prefix_nodes,
                               max_order, backoff, min_count, Graph{nbr, deg, n_nodes, d},
                               Table{keys, row_of, counts, (uint64_t)capacity}, probs, used_order, err);
}

int scn_markov_hash_path_scores(int32_t n_paths, const int32_t* path_ptr, const int32_t* path_nodes, int32_t max_order, int32_t backoff,
                                int32_t min_count, double alpha, int32_t n_nodes, int32_t d, const int32_t* nbr, const int32_t* deg,
                                const uint64_t* keys, const int32_t* row_of, int64_t capacity, const int32_t* counts, double* prob,
                                int32_t* rank, int32_t* total, int32_t* used_order, int32_t* err, void* stream) {
    const int st = check_reader(n_paths, n_nodes, d, max_order, capacity, backoff, min_count);
    if (st != SCN_OK) return st;
    if (!(alpha >= 0.0)) return SCN_ERR_BAD_ARG;                     // negative or NaN
    if (n_paths == 0) return SCN_OK;
    if (!path_ptr || !nbr || !deg || !keys || !row_of || !counts || !err) return SCN_ERR_BAD_ARG;
    if (!path_nodes && !prob && !rank && !total && !used_order) return SCN_OK;      // paths without a node: nothing to write
    if (!path_nodes || !prob || !rank || !total || !used_order) return SCN_ERR_BAD_ARG;
    return scn::launch_checked(hash_path_scores_kernel, dim3((unsigned)n_paths), dim3(WAVE), 0, (hipStream_t)stream, path_ptr,
                               path_nodes, max_order, backoff, min_count, alpha, Graph{nbr, deg, n_nodes, d},
                               Table{keys, row_of, counts, (uint64_t)capacity}, prob, rank, total, used_order, err);
}

}  // extern "C"
