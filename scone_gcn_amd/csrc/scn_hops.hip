// Multi-hop prediction (STM:110-206): the device steps between the forwards of a greedy rollout, of a probability tree or of a beam
// search.  The forwards themselves are the fused layer kernels; these kernels choose the next node, look up the edge it crosses, build
// the child flow slabs, prune a beam and reduce the leaf probabilities per trajectory, so that no level goes through the host.
#include "scn_internal.h"

#include <climits>

namespace {

// np.argmax over d slots of one row after preds[limit:] = fill (-100 in STM:116-119): the first maximum wins, a NaN counts as the
// maximum (the first NaN wins)
__device__ __forceinline__ int masked_argmax(const float* __restrict__ row, int d, int lim, float fill) {
    float bv = 0 < lim ? row[0] : fill;
    int best = 0;
    if (isnan(bv)) return 0;
    for (int j = 1; j < d; ++j) {
        const float t = j < lim ? row[j] : fill;
        if (isnan(t)) return j;
        if (t > bv) {
            bv = t;
            best = j;
        }
    }
    return best;
}

// The step tables of a call (multihop.StepTables: node / edge / sign [n_nodes, d] and deg [n_nodes]) and the bounds a lookup is held to.
// Each kernel used to clamp a degree its own way -- not at all, at both ends, at the upper end only; they agree wherever
// 0 <= deg <= d, which is every table the host builds (and a slot index never reaches d), so the one clamp of live_deg serves all.
// A wrapper whose ABI has no deg, edge, sign or n_rows fills that member with NULL / 0: its kernel then must not call the method
// that reads it (live_deg reads deg; no_edge reads edge, node and n_rows).  tree_target calls live_deg only, sample_draw both but
// never reads sign, sample_expand neither.
struct StepTab {
    const int32_t* deg;
    const int32_t* node;
    const int32_t* edge;
    const float* sign;
    int n_nodes, d, n_rows;
    // the slots of node v that are candidates: 0 for a node outside [0, n_nodes) (a dead entry), else deg[v] clamped to [0, d]
    __device__ __forceinline__ int live_deg(int v) const {
        if (v < 0 || v >= n_nodes) return 0;
        const int dv = deg[v];
        return dv < 0 ? 0 : (dv > d ? d : dv);
    }
    // slot j of the live node v has no edge (KeyError in the reference)
    __device__ __forceinline__ bool no_edge(int v, int j) const {
        const size_t k = (size_t)v * d + j;
        return edge[k] < 0 || edge[k] >= n_rows || node[k] < 0;
    }
};

// The entries of the next level, as the callers allocate them: parent / slot / count where the decoder keeps them, no paths on a final level
struct Children {
    int32_t* root;
    int32_t* node;
    float* score;
    int32_t* parent;
    int32_t* slot;
    int32_t* count;
    int32_t* path_row;
    float* path_sign;
};

// Child c: the entry itself (by lane 0), then the h path entries of its parent (from src of path_row / path_sign) with (edge, sign)
// appended -- by one thread, or lane-strided by the `stride` lanes of a wave that owns the child
__device__ __forceinline__ void write_child(const Children& ch, size_t c, int root, int node, float score, int parent, int slot, int count,
                                            const int32_t* __restrict__ path_row, const float* __restrict__ path_sign, size_t src, int h,
                                            int edge, float sign, int lane = 0, int stride = 1) {
    if (lane == 0) {
        ch.root[c] = root;
        ch.node[c] = node;
        ch.score[c] = score;
        if (ch.parent) ch.parent[c] = parent;
        if (ch.slot) ch.slot[c] = slot;
        if (ch.count) ch.count[c] = count;
    }
    if (!ch.path_row) return;
    const size_t dst = c * (size_t)(h + 1);
    for (int q = lane; q <= h; q += stride) {
        ch.path_row[dst + q] = q < h ? path_row[src + q] : edge;
        ch.path_sign[dst + q] = q < h ? path_sign[src + q] : sign;
    }
}

// child c of a beam that has fewer candidates than entries: dead
__device__ __forceinline__ void write_dead_child(const Children& ch, size_t c, int h) {
    ch.root[c] = -1;
    ch.node[c] = -1;
    ch.score[c] = -__builtin_inff();
    ch.parent[c] = -1;
    ch.slot[c] = -1;
    if (!ch.path_row) return;
    for (int q = 0; q <= h; ++q) {
        ch.path_row[c * (size_t)(h + 1) + q] = -1;
        ch.path_sign[c * (size_t)(h + 1) + q] = 0.f;
    }
}

__global__ __launch_bounds__(256) void hop_select_kernel(int n, StepTab tab, const float* __restrict__ logp,
                                                         const int32_t* __restrict__ n_limit, float fill, int32_t* cur, int32_t* last, int ns,
                                                         float* x, int advance, int32_t* __restrict__ choice,
                                                         int32_t* __restrict__ next_node, int32_t* err) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int v = cur[i], d = tab.d;
    const int c = masked_argmax(logp + (size_t)i * d, d, n_limit ? n_limit[i] : tab.live_deg(v), fill);
    choice[i] = c;
    if (!tab.edge) return;                                           // final hop of the accuracy: no lookup (STM:121-122)
    if (v < 0 || v >= tab.n_nodes || tab.no_edge(v, c)) {             // the pair has no edge: nothing written
        atomicMin(err, i);
        return;
    }
    const size_t k = (size_t)v * d + c;
    const int u = tab.node[k];
    if (next_node) next_node[i] = u;
    if (x) x[((size_t)(i / ns) * tab.n_rows + tab.edge[k]) * ns + (i % ns)] = tab.sign[k];     // SET, not add (STM:149-150)
    if (advance) {
        cur[i] = u;
        last[i] = u;
    }
}

// one thread per (leaf, slot): the children of leaf l go to offset[l] + j, leaf-major and slot-minor (STM:176-198)
__global__ __launch_bounds__(256) void tree_expand_kernel(int n_leaves, int h, StepTab tab, const int32_t* __restrict__ root,
                                                          const int32_t* __restrict__ node, const float* __restrict__ prob,
                                                          const int32_t* __restrict__ path_row, const float* __restrict__ path_sign,
                                                          const float* __restrict__ logp, const int32_t* __restrict__ offset,
                                                          int n_children, Children ch, int32_t* err) {
    const int d = tab.d;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)n_leaves * d) return;
    const int l = (int)(t / d), j = (int)(t % d);
    const int v = node[l];
    if (j >= tab.live_deg(v)) return;
    const size_t k = (size_t)v * d + j;
    const int c = offset[l] + j;
    if (tab.no_edge(v, j) || c < 0 || c >= n_children) {
        atomicMin(err, (int)t);
        return;
    }
    write_child(ch, c, root[l], tab.node[k], prob[l] * expf(logp[(size_t)l * d + j]), 0, 0, 0, path_row, path_sign, (size_t)l * h, h,
                tab.edge[k], tab.sign[k]);
}

// one thread per (slab, row) of the output: the ns = 4 leaves' root columns, one 16-byte store
__global__ __launch_bounds__(256) void tree_copy_kernel(int n_leaves, int64_t n_items, const int32_t* __restrict__ root, int n_roots,
                                                        const float* __restrict__ root_x, int n_rows, float* __restrict__ x) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_items; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = t / n_rows;
        const int r = (int)(t % n_rows);
        *reinterpret_cast<float4*>(x + (size_t)t * 4) = scn::root_columns(s, r, n_leaves, root, n_roots, root_x, n_rows);
    }
}

// one thread per leaf: its path entries in level order, so the last write of an edge wins and a root entry is overwritten (STM:187)
__global__ __launch_bounds__(256) void tree_patch_kernel(int n_leaves, int h, const int32_t* __restrict__ path_row,
                                                         const float* __restrict__ path_sign, int n_rows, float* __restrict__ x) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_leaves) return;
    for (int q = 0; q < h; ++q) {
        const int r = path_row[(size_t)l * h + q];
        if (r >= 0 && r < n_rows) x[((size_t)(l >> 2) * n_rows + r) * 4 + (l & 3)] = path_sign[(size_t)l * h + q];
    }
}

// one wave per root over its contiguous leaves; lane partial sums in a fixed order, then a fixed shuffle tree: bitwise repeatable
__global__ __launch_bounds__(64) void tree_target_kernel(int n_roots, const int32_t* __restrict__ leaf_ptr, const int32_t* __restrict__ node,
                                                         const float* __restrict__ prob, const float* __restrict__ logp, StepTab tab,
                                                         const int32_t* __restrict__ target, float* __restrict__ out) {
    const int r = blockIdx.x;
    const int lane = threadIdx.x, d = tab.d;
    if (r >= n_roots) return;
    const int tg = target[r];
    float s = 0.f;
    int cnt = 0;
    for (int l = leaf_ptr[r] + lane; l < leaf_ptr[r + 1]; l += 64) {
        const int v = node[l];
        const int dv = tab.live_deg(v);
        for (int j = 0; j < dv; ++j) {
            if (tab.node[(size_t)v * d + j] == tg) {
                s += prob[l] * expf(logp[(size_t)l * d + j]);
                ++cnt;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_down(s, o, 64);
        cnt += __shfl_down(cnt, o, 64);
    }
    if (lane == 0) out[r] = cnt ? s / (float)cnt : __builtin_nanf("");     // 0 / 0 in the reference (STM:203)
}

// The beam's total order as one 64-bit key, higher = earlier: the score mapped to an unsigned that orders like the float (a NaN
// above +inf, -0 with +0), then the candidate's index c = k * d + j counted down, so equal scores fall to the lower k, then the lower
// j.  Keys of distinct candidates differ, none is 0 (the score half of -inf is 0x007fffff) and none is ~0.
__device__ __forceinline__ unsigned long long beam_key(float s, int c) {
    unsigned u;
    if (isnan(s)) {
        u = 0xffffffffu;
    } else {
        const unsigned b = __float_as_uint(s == 0.f ? 0.f : s);
        u = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    return ((unsigned long long)u << 32) | (unsigned)(0x7fffffff - c);
}

// one wave per root.  Round o finds, lane-strided over the root's w_in * d candidates and then by a shuffle butterfly, the highest key
// strictly below round o - 1's winner: no bookkeeping, any d, and nothing depends on the order lanes or blocks run in.
__global__ __launch_bounds__(64) void beam_step_kernel(int w_in, int w_out, int h, StepTab tab, const int32_t* __restrict__ node,
                                                       const float* __restrict__ score, const int32_t* __restrict__ path_row,
                                                       const float* __restrict__ path_sign, const float* __restrict__ logp, Children ch,
                                                       int32_t* err) {
    __shared__ int s_node[SCN_BEAM_MAX];
    __shared__ int s_lim[SCN_BEAM_MAX];              // slots of entry k that are candidates: deg[node], 0 for a dead entry
    __shared__ float s_score[SCN_BEAM_MAX];
    const int r = blockIdx.x;
    const int lane = threadIdx.x, d = tab.d;
    const size_t in0 = (size_t)r * w_in;
    for (int k = lane; k < w_in; k += 64) {
        const int v = node[in0 + k];
        s_node[k] = (v >= 0 && v < tab.n_nodes) ? v : -1;
        s_lim[k] = tab.live_deg(v);
        s_score[k] = score[in0 + k];
    }
    __syncthreads();
    const float* __restrict__ lp = logp + in0 * d;
    const int n_cand = w_in * d;
    // candidate c = k * d + j of lane `lane` advances by 64: (k, j) += (64 / d, 64 % d) with one carry
    const int k0 = lane / d, j0 = lane % d, dk = 64 / d, dj = 64 % d;
    for (int c = lane, k = k0, j = j0; c < n_cand; c += 64) {
        if (j < s_lim[k] && tab.no_edge(s_node[k], j)) atomicMin(err, (int)(in0 * d) + c);
        k += dk;
        j += dj;
        if (j >= d) {
            j -= d;
            ++k;
        }
    }
    const size_t out0 = (size_t)r * w_out;
    unsigned long long prev = ~0ull;
    int o = 0;
    for (; o < w_out; ++o) {
        unsigned long long best = 0;
        for (int c = lane, k = k0, j = j0; c < n_cand; c += 64) {
            if (j < s_lim[k]) {
                const unsigned long long key = beam_key(s_score[k] + lp[c], c);
                if (key < prev && key > best) best = key;
            }
            k += dk;
            j += dj;
            if (j >= d) {
                j -= d;
                ++k;
            }
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            const unsigned long long other = __shfl_xor(best, m, 64);
            best = other > best ? other : best;
        }
        if (best == 0) break;                                             // (wave-uniform) every candidate is placed
        prev = best;
        const int c = 0x7fffffff - (int)(unsigned)(best & 0xffffffffu);
        const int k = c / d, j = c - k * d;
        const size_t t = (size_t)s_node[k] * d + j;
        write_child(ch, out0 + o, r, tab.node[t], s_score[k] + lp[c], k, j, 0, path_row, path_sign, (in0 + k) * (size_t)h, h, tab.edge[t],
                    tab.sign[t], lane, 64);
    }
    for (int p = o + lane; p < w_out; p += 64) write_dead_child(ch, out0 + p, h);      // fewer than w_out candidates: the rest are dead
}


// ---- sampled paths: one entry per distinct path with a count; a level step = draw (pick per sample) + expand (merge equal picks) ----
constexpr int SAMPLE_THREADS = 256;
constexpr int SAMPLE_WORDS = SCN_SAMPLE_PAIRS_MAX / 32;      // words of the per-root (entry, slot) bitmap in LDS

// The slot rule of one sample in one entry (include/scone_hip.h): the masked argmax when inv_T is +inf or the maximum is not finite;
// else the first slot whose fp32 running sum of expf((logp_j - m) * inv_T) exceeds u * total, and the last slot of positive weight
// where rounding at the top end leaves none.  lim >= 1.  Every operation spelled out: one subtract, one multiply, no division.
__device__ __forceinline__ int sample_slot(const float* __restrict__ row, int d, int lim, float inv_T, float u) {
#pragma clang fp contract(off)
    const int a = masked_argmax(row, d, lim, -__builtin_inff());
    const float m = row[a];
    if (isinf(inv_T) || !isfinite(m)) return a;
    float total = 0.f;
    for (int j = 0; j < lim; ++j) total += expf((row[j] - m) * inv_T);
    const float thr = u * total;
    float c = 0.f;
    int last = a;
    for (int j = 0; j < lim; ++j) {
        const float w = expf((row[j] - m) * inv_T);
        c += w;
        if (c > thr) return j;
        if (w > 0.f) last = j;
    }
    return last;
}

// the entries of root r: [l0, l0 + ne), clamped to the level and to max_entries (a longer range is a caller's error, guarded only)
__device__ __forceinline__ void sample_range(const int32_t* __restrict__ leaf_ptr, int r, int n_leaves, int max_entries, int& l0, int& ne) {
    const int a = leaf_ptr[r], b = leaf_ptr[r + 1];
    l0 = a < 0 ? 0 : (a > n_leaves ? n_leaves : a);
    const int l1 = b < l0 ? l0 : (b > n_leaves ? n_leaves : b);
    ne = l1 - l0 < max_entries ? l1 - l0 : max_entries;
}

// one workgroup per root: the missing-edge word over every live (k, j), then every sample's pick and the bitmap of the used (k, j)
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_draw_kernel(int n_samples, int max_entries, int n_leaves, int h,
                                                                     uint64_t seed, float inv_T, const int32_t* __restrict__ leaf_ptr,
                                                                     const int32_t* __restrict__ node, const float* __restrict__ logp,
                                                                     const int32_t* __restrict__ entry_of, StepTab tab,
                                                                     int32_t* __restrict__ pick, int32_t* __restrict__ n_child, int32_t* err) {
    __shared__ unsigned s_bits[SAMPLE_WORDS];
    __shared__ int s_total;
    const int r = blockIdx.x, t = threadIdx.x, d = tab.d;
    int l0, ne;
    sample_range(leaf_ptr, r, n_leaves, max_entries, l0, ne);
    const int n_pairs = ne * d, n_words = (n_pairs + 31) >> 5;
    for (int w = t; w < n_words; w += SAMPLE_THREADS) s_bits[w] = 0u;
    if (t == 0) s_total = 0;
    for (int c = t; c < n_pairs; c += SAMPLE_THREADS) {
        const int k = c / d, j = c - k * d;
        const int v = node[l0 + k];
        if (j < tab.live_deg(v) && tab.no_edge(v, j)) atomicMin(err, (l0 + k) * d + j);
    }
    __syncthreads();
    const size_t s0 = (size_t)r * n_samples;
    for (int s = t; s < n_samples; s += SAMPLE_THREADS) {
        const int k = entry_of[s0 + s];
        int p = -1;
        if (k >= 0 && k < ne) {
            const int lim = tab.live_deg(node[l0 + k]);
            if (lim > 0) {
                const float u = scn::sample_uniform(seed, r, s, h);
                p = k * d + sample_slot(logp + (size_t)(l0 + k) * d, d, lim, inv_T, u);
                atomicOr(&s_bits[p >> 5], 1u << (p & 31));
            }
        }
        pick[s0 + s] = p;
    }
    __syncthreads();
    int cnt = 0;
    for (int w = t; w < n_words; w += SAMPLE_THREADS) cnt += __popc(s_bits[w]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
    if ((t & 63) == 0 && cnt) atomicAdd(&s_total, cnt);
    __syncthreads();
    if (t == 0) n_child[r] = s_total;
}

// one workgroup per root: the bitmap again from the picks, its running population count, then one child per set bit at
// child_ptr[r] + rank (ascending pick = lower parent, then lower slot) and every sample's rank
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_expand_kernel(int n_samples, int max_entries, int n_leaves, int h, StepTab tab,
                                                                       const int32_t* __restrict__ leaf_ptr, const int32_t* __restrict__ node,
                                                                       const float* __restrict__ score, const int32_t* __restrict__ path_row,
                                                                       const float* __restrict__ path_sign, const float* __restrict__ logp,
                                                                       const int32_t* __restrict__ pick, const int32_t* __restrict__ child_ptr,
                                                                       int n_children, Children ch, int32_t* __restrict__ entry_of_next) {
    __shared__ unsigned s_bits[SAMPLE_WORDS];
    __shared__ int s_before[SAMPLE_WORDS];           // set bits in the words before this one
    __shared__ int s_count[SCN_SAMPLE_MAX];          // samples of the child of each rank (children <= samples)
    __shared__ int s_wave[SAMPLE_THREADS / 64];
    const int r = blockIdx.x, t = threadIdx.x, d = tab.d, n_nodes = tab.n_nodes;
    int l0, ne;
    sample_range(leaf_ptr, r, n_leaves, max_entries, l0, ne);
    const int n_pairs = ne * d, n_words = (n_pairs + 31) >> 5;
    for (int w = t; w < n_words; w += SAMPLE_THREADS) s_bits[w] = 0u;
    for (int s = t; s < n_samples; s += SAMPLE_THREADS) s_count[s] = 0;
    __syncthreads();
    const size_t s0 = (size_t)r * n_samples;
    // a pick outside the root's pairs, or through an entry that stands on no node, is no pick (only the draw's own output is in range)
    auto valid = [&](int p) {
        if (p < 0 || p >= n_pairs) return false;
        const int v = node[l0 + p / d];
        return v >= 0 && v < n_nodes;
    };
    for (int s = t; s < n_samples; s += SAMPLE_THREADS) {
        const int p = pick[s0 + s];
        if (valid(p)) atomicOr(&s_bits[p >> 5], 1u << (p & 31));
    }
    __syncthreads();
    // exclusive scan of the words' population counts: thread t owns the words [t * per, (t + 1) * per)
    const int per = (n_words + SAMPLE_THREADS - 1) / SAMPLE_THREADS;
    const int w0 = t * per, w1 = w0 + per < n_words ? w0 + per : n_words;
    int mine = 0;
    for (int w = w0; w < w1; ++w) mine += __popc(s_bits[w]);
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int other = __shfl_up(incl, o, 64);
        if ((t & 63) >= o) incl += other;
    }
    if ((t & 63) == 63) s_wave[t >> 6] = incl;
    __syncthreads();
    int run = incl - mine;
    for (int q = 0; q < (t >> 6); ++q) run += s_wave[q];
    for (int w = w0; w < w1; ++w) {
        s_before[w] = run;
        run += __popc(s_bits[w]);
    }
    __syncthreads();
    for (int s = t; s < n_samples; s += SAMPLE_THREADS) {
        const int p = pick[s0 + s];
        int rank = -1;
        if (valid(p)) {
            rank = s_before[p >> 5] + __popc(s_bits[p >> 5] & ((1u << (p & 31)) - 1u));
            atomicAdd(&s_count[rank], 1);
        }
        entry_of_next[s0 + s] = rank;
    }
    __syncthreads();
    const int c0 = child_ptr[r];
    for (int w = t; w < n_words; w += SAMPLE_THREADS) {
        unsigned bits = s_bits[w];
        int rank = s_before[w];
        for (; bits; bits &= bits - 1u, ++rank) {
            const int p = (w << 5) + __ffs(bits) - 1;
            const int k = p / d, j = p - k * d;
            const int c = c0 + rank;
            if (c < 0 || c >= n_children) continue;                      // child_ptr is not the scan of the draw's n_child: guarded only
            const size_t q = (size_t)node[l0 + k] * d + j;
            write_child(ch, c, r, tab.node[q], score[l0 + k] + logp[(size_t)(l0 + k) * d + j], k, j, s_count[rank], path_row, path_sign,
                        (size_t)(l0 + k) * h, h, tab.edge[q], tab.sign[q]);
        }
    }
}
}  // namespace

extern "C" {

int scn_hop_select(int32_t n, int32_t d, const float* logp, const int32_t* n_limit, float fill, const int32_t* deg, int32_t* cur,
                   int32_t* last, int32_t n_nodes, const int32_t* step_node, const int32_t* step_edge, const float* step_sign,
                   int32_t n_rows, int32_t ns, float* x, int32_t advance, int32_t* choice, int32_t* next_node, int32_t* err,
                   void* stream) {
    if (n < 0 || d <= 0 || n_nodes <= 0 || n_rows < 0 || ns <= 0) return SCN_ERR_BAD_SHAPE;
    if (!logp || !cur || !choice || (!n_limit && !deg)) return SCN_ERR_BAD_ARG;
    if (step_edge && (!step_node || !step_sign || !err)) return SCN_ERR_BAD_ARG;
    if (advance && (!step_edge || !last)) return SCN_ERR_BAD_ARG;
    if (x && !step_edge) return SCN_ERR_BAD_ARG;
    if (n == 0) return SCN_OK;
    hipLaunchKernelGGL(hop_select_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                       StepTab{deg, step_node, step_edge, step_sign, n_nodes, d, n_rows}, logp, n_limit, fill, cur, last, ns, x, advance,
                       choice, next_node, err);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int scn_tree_expand(int32_t n_leaves, int32_t h, int32_t d, const int32_t* root, const int32_t* node, const float* prob,
                    const int32_t* path_row, const float* path_sign, const float* logp, const int32_t* offset, const int32_t* deg,
                    int32_t n_nodes, const int32_t* step_node, const int32_t* step_edge, const float* step_sign, int32_t n_rows,
                    int32_t n_children, int32_t* c_root, int32_t* c_node, float* c_prob, int32_t* c_path_row, float* c_path_sign,
                    int32_t* err, void* stream) {
    if (n_leaves < 0 || h < 0 || d <= 0 || n_nodes <= 0 || n_rows <= 0 || n_children < 0) return SCN_ERR_BAD_SHAPE;
    if ((int64_t)n_leaves * d >= INT_MAX) return SCN_ERR_UNSUPPORTED;
    if (n_leaves == 0) return SCN_OK;
    if (!root || !node || !prob || !logp || !offset || !deg || !step_node || !step_edge || !step_sign || !err) return SCN_ERR_BAD_ARG;
    if (h > 0 && (!path_row || !path_sign)) return SCN_ERR_BAD_ARG;
    if (n_children > 0 && (!c_root || !c_node || !c_prob || !c_path_row || !c_path_sign)) return SCN_ERR_BAD_ARG;
    const int64_t items = (int64_t)n_leaves * d;
    hipLaunchKernelGGL(tree_expand_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_leaves, h,
                       StepTab{deg, step_node, step_edge, step_sign, n_nodes, d, n_rows}, root, node, prob, path_row, path_sign, logp, offset,
                       n_children, Children{c_root, c_node, c_prob, nullptr, nullptr, nullptr, c_path_row, c_path_sign}, err);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int scn_tree_slabs(int32_t n_leaves, int32_t n_slabs, int32_t h, const int32_t* root, const int32_t* path_row, const float* path_sign,
                   int32_t n_roots, const float* root_x, int32_t n_rows, int32_t ns, float* x, void* stream) {
    if (n_leaves < 0 || n_slabs <= 0 || h < 0 || n_roots <= 0 || n_rows <= 0) return SCN_ERR_BAD_SHAPE;
    if (ns != 4) return SCN_ERR_UNSUPPORTED;
    if ((int64_t)n_leaves > (int64_t)n_slabs * ns) return SCN_ERR_BAD_SHAPE;
    if (!x || !root_x || (n_leaves > 0 && !root) || (h > 0 && n_leaves > 0 && (!path_row || !path_sign))) return SCN_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(x) & 15) != 0) return SCN_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t items = (int64_t)n_slabs * n_rows;
    const int64_t blocks = (items + 255) / 256;
    hipLaunchKernelGGL(tree_copy_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, n_leaves, items, root,
                       n_roots, root_x, n_rows, x);
    SCN_LAUNCH_CHECK();
    if (h > 0 && n_leaves > 0) {
        hipLaunchKernelGGL(tree_patch_kernel, dim3((unsigned)((n_leaves + 255) / 256)), dim3(256), 0, st, n_leaves, h, path_row,
                           path_sign, n_rows, x);
        SCN_LAUNCH_CHECK();
    }
    return SCN_OK;
}

int scn_tree_target(int32_t n_roots, const int32_t* leaf_ptr, const int32_t* node, const float* prob, const float* logp, int32_t d,
                    const int32_t* deg, int32_t n_nodes, const int32_t* step_node, const int32_t* target, float* out, void* stream) {
    if (n_roots < 0 || d <= 0 || n_nodes <= 0) return SCN_ERR_BAD_SHAPE;
    if (n_roots == 0) return SCN_OK;
    if (!leaf_ptr || !node || !prob || !logp || !deg || !step_node || !target || !out) return SCN_ERR_BAD_ARG;
    hipLaunchKernelGGL(tree_target_kernel, dim3((unsigned)n_roots), dim3(64), 0, (hipStream_t)stream, n_roots, leaf_ptr, node, prob, logp,
                       StepTab{deg, step_node, nullptr, nullptr, n_nodes, d, 0}, target, out);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int scn_beam_step(int32_t n_roots, int32_t w_in, int32_t w_out, int32_t h, int32_t d, const int32_t* node, const float* score,
                  const int32_t* path_row, const float* path_sign, const float* logp, const int32_t* deg, int32_t n_nodes,
                  const int32_t* step_node, const int32_t* step_edge, const float* step_sign, int32_t n_rows, int32_t* c_root,
                  int32_t* c_node, float* c_score, int32_t* c_parent, int32_t* c_slot, int32_t* c_path_row, float* c_path_sign,
                  int32_t* err, void* stream) {
    if (n_roots < 0 || w_in <= 0 || w_out <= 0 || h < 0 || d <= 0 || n_nodes <= 0 || n_rows <= 0) return SCN_ERR_BAD_SHAPE;
    if (w_in > SCN_BEAM_MAX || w_out > SCN_BEAM_MAX) return SCN_ERR_UNSUPPORTED;
    if ((int64_t)n_roots * w_in * d >= INT_MAX || (int64_t)n_roots * w_out >= INT_MAX) return SCN_ERR_UNSUPPORTED;
    if (n_roots == 0) return SCN_OK;
    if (!node || !score || !logp || !deg || !step_node || !step_edge || !step_sign || !err) return SCN_ERR_BAD_ARG;
    if (!c_root || !c_node || !c_score || !c_parent || !c_slot) return SCN_ERR_BAD_ARG;
    if (c_path_row && (!c_path_sign || (h > 0 && (!path_row || !path_sign)))) return SCN_ERR_BAD_ARG;
    hipLaunchKernelGGL(beam_step_kernel, dim3((unsigned)n_roots), dim3(64), 0, (hipStream_t)stream, w_in, w_out, h,
                       StepTab{deg, step_node, step_edge, step_sign, n_nodes, d, n_rows}, node, score, path_row, path_sign, logp,
                       Children{c_root, c_node, c_score, c_parent, c_slot, nullptr, c_path_row, c_path_sign}, err);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int scn_sample_uniform(uint64_t seed, int32_t root, int32_t sample, int32_t hop, float* u) {
    if (!u) return SCN_ERR_BAD_ARG;
    *u = scn::sample_uniform(seed, root, sample, hop);
    return SCN_OK;
}

static int sample_shape(int32_t n_roots, int32_t n_samples, int32_t max_entries, int32_t n_leaves, int32_t h, int32_t d, int32_t n_nodes,
                        int32_t n_rows) {
    if (n_roots < 0 || n_samples <= 0 || max_entries <= 0 || n_leaves < 0 || h < 0 || d <= 0 || n_nodes <= 0 || n_rows <= 0)
        return SCN_ERR_BAD_SHAPE;
    if (n_samples > SCN_SAMPLE_MAX || (int64_t)max_entries * d > SCN_SAMPLE_PAIRS_MAX) return SCN_ERR_UNSUPPORTED;
    if ((int64_t)n_leaves * d >= INT_MAX || (int64_t)n_roots * n_samples >= INT_MAX) return SCN_ERR_UNSUPPORTED;
    return SCN_OK;
}

int scn_sample_draw(int32_t n_roots, int32_t n_samples, int32_t max_entries, int32_t n_leaves, int32_t h, int32_t d, uint64_t seed,
                    float inv_T, const int32_t* leaf_ptr, const int32_t* node, const float* logp, const int32_t* entry_of,
                    const int32_t* deg, int32_t n_nodes, const int32_t* step_node, const int32_t* step_edge, int32_t n_rows,
                    int32_t* pick, int32_t* n_child, int32_t* err, void* stream) {
    const int st = sample_shape(n_roots, n_samples, max_entries, n_leaves, h, d, n_nodes, n_rows);
    if (st != SCN_OK) return st;
    if (!(inv_T >= 0.f)) return SCN_ERR_BAD_ARG;
    if (n_roots == 0) return SCN_OK;
    if (!leaf_ptr || !node || !logp || !entry_of || !deg || !step_node || !step_edge || !pick || !n_child || !err) return SCN_ERR_BAD_ARG;
    hipLaunchKernelGGL(sample_draw_kernel, dim3((unsigned)n_roots), dim3(SAMPLE_THREADS), 0, (hipStream_t)stream, n_samples, max_entries,
                       n_leaves, h, seed, inv_T, leaf_ptr, node, logp, entry_of, StepTab{deg, step_node, step_edge, nullptr, n_nodes, d, n_rows},
                       pick, n_child, err);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int scn_sample_expand(int32_t n_roots, int32_t n_samples, int32_t max_entries, int32_t n_leaves, int32_t h, int32_t d,
                      const int32_t* leaf_ptr, const int32_t* node, const float* score, const int32_t* path_row, const float* path_sign,
                      const float* logp, const int32_t* pick, const int32_t* child_ptr, int32_t n_children, int32_t n_nodes,
                      const int32_t* step_node, const int32_t* step_edge, const float* step_sign, int32_t* c_root, int32_t* c_node,
                      float* c_score, int32_t* c_parent, int32_t* c_slot, int32_t* c_count, int32_t* c_path_row, float* c_path_sign,
                      int32_t* entry_of_next, void* stream) {
    const int st = sample_shape(n_roots, n_samples, max_entries, n_leaves, h, d, n_nodes, 1);
    if (st != SCN_OK) return st;
    if (n_children < 0) return SCN_ERR_BAD_SHAPE;
    if (n_roots == 0) return SCN_OK;
    if (!leaf_ptr || !node || !score || !logp || !pick || !child_ptr || !step_node || !step_edge || !step_sign || !entry_of_next)
        return SCN_ERR_BAD_ARG;
    if (n_children > 0 && (!c_root || !c_node || !c_score || !c_parent || !c_slot || !c_count)) return SCN_ERR_BAD_ARG;
    if (c_path_row && (!c_path_sign || (h > 0 && (!path_row || !path_sign)))) return SCN_ERR_BAD_ARG;
    hipLaunchKernelGGL(sample_expand_kernel, dim3((unsigned)n_roots), dim3(SAMPLE_THREADS), 0, (hipStream_t)stream, n_samples,
                       max_entries, n_leaves, h, StepTab{nullptr, step_node, step_edge, step_sign, n_nodes, d, 0}, leaf_ptr, node, score,
                       path_row, path_sign, logp, pick, child_ptr, n_children,
                       Children{c_root, c_node, c_score, c_parent, c_slot, c_count, c_path_row, c_path_sign}, entry_of_next);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

}  // extern "C"
