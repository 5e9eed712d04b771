// Readout (+ log-softmax), its backward, flow scatter and the fused Adam/ridge step.
#include <cstring>
#include <type_traits>

#include "scn_internal.h"

namespace scn {

#include "scn_readout_dev.inc"

__global__ __launch_bounds__(64) void readout_fwd_kernel(int ns, int n_edges, int c, const float* __restrict__ H,
                                                         const float* __restrict__ w, const int32_t* __restrict__ nbr,
                                                         int max_deg, const int32_t* __restrict__ last_nodes,
                                                         const int32_t* __restrict__ inc_ptr,
                                                         const int32_t* __restrict__ inc_edge,
                                                         const float* __restrict__ inc_sign,
                                                         float* __restrict__ bh, float* __restrict__ logits,
                                                         float* __restrict__ logp) {
    readout_fwd_body(blockIdx.x, threadIdx.x, ns, n_edges, c, H, w, nbr, max_deg, last_nodes, inc_ptr, inc_edge, inc_sign, bh, logits, logp);
}

constexpr int RO_ZERO_THREADS = 512;           // clear == 2: eight waves zero the column, wave 0 goes on alone
__global__ __launch_bounds__(RO_ZERO_THREADS) void readout_bwd_kernel(int ns, int n_edges, int c, const float* __restrict__ H,
                                                         const float* __restrict__ w, const int32_t* __restrict__ nbr,
                                                         int max_deg, const int32_t* __restrict__ last_nodes,
                                                         const int32_t* __restrict__ inc_ptr,
                                                         const int32_t* __restrict__ inc_edge,
                                                         const float* __restrict__ inc_sign,
                                                         const int32_t* __restrict__ edge_nodes,
                                                         const float* __restrict__ d_logp,
                                                         const float* __restrict__ logp, int act,
                                                         float* __restrict__ dz, float* __restrict__ dl_out, int clear) {
    // clear == 1: write zeros to exactly the dz entries the normal pass writes (scn_readout_clear_dz)
    // clear == 2: the workgroup (RO_ZERO_THREADS threads in this form, 64 otherwise) first zeroes its trajectory's whole column of dz
    //             ([s][all rows][i][:]: nobody else writes there), then wave 0 runs the normal pass alone -- small complexes: no fill
    //             launch over the gradient buffer, which may hold anything
    const int n = blockIdx.x;
    if (clear == 2) {
        readout_zero_column(dz, n / ns, n - (n / ns) * ns, ns, n_edges, c, threadIdx.x, blockDim.x);
        __syncthreads();
        clear = 0;
        if (threadIdx.x >= 64) return;                 // (a finished wave no longer takes part in the barriers below)
    }
    readout_bwd_body(n, threadIdx.x, ns, n_edges, c, H, w, nbr, max_deg, last_nodes, inc_ptr, inc_edge, inc_sign, edge_nodes, d_logp, logp,
                     act, dz, dl_out, clear);
}

// The readout of a step in ONE launch (scn_readout_step), one wave per trajectory: the forward (bh, logits, logp), the cross-entropy's
// scaling d_logp = y * scale of the trajectory's own max_deg entries, and the backward (d_logits, the dz rows on a buffer that is
// all-zero) -- each the body of its own kernel, in that order, so every output has the separate launches' bits.  The backward reads
// back what this wave's own lanes stored (logp, d_logp) and H rows the forward just read.  Workgroup 0 also zero-fills zero_buf, which
// nothing else in the launch touches (the gradient buffer of a fresh step: scn_masked_ce_begin's pair).
__global__ __launch_bounds__(64) void readout_step_kernel(int ns, int n_edges, int c, const float* __restrict__ H,
                                                          const float* __restrict__ w, const int32_t* __restrict__ nbr,
                                                          int max_deg, const int32_t* __restrict__ last_nodes,
                                                          const int32_t* __restrict__ inc_ptr,
                                                          const int32_t* __restrict__ inc_edge,
                                                          const float* __restrict__ inc_sign,
                                                          const int32_t* __restrict__ edge_nodes, const float* __restrict__ y,
                                                          float scale, int act, float* __restrict__ bh, float* __restrict__ logits,
                                                          float* logp, float* d_logp, float* __restrict__ dl_out,
                                                          float* __restrict__ dz, float* __restrict__ zero_buf, int64_t zero_n) {
    const int n = blockIdx.x, lane = threadIdx.x;
    if (n == 0)
        for (int64_t t = lane; t < zero_n; t += 64) zero_buf[t] = 0.f;
    readout_fwd_body(n, lane, ns, n_edges, c, H, w, nbr, max_deg, last_nodes, inc_ptr, inc_edge, inc_sign, bh, logits, logp);
    if (lane < max_deg) d_logp[(size_t)n * max_deg + lane] = y[(size_t)n * max_deg + lane] * scale;
    __syncthreads();
    readout_bwd_body(n, lane, ns, n_edges, c, H, w, nbr, max_deg, last_nodes, inc_ptr, inc_edge, inc_sign, edge_nodes, d_logp, logp, act,
                     dz, dl_out, 0);
}

__global__ __launch_bounds__(1024) void readout_dw_kernel(int nd, int c, const float* __restrict__ dl,
                                                          const float* __restrict__ bh, float* __restrict__ d_w) {
    readout_dw_body(threadIdx.x, nd, c, dl, bh, d_w);
}

// Keep mask of a last layer's forward (scn_keep_mask): thread = leaf i of slab i / ns, standing on node[i]; bit (b, slab) is set for
// every block b of T(node[i]) (the `top` table of scn_field_lists).  A node outside [0, n_nodes) or a block outside [0, n_blocks)
// is a caller's error that is only guarded against: nothing is read or written through it.
// LIST (scn_keep_mask_units): the thread whose atomic OR found the word zero appends the word's index b * words + w to the mask's
// unit list -- exactly once per non-empty word, in no particular order; the position is an atomicAdd on the list's counter.  Without
// a list the kernel is the loop it always was.
template <bool LIST>
__global__ __launch_bounds__(256) void keep_mask_kernel(int n, int ns, const int32_t* __restrict__ node, int n_nodes,
                                                        const int32_t* __restrict__ top_ptr, const int32_t* __restrict__ top_blk,
                                                        int n_blocks, int words, uint32_t* __restrict__ mask,
                                                        uint32_t* __restrict__ units, uint32_t* __restrict__ count, uint32_t capacity) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int v = node[i];
    if (v < 0 || v >= n_nodes) return;
    const int s = i / ns;
    const uint32_t bit = 1u << (s & 31);
    if (!LIST) {
        for (int t = top_ptr[v]; t < top_ptr[v + 1]; ++t) {
            const int b = top_blk[t];
            if (b >= 0 && b < n_blocks) atomicOr(&mask[(size_t)b * words + (s >> 5)], bit);
        }
        return;
    }
    // The OR's old value is a memory round trip, and so is the list position: four blocks of T(v) at a time (most nodes have no
    // more), their ORs in flight together, then ONE atomicAdd for the chunk's new words -- two dependent round trips per chunk, not
    // two per block.
    constexpr int CH = 4;
    const int t1 = top_ptr[v + 1];
    for (int t0 = top_ptr[v]; t0 < t1; t0 += CH) {
        size_t w[CH];
        bool ok[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int b = t0 + j < t1 ? top_blk[t0 + j] : -1;
            ok[j] = b >= 0 && b < n_blocks;
            w[j] = ok[j] ? (size_t)b * words + (s >> 5) : 0;
        }
        uint32_t before[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) before[j] = ok[j] ? atomicOr(&mask[w[j]], bit) : ~0u;
        uint32_t fresh = 0;
#pragma unroll
        for (int j = 0; j < CH; ++j) fresh += before[j] == 0;
        if (fresh) {
            uint32_t pos = atomicAdd(count, fresh);
#pragma unroll
            for (int j = 0; j < CH; ++j)
                if (before[j] == 0) {
                    if (pos < capacity) units[pos] = (uint32_t)w[j];   // (capacity >= n_blocks * words, checked by the host: always)
                    ++pos;
                }
        }
    }
}

// One hop out from a keep mask (scn_mask_hop), for the top layer's backward (scn_conv_backward_dzmask).  readout_bwd_kernel writes dz
// on exactly the rows readout_fwd_kernel reads of H -- the edges inc_edge[inc_ptr[v] .. inc_ptr[v + 1]) of every neighbour v >= 0 of
// the last node, less the edges it skips as handled from the other endpoint, which are among them -- so the keep mask M0 of the
// forward is also where the readout's gradient can be non-zero.  Block b of the backward stages the blocks of A(b) (the `adj` table
// of scn_field_lists): out[b][w] = OR of in[b'][w] over b' in A(b).  Pull form, thread = (b, w): one plain store per word, no atomics,
// the result does not depend on any order.  A block outside [0, n_blocks) is only guarded against, as in field_hop_kernel.
// LIST (scn_mask_hop_units): a thread whose word is non-zero appends its index t to the unit list of `out`; a wave reserves the
// positions of its non-zero words with ONE atomicAdd on the list's counter.
template <bool LIST>
__global__ __launch_bounds__(256) void mask_hop_kernel(int n_blocks, int words, const int32_t* __restrict__ adj_ptr,
                                                       const int32_t* __restrict__ adj_blk, const uint32_t* __restrict__ in,
                                                       uint32_t* __restrict__ out, uint32_t* __restrict__ units,
                                                       uint32_t* __restrict__ count, uint32_t capacity) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)n_blocks * words) return;
    const int b = (int)(t / words), w = (int)(t - (int64_t)b * words);
    uint32_t acc = 0;
    for (int k = adj_ptr[b]; k < adj_ptr[b + 1]; ++k) {
        const int b2 = adj_blk[k];
        if (b2 >= 0 && b2 < n_blocks) acc |= in[(size_t)b2 * words + w];
    }
    out[t] = acc;
    if (LIST) {
        const uint64_t live = __builtin_amdgcn_ballot_w64(acc != 0);        // (of the wave's active lanes)
        if (live) {
            const int lead = __builtin_ctzll(live), lane = threadIdx.x & 63;
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(live >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)live, 0u));
            uint32_t base = 0;
            if (lane == lead) base = atomicAdd(count, (uint32_t)__builtin_popcountll(live));
            base = __shfl(base, lead, 64);
            if (acc != 0 && base + rank < capacity) units[base + rank] = (uint32_t)t;   // (capacity >= n_blocks * words: always)
        }
    }
}

// The masks of a whole step in ONE launch (scn_cone_masks): workgroup g builds, for micro-batch g, the chain the three kernels above
// build in 2 + L launches -- M0 = keep mask of its last nodes, M_k = hop(M_{k-1}), every mask's unit list and count -- with the mask
// being read in LDS.  Thread t owns the words t, t + CM_THREADS, ... of every mask (at most MAXT of them: the trip count is a
// compile-time bound, so a hop's results stay in registers until everybody has read the image they replace: ONE LDS image).
//   M0:   the image is zeroed, the leaves OR their bits in with LDS atomics (CM_LEAF_LANES threads stride over a leaf's T(v)), the image
//         goes out to global in 16-byte stores (words before the first and after the last 16-byte boundary of the destination singly);
//   hop:  the pull form of mask_hop_kernel, `in` from LDS, the adjacency from global in aligned 16-byte loads, one plain store per word.  The
//         trips are a pipeline (a trip's row and first entries are fetched while the trips before it gather), and the first hop's
//         way into it does not depend on the mask: it is issued before the keep phase, whose chain of loads it overlaps;
//   list: pass j of the owned words covers [j * CM_THREADS, (j + 1) * CM_THREADS) in thread order, so (pass, wave) cells in order are
//         the words in order: a ballot per cell, one workgroup prefix over the cells' counts in LDS, and every live lane knows its
//         position.  No global atomic anywhere; entries ascend; nothing is written at or past the count; the L counts and the zeros
//         behind them are stored once, at the end.
// Every word of every mask is written, so the buffers may hold anything on entry: no memset.  Workgroups share nothing.  The guards
// of the kernels above hold: a node outside [0, n_nodes) or a block outside [0, n_blocks) contributes nothing and nothing is read or
// written through it.
constexpr int CM_THREADS = 1024, CM_WAVES = CM_THREADS / 64, CM_LEAF_LANES = 8;
static_assert(SCN_CONE_MASKS_MAX_WORDS % CM_THREADS == 0 && SCN_CONE_MASKS_MAX_WORDS * 4 + 4096 <= 160 * 1024,
              "the image and the list's cells fit a workgroup's LDS");
struct ConeMasksArgs { scn_cone_mb mb[SCN_CONE_MASKS_MAX_MB]; };
// words of one mask of a micro-batch of n leaves: n_blocks * ceil(ceil(n / ns) / 32), n > 0 (the host's checks, in 64 bits)
static inline int64_t cone_masks_words(int32_t n, int32_t ns, int32_t n_blocks) {
    const int64_t n_slabs = ((int64_t)n - 1) / ns + 1;
    return (int64_t)n_blocks * ((n_slabs + 31) / 32);
}

// exclusive prefix of v over the workgroup's threads in thread order (wave_sums: CM_WAVES words of LDS, free on entry); total = the sum
__device__ __forceinline__ uint32_t cm_exclusive_scan(uint32_t v, uint32_t* wave_sums, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wave_sums[wave] = incl;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < CM_WAVES; ++i) {
        const uint32_t x = wave_sums[i];
        base += i < wave ? x : 0u;
        total += x;
    }
    return base + incl - v;
}

// the unit list of the mask whose owned words are acc[0 .. MAXT): returns its count (the same in every thread).  Two barriers inside,
// one behind: cells and wave_sums are free again on return.
template <int MAXT>
__device__ __forceinline__ uint32_t cm_list(const uint32_t (&acc)[MAXT], int n_words, uint32_t* cells, uint32_t* wave_sums,
                                            uint32_t* __restrict__ units) {
    static_assert(MAXT * CM_WAVES <= CM_THREADS, "one thread per (pass, wave) cell");
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int j = 0; j < MAXT; ++j) {
        const uint64_t live = __builtin_amdgcn_ballot_w64(acc[j] != 0);
        if (lane == 0) cells[j * CM_WAVES + wave] = (uint32_t)__builtin_popcountll(live);
    }
    __syncthreads();
    uint32_t total;
    const uint32_t first = cm_exclusive_scan(t < MAXT * CM_WAVES ? cells[t] : 0u, wave_sums, total);
    __syncthreads();                                   // (every thread has read its cell's count)
    if (t < MAXT * CM_WAVES) cells[t] = first;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < MAXT; ++j) {
        const uint64_t live = __builtin_amdgcn_ballot_w64(acc[j] != 0);
        const uint32_t rank =__builtin_amdgcn_mbcnt_hi((uint32_t)(live >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)live, 0u));
        const int idx = t + j * CM_THREADS;
        if (acc[j] != 0 && idx < n_words) units[cells[j * CM_WAVES + wave] + rank] = (uint32_t)idx;
    }
    __syncthreads();
    return total;
}

// A hop's view of the adjacency.  The row of the word owned in trip j is the range [lo, hi) of adj_blk (empty past the mask's end).  A
// CmBatch is CM_BATCH consecutive entries of the table from cm_first(q) on -- q itself, or, where the table lies on a 16-byte boundary
// (wide), the boundary at or before it, so that the entries come in aligned 16-byte loads (what they bring from outside the row is not
// used); at the table's end, and for a table that does not lie so, single guarded loads.  A part wholly beyond the row is not loaded.
constexpr int CM_BATCH = 16;
struct CmRows {
    const int32_t* __restrict__ adj_ptr;
    const int32_t* __restrict__ adj_blk;
    int nnz, n_words, words;
    bool wide;
};
struct CmRange { int lo, hi; };
struct CmBatch { int4 q[CM_BATCH / 4]; };

__device__ __forceinline__ CmRange cm_range(const CmRows& R, int idx) {
    CmRange r{0, 0};
    if (idx < R.n_words) {
        const int b = R.words == 1 ? idx : idx / R.words;
        r.lo = R.adj_ptr[b];
        r.hi = R.adj_ptr[b + 1];
    }
    return r;
}
__device__ __forceinline__ int cm_first(const CmRows& R, int q) { return R.wide ? q & ~3 : q; }
__device__ __forceinline__ CmBatch cm_batch(const CmRows& R, int q, int hi) {
    CmBatch B;
    const int p0 = cm_first(R, q);
#pragma unroll
    for (int c = 0; c < CM_BATCH / 4; ++c) {
        const int p = p0 + 4 * c;
        B.q[c] = make_int4(-1, -1, -1, -1);
        if (p < hi) {
            if (R.wide && p + 4 <= R.nnz) {
                B.q[c] = *reinterpret_cast<const int4*>(R.adj_blk + p);
            } else {
                if (p >= q && p < hi) B.q[c].x = R.adj_blk[p];
                if (p + 1 >= q && p + 1 < hi) B.q[c].y = R.adj_blk[p + 1];
                if (p + 2 >= q && p + 2 < hi) B.q[c].z = R.adj_blk[p + 2];
                if (p + 3 >= q && p + 3 < hi) B.q[c].w = R.adj_blk[p + 3];
            }
        }
    }
    return B;
}
// OR of img[b' * words + w] over the batch's entries b' that lie in the row's part [q, hi) and in [0, n_blocks).  Every other entry
// reads the zero word the image keeps at `zero_at`: sixteen independent LDS reads under one wait, no branch per entry.
__device__ __forceinline__ uint32_t cm_gather(const CmRows& R, const CmBatch& B, int q, int hi, const uint32_t* img, int n_blocks, int w,
                                              int zero_at) {
    uint32_t a = 0;
    const int p0 = cm_first(R, q);
#pragma unroll
    for (int c = 0; c < CM_BATCH / 4; ++c) {
        const int v[4] = {B.q[c].x, B.q[c].y, B.q[c].z, B.q[c].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int p = p0 + 4 * c + e;
            a |= img[p >= q && p < hi && v[e] >= 0 && v[e] < n_blocks ? v[e] * R.words + w : zero_at];
        }
    }
    return a;
}

// The keep phase of a node -> blocks table into the zeroed LDS image: CM_LEAF_LANES threads stride over a leaf's row of the table and
// OR the leaf's slab bit into the words of its blocks.  Barriers are the caller's: one before (the image is zero), one behind.
__device__ __forceinline__ void cm_keep(const int32_t* __restrict__ node, int n, int ns, int n_nodes, const int32_t* __restrict__ ptr,
                                        const int32_t* __restrict__ blk, int n_blocks, int words, uint32_t* img) {
    const int t = threadIdx.x;
    for (int i = t / CM_LEAF_LANES; i < n; i += CM_THREADS / CM_LEAF_LANES) {
        const int v = node[i];
        if (v < 0 || v >= n_nodes) continue;
        const int s = i / ns;
        const uint32_t bit = 1u << (s & 31);
        const int q1 = ptr[v + 1];
        for (int q = ptr[v] + t % CM_LEAF_LANES; q < q1; q += CM_LEAF_LANES) {
            const int b = blk[q];
            if (b >= 0 && b < n_blocks) atomicOr(&img[b * words + (s >> 5)], bit);
        }
    }
}

// The image's n_words words out to global: 16-byte stores between the destination's first and last 16-byte boundary, single words
// outside them.
__device__ __forceinline__ void cm_stream_out(uint32_t* __restrict__ dst, const uint32_t* img, int n_words) {
    const int t = threadIdx.x;
    const int head = min(n_words, (int)(((16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u) >> 2));
    const int body = (n_words - head) & ~3;
    if (t < head) dst[t] = img[t];
    for (int i = head + t * 4; i < head + body; i += CM_THREADS * 4)
        *reinterpret_cast<uint4*>(dst + i) = make_uint4(img[i], img[i + 1], img[i + 2], img[i + 3]);
    if (t < n_words - head - body) dst[head + body + t] = img[head + body + t];
}

// VIS (scn_cone_masks_visits): behind the chain the workgroup also builds the visit masks V_1 .. V_{L-1} of its micro-batch, V_k = the
// keep mask of its last nodes against the table T_k (node -> the blocks holding a row k operator hops out from the readout's rows):
// the image is zeroed, the keep phase runs against T_k, the image goes out.  Every word of every V_k is written; no lists.
struct ConeVisitArgs {
    uint32_t* out[SCN_CONE_MASKS_MAX_MB];              // [L - 1][stride] of every micro-batch
    const int32_t* ptr[SCN_UNIT_COUNTERS - 1];         // T_1 .. T_{L-1}
    const int32_t* blk[SCN_UNIT_COUNTERS - 1];
};

struct ConeNoVisits {};

template <int MAXT, bool VIS>
__global__ __launch_bounds__(CM_THREADS) void cone_masks_kernel(ConeMasksArgs A, std::conditional_t<VIS, ConeVisitArgs, ConeNoVisits> VA,
                                                                int ns, int n_nodes, int n_blocks,
                                                                const int32_t* __restrict__ top_ptr, const int32_t* __restrict__ top_blk,
                                                                const int32_t* __restrict__ adj_ptr, const int32_t* __restrict__ adj_blk,
                                                                int L) {
    extern __shared__ __attribute__((aligned(16))) uint32_t cm_img[];           // the mask being read: n_words, rounded up to four, + four
    __shared__ uint32_t cells[MAXT * CM_WAVES], wave_sums[CM_WAVES];
    const scn_cone_mb& mb = A.mb[blockIdx.x];
    const int t = threadIdx.x;
    const int n = mb.n;
    const int32_t* __restrict__ node = mb.node;
    const int n_slabs = (n - 1) / ns + 1, words = (n_slabs + 31) / 32;           // (n > 0)
    const int n_words = n_blocks * words;                                       // (<= MAXT * CM_THREADS: the host's check)
    uint32_t* __restrict__ mask = mb.masks;
    uint32_t* __restrict__ units = mb.units;

    // the first hop's way in -- the rows of trips 0 and 1 and the first batch of trip 0 -- does not depend on the mask: its two
    // dependent trips to memory are issued here, ahead of the keep phase, and overlap the leaves' node -> top_ptr -> top_blk chain
    const CmRows R{adj_ptr, adj_blk, L > 1 ? adj_ptr[n_blocks] : 0, n_words, words, ((uintptr_t)adj_blk & 15u) == 0};
    CmRange r0{0, 0}, r1{0, 0};
    CmBatch b0 = cm_batch(R, 0, 0);
    if (L > 1) {
        r0 = cm_range(R, t);
        r1 = cm_range(R, t + CM_THREADS);
        b0 = cm_batch(R, r0.lo, r0.hi);
    }

    // M0 into the LDS image
    const int zero_at = (n_words + 3) & ~3;            // four words behind the image that stay zero: what a hop reads for an entry it passes over
    for (int i = t * 4; i < zero_at + 4; i += CM_THREADS * 4) *reinterpret_cast<uint4*>(cm_img + i) = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    cm_keep(node, n, ns, n_nodes, top_ptr, top_blk, n_blocks, words, cm_img);
    __syncthreads();
    cm_stream_out(mask, cm_img, n_words);
    uint32_t acc[MAXT];
#pragma unroll
    for (int j = 0; j < MAXT; ++j) {
        const int idx = t + j * CM_THREADS;
        acc[j] = idx < n_words ? cm_img[idx] : 0u;
    }
    uint32_t counts[SCN_UNIT_COUNTERS] = {};
    counts[0] = cm_list<MAXT>(acc, n_words, cells, wave_sums, units);

#pragma unroll 1
    for (int k = 1; k < L; ++k) {
        mask += mb.stride;
        units += mb.stride;
        if (k > 1) {
            r0 = cm_range(R, t);
            r1 = cm_range(R, t + CM_THREADS);
            b0 = cm_batch(R, r0.lo, r0.hi);
        }
        // a pipeline over the trips: while trip j gathers from the image, the first batch of trip j + 1 and the row of trip j + 2 are
        // under way (a row longer than a batch fetches the rest of it in place)
#pragma unroll
        for (int j = 0; j < MAXT; ++j) {
            const CmRange r2 = j + 2 < MAXT ? cm_range(R, t + (j + 2) * CM_THREADS) : CmRange{0, 0};
            const CmBatch b1 = cm_batch(R, r1.lo, r1.hi);
            const int idx = t + j * CM_THREADS;
            const int w = words == 1 ? 0 : idx % words;
            uint32_t a = cm_gather(R, b0, r0.lo, r0.hi, cm_img, n_blocks, w, zero_at);
            for (int q = cm_first(R, r0.lo) + CM_BATCH; q < r0.hi; q += CM_BATCH)
                a |= cm_gather(R, cm_batch(R, q, r0.hi), q, r0.hi, cm_img, n_blocks, w, zero_at);
            acc[j] = a;
            if (idx < n_words) mask[idx] = a;
            r0 = r1;
            r1 = r2;
            b0 = b1;
        }
        __syncthreads();                               // everybody has read M_{k-1}: the image becomes M_k
#pragma unroll
        for (int j = 0; j < MAXT; ++j) {
            const int idx = t + j * CM_THREADS;
            if (idx < n_words) cm_img[idx] = acc[j];
        }
        __syncthreads();
        const uint32_t c = cm_list<MAXT>(acc, n_words, cells, wave_sums, units);
#pragma unroll
        for (int i = 1; i < SCN_UNIT_COUNTERS; ++i)
            if (i == k) counts[i] = c;
    }
    if (t < SCN_UNIT_COUNTERS) {
        uint32_t c = 0;
#pragma unroll
        for (int i = 0; i < SCN_UNIT_COUNTERS; ++i)
            if (i == t) c = counts[i];
        mb.counters[t] = c;
    }
    if constexpr (VIS) {
        uint32_t* __restrict__ vis = VA.out[blockIdx.x];
#pragma unroll 1
        for (int k = 1; k < L; ++k, vis += mb.stride) {
            __syncthreads();                           // everybody is done with the image (cm_list's readers, the V before this one going out)
            for (int i = t * 4; i < zero_at; i += CM_THREADS * 4) *reinterpret_cast<uint4*>(cm_img + i) = make_uint4(0u, 0u, 0u, 0u);
            __syncthreads();
            cm_keep(node, n, ns, n_nodes, VA.ptr[k - 1], VA.blk[k - 1], n_blocks, words, cm_img);
            __syncthreads();
            cm_stream_out(vis, cm_img, n_words);
        }
    }
}

// one instantiation's launch; its dynamic-LDS attribute is set once per device, at the instantiation's full size, not per call
// (VA: a ConeVisitArgs, and the kernel builds the visit masks too, or a ConeNoVisits)
template <int MAXT, class Visits>
static int cone_masks_launch(const ConeMasksArgs& A, const Visits& VA, int n_mb, size_t lds, hipStream_t st, int ns, int n_nodes,
                             int n_blocks, const int32_t* top_ptr, const int32_t* top_blk, const int32_t* adj_ptr, const int32_t* adj_blk,
                             int L) {
    constexpr bool VIS = std::is_same<Visits, ConeVisitArgs>::value;
    static bool attr_set[64] = {};
    int dev = 0;
    SCN_HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
        SCN_HIP_TRY(hipFuncSetAttribute((const void*)cone_masks_kernel<MAXT, VIS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        MAXT * CM_THREADS * 4 + 16));
        if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
    hipLaunchKernelGGL((cone_masks_kernel<MAXT, VIS>), dim3(n_mb), dim3(CM_THREADS), lds, st, A, VA, ns, n_nodes, n_blocks, top_ptr, top_blk,
                       adj_ptr, adj_blk, L);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

// scn_cone_masks (Visits = ConeNoVisits; visits .. visit_blk unused) and scn_cone_masks_visits (ConeVisitArgs) behind their own checks
template <class Visits>
static int cone_masks_run(int32_t n_mb, const scn_cone_mb* mb, uint32_t* const* visits, int32_t ns, int32_t n_nodes, int32_t n_blocks,
                          const int32_t* top_ptr, const int32_t* top_blk, const int32_t* adj_ptr, const int32_t* adj_blk, int32_t L,
                          const int32_t* const* visit_ptr, const int32_t* const* visit_blk, void* stream) {
    constexpr bool VIS = std::is_same<Visits, ConeVisitArgs>::value;
    if (!mb || !top_ptr || !top_blk || !adj_ptr || !adj_blk) return SCN_ERR_BAD_ARG;
    if (n_mb <= 0 || ns <= 0 || n_nodes <= 0 || n_blocks <= 0 || L <= 0) return SCN_ERR_BAD_SHAPE;
    if (L > SCN_UNIT_COUNTERS) return SCN_ERR_UNSUPPORTED;
    if (VIS && L > 1) {
        if (!visits || !visit_ptr || !visit_blk) return SCN_ERR_BAD_ARG;
        for (int k = 0; k < L - 1; ++k)
            if (!visit_ptr[k] || !visit_blk[k]) return SCN_ERR_BAD_ARG;
    }
    // everything is checked before the first launch: a declined call has launched and written nothing
    int64_t widest = 0;
    for (int i = 0; i < n_mb; ++i) {
        if (!mb[i].node || !mb[i].masks || !mb[i].units || !mb[i].counters || (VIS && L > 1 && !visits[i])) return SCN_ERR_BAD_ARG;
        if (mb[i].n <= 0) return SCN_ERR_BAD_SHAPE;
        const int64_t n_words = cone_masks_words(mb[i].n, ns, n_blocks);
        if (L > 1 && mb[i].stride < n_words) return SCN_ERR_WORKSPACE;
        widest = std::max(widest, n_words);
    }
    if (widest > INT32_MAX || widest > SCN_CONE_MASKS_MAX_WORDS) return SCN_ERR_UNSUPPORTED;
    const size_t lds = (size_t)((widest + 3) / 4 * 4 + 4) * sizeof(uint32_t);         // (the image and its four zero words)
    const int trips = (int)((widest + CM_THREADS - 1) / CM_THREADS);
    for (int i0 = 0; i0 < n_mb; i0 += SCN_CONE_MASKS_MAX_MB) {
        const int m = std::min<int>(SCN_CONE_MASKS_MAX_MB, n_mb - i0);
        ConeMasksArgs A{};
        std::memcpy(A.mb, mb + i0, sizeof(scn_cone_mb) * (size_t)m);
        Visits VA{};
        if constexpr (VIS) {
            for (int k = 0; k < L - 1; ++k) VA.ptr[k] = visit_ptr[k], VA.blk[k] = visit_blk[k];
            if (L > 1) std::memcpy(VA.out, visits + i0, sizeof(uint32_t*) * (size_t)m);
        }
        int rc;
        if (trips <= 4)
            rc = cone_masks_launch<4>(A, VA, m, lds, (hipStream_t)stream, ns, n_nodes, n_blocks, top_ptr, top_blk, adj_ptr, adj_blk, L);
        else if (trips <= 20)
            rc = cone_masks_launch<20>(A, VA, m, lds, (hipStream_t)stream, ns, n_nodes, n_blocks, top_ptr, top_blk, adj_ptr, adj_blk, L);
        else
            rc = cone_masks_launch<SCN_CONE_MASKS_MAX_WORDS / CM_THREADS>(A, VA, m, lds, (hipStream_t)stream, ns, n_nodes, n_blocks, top_ptr,
                                                                          top_blk, adj_ptr, adj_blk, L);
        if (rc != SCN_OK) return rc;
    }
    return SCN_OK;
}

__global__ __launch_bounds__(64) void node_readout_fwd_kernel(int ns, int n_nodes, const float* __restrict__ X,
                                                              const int32_t* __restrict__ nbr, int max_deg,
                                                              const int32_t* __restrict__ last_nodes,
                                                              float* __restrict__ logits, float* __restrict__ logp) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const int s = n / ns, i = n - s * ns;
    const int vlast = last_nodes[n];
    float x = -INFINITY, lg = 0.f;
    if (lane < max_deg) {
        int v = nbr[(size_t)vlast * max_deg + lane];
        if (v < 0) v += n_nodes;                      // index -1 wraps to the last node (TE:201)
        lg = X[((size_t)s * n_nodes + v) * ns + i];
        x = lg;
    }
    const float m = wave_max(x);
    const float se = wave_sum(lane < max_deg ? expf(x - m) : 0.f);
    const float lse = m + logf(se);
    if (lane < max_deg) {
        logits[(size_t)n * max_deg + lane] = lg;
        logp[(size_t)n * max_deg + lane] = lg - lse;
    }
}

__global__ __launch_bounds__(64) void node_readout_bwd_kernel(int ns, int n_nodes, const float* __restrict__ X,
                                                              const int32_t* __restrict__ nbr, int max_deg,
                                                              const int32_t* __restrict__ last_nodes,
                                                              const float* __restrict__ d_logp,
                                                              const float* __restrict__ logp, int act,
                                                              float* __restrict__ dz) {
    __shared__ float dl[RO_MAXD];
    const int n = blockIdx.x, lane = threadIdx.x;
    const int s = n / ns, i = n - s * ns;
    const int vlast = last_nodes[n];
    const float g = lane < max_deg ? d_logp[(size_t)n * max_deg + lane] : 0.f;
    const float gs = wave_sum(g);
    if (lane < max_deg) dl[lane] = g - expf(logp[(size_t)n * max_deg + lane]) * gs;
    __syncthreads();
    if (lane == 0) {                                   // serial: several padded entries may hit the same node
        for (int d = 0; d < max_deg; ++d) {
            int v = nbr[(size_t)vlast * max_deg + d];
            if (v < 0) v += n_nodes;
            const size_t o = ((size_t)s * n_nodes + v) * ns + i;
            dz[o] += dl[d] * act_grad_from_output(act, X[o]);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The same four kernels for neighbourhoods wider than one wave's lanes (RO_MAXD < max_deg <= RO_WIDE): hub nodes.  One wave per
// trajectory as before; the per-slot values (logits, d_logits, neighbour ids) live in LDS arrays of RO_WIDE entries and the lanes
// stride over the slots.  Plain loops: a complex with such a node is rare and its readout is still a sliver of the step.
// ------------------------------------------------------------------------------------------------
constexpr int RO_WIDE = 1024;

__device__ __forceinline__ float lds_logsumexp(const float* vals, int n, int lane) {
    float m = -INFINITY;
    for (int d = lane; d < n; d += 64) m = fmaxf(m, vals[d]);
    m = wave_max(m);
    float se = 0.f;
    for (int d = lane; d < n; d += 64) se += expf(vals[d] - m);
    se = wave_sum(se);
    return m + logf(se);
}

__global__ __launch_bounds__(64) void readout_fwd_wide_kernel(int ns, int n_edges, int c, const float* __restrict__ H,
                                                              const float* __restrict__ w, const int32_t* __restrict__ nbr,
                                                              int max_deg, const int32_t* __restrict__ last_nodes,
                                                              const int32_t* __restrict__ inc_ptr,
                                                              const int32_t* __restrict__ inc_edge,
                                                              const float* __restrict__ inc_sign, float* __restrict__ bh,
                                                              float* __restrict__ logits, float* __restrict__ logp) {
    __shared__ float lgs[RO_WIDE];
    const int n = blockIdx.x, lane = threadIdx.x;
    const int s = n / ns, i = n - s * ns;
    const int vlast = last_nodes[n];
    for (int d = 0; d < max_deg; ++d) {
        const int v = nbr[(size_t)vlast * max_deg + d];
        float lg = 0.f;
        for (int c0 = 0; c0 < c; c0 += 64) {
            const int cc = c0 + lane;
            float acc = 0.f;
            if (v >= 0 && cc < c)
                for (int j = inc_ptr[v]; j < inc_ptr[v + 1]; ++j)
                    acc = fmaf(inc_sign[j], H[(((size_t)s * n_edges + inc_edge[j]) * ns + i) * c + cc], acc);
            if (cc < c) {
                bh[((size_t)n * max_deg + d) * c + cc] = acc;
                lg = fmaf(acc, w[cc], lg);
            }
        }
        lg = wave_sum(lg);
        if (lane == 0) lgs[d] = lg;
    }
    __syncthreads();
    const float lse = lds_logsumexp(lgs, max_deg, lane);       // padding rows (logit 0) take part, as in the reference (TE:151-152)
    for (int d = lane; d < max_deg; d += 64) {
        logits[(size_t)n * max_deg + d] = lgs[d];
        logp[(size_t)n * max_deg + d] = lgs[d] - lse;
    }
}

__global__ __launch_bounds__(64) void readout_bwd_wide_kernel(int ns, int n_edges, int c, const float* __restrict__ H,
                                                              const float* __restrict__ w, const int32_t* __restrict__ nbr,
                                                              int max_deg, const int32_t* __restrict__ last_nodes,
                                                              const int32_t* __restrict__ inc_ptr,
                                                              const int32_t* __restrict__ inc_edge,
                                                              const float* __restrict__ inc_sign,
                                                              const int32_t* __restrict__ edge_nodes,
                                                              const float* __restrict__ d_logp,
                                                              const float* __restrict__ logp, int act,
                                                              float* __restrict__ dz, float* __restrict__ dl_out, int clear) {
    __shared__ float dl[RO_WIDE];
    __shared__ int nb[RO_WIDE];
    const int n = blockIdx.x, lane = threadIdx.x;
    const int s = n / ns, i = n - s * ns;
    const int vlast = last_nodes[n];
    float g = 0.f;
    if (!clear)
        for (int d = lane; d < max_deg; d += 64) g += d_logp[(size_t)n * max_deg + d];
    const float gs = wave_sum(g);
    for (int d = lane; d < max_deg; d += 64) {
        if (!clear) {
            const float v = d_logp[(size_t)n * max_deg + d] - expf(logp[(size_t)n * max_deg + d]) * gs;
            dl[d] = v;
            dl_out[(size_t)n * max_deg + d] = v;
        } else {
            dl[d] = 0.f;
        }
        nb[d] = nbr[(size_t)vlast * max_deg + d];
    }
    __syncthreads();
    for (int d = 0; d < max_deg; ++d) {
        const int v = nb[d];
        if (v < 0) continue;
        for (int j = inc_ptr[v]; j < inc_ptr[v + 1]; ++j) {
            const int e = inc_edge[j];
            const int t = edge_nodes[2 * e], h = edge_nodes[2 * e + 1];
            const int other = (t == v) ? h : t;
            int dk = -1;                                       // slot of the edge's other endpoint, if it is a neighbour too (the last such slot)
            for (int q = lane; q < max_deg; q += 64)
                if (nb[q] == other) dk = q;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) dk = max(dk, __shfl_xor(dk, o, 64));
            if (dk >= 0 && other < v) continue;                // handled from the other endpoint's side
            const size_t base = (((size_t)s * n_edges + e) * ns + i) * c;
            if (clear) {
                for (int cc = lane; cc < c; cc += 64) dz[base + cc] = 0.f;
                continue;
            }
            const float coef = inc_sign[j] * (dl[d] - (dk >= 0 ? dl[dk] : 0.f));
            for (int cc = lane; cc < c; cc += 64) dz[base + cc] = coef * w[cc] * act_grad_from_output(act, H[base + cc]);
        }
    }
}

__global__ __launch_bounds__(64) void node_readout_fwd_wide_kernel(int ns, int n_nodes, const float* __restrict__ X,
                                                                   const int32_t* __restrict__ nbr, int max_deg,
                                                                   const int32_t* __restrict__ last_nodes,
                                                                   float* __restrict__ logits, float* __restrict__ logp) {
    __shared__ float lgs[RO_WIDE];
    const int n = blockIdx.x, lane = threadIdx.x;
    const int s = n / ns, i = n - s * ns;
    const int vlast = last_nodes[n];
    for (int d = lane; d < max_deg; d += 64) {
        int v = nbr[(size_t)vlast * max_deg + d];
        if (v < 0) v += n_nodes;                      // index -1 wraps to the last node (TE:201)
        lgs[d] = X[((size_t)s * n_nodes + v) * ns + i];
    }
    __syncthreads();
    const float lse = lds_logsumexp(lgs, max_deg, lane);
    for (int d = lane; d < max_deg; d += 64) {
        logits[(size_t)n * max_deg + d] = lgs[d];
        logp[(size_t)n * max_deg + d] = lgs[d] - lse;
    }
}

__global__ __launch_bounds__(64) void node_readout_bwd_wide_kernel(int ns, int n_nodes, const float* __restrict__ X,
                                                                   const int32_t* __restrict__ nbr, int max_deg,
                                                                   const int32_t* __restrict__ last_nodes,
                                                                   const float* __restrict__ d_logp,
                                                                   const float* __restrict__ logp, int act,
                                                                   float* __restrict__ dz) {
    __shared__ float dl[RO_WIDE];
    const int n = blockIdx.x, lane = threadIdx.x;
    const int s = n / ns, i = n - s * ns;
    const int vlast = last_nodes[n];
    float g = 0.f;
    for (int d = lane; d < max_deg; d += 64) g += d_logp[(size_t)n * max_deg + d];
    const float gs = wave_sum(g);
    for (int d = lane; d < max_deg; d += 64) dl[d] = d_logp[(size_t)n * max_deg + d] - expf(logp[(size_t)n * max_deg + d]) * gs;
    __syncthreads();
    if (lane == 0) {                                   // serial: several padded entries may hit the same node
        for (int d = 0; d < max_deg; ++d) {
            int v = nbr[(size_t)vlast * max_deg + d];
            if (v < 0) v += n_nodes;
            const size_t o = ((size_t)s * n_nodes + v) * ns + i;
            dz[o] += dl[d] * act_grad_from_output(act, X[o]);
        }
    }
}

__global__ void scatter_flows_kernel(int ns, int n_edges, int64_t n_entries, const int32_t* __restrict__ sample_of,
                                     const int32_t* __restrict__ edge_idx, const float* __restrict__ val,
                                     float* __restrict__ x) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_entries) return;
    const int n = sample_of[t];
    const int s = n / ns, i = n - s * ns;
    // accumulate: the reference builds a flow with f[k] += +-1 per traversed edge (SDG:327-344), so a repeated
    // (trajectory, edge) entry adds up -- like SparseFlows.todense() on the host (x is zeroed just before)
    atomicAdd(&x[((size_t)s * n_edges + edge_idx[t]) * ns + i], val[t]);
}

// masked cross-entropy of STM:54 for one micro-batch: d_logp = y * scale (scale = -1 / global batch size) and
// loss[0] += sum logp * d_logp in fp64, one block, fixed summation order
// logp[n][:] = z - logsumexp(z), z = sum over the parts of logits_k[n][:]  (one wave per trajectory, lanes stride over the slots)
struct LogitParts { const float* p[4]; };
__global__ __launch_bounds__(64) void logits_sum_log_softmax_kernel(int max_deg, int n_parts, LogitParts L, float* __restrict__ logits,
                                                                    float* __restrict__ logp) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const size_t base = (size_t)n * max_deg;
    float m = -INFINITY;
    for (int d = lane; d < max_deg; d += 64) {
        float z = L.p[0][base + d];
        if (n_parts > 1) z += L.p[1][base + d];
        if (n_parts > 2) z += L.p[2][base + d];
        if (n_parts > 3) z += L.p[3][base + d];
        logits[base + d] = z;
        m = fmaxf(m, z);
    }
    m = wave_max(m);
    float se = 0.f;
    for (int d = lane; d < max_deg; d += 64) se += expf(logits[base + d] - m);       // (this lane's own stores)
    se = wave_sum(se);
    const float lse = m + logf(se);
    for (int d = lane; d < max_deg; d += 64) logp[base + d] = logits[base + d] - lse;
}

__global__ __launch_bounds__(1024) void masked_ce_kernel(int64_t n, const float* __restrict__ logp,
                                                         const float* __restrict__ y, float scale,
                                                         float* __restrict__ d_logp, double* __restrict__ loss,
                                                         int overwrite = 0, float* __restrict__ zero_buf = nullptr, int64_t zero_n = 0) {
    for (int64_t t = threadIdx.x; t < zero_n; t += 1024) zero_buf[t] = 0.f;
    masked_ce_body<true>(threadIdx.x, n, logp, y, scale, d_logp, loss, overwrite);
}

__global__ void adam_kernel(int64_t n, float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, float lr, float b1, float b2, float eps, float c1, float c2,
                            float wd2, float g_scale) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    adam_update(w + t, g[t], m + t, v + t, lr, b1, b2, eps, c1, c2, wd2, g_scale);
}

// The same update (adam_update, scn_internal.h) with the step index in DEVICE memory: one workgroup (the flat buffer of every model of the reference is a few
// thousand floats), which reads step[0] = i, applies update i and leaves i + 1 there -- a launch whose arguments never change, so
// the optimiser step can sit inside a captured graph behind the gradient launches (on the reference's own problem sizes the
// hand-over from a graph replay to a plain launch is ~8 us of an ~80 us step).
constexpr int ADAM_DEV_THREADS = 1024;
__global__ __launch_bounds__(ADAM_DEV_THREADS) void adam_dev_kernel(int64_t n, float* __restrict__ w, const float* __restrict__ g,
                                                                  float* __restrict__ m, float* __restrict__ v, float lr, float b1,
                                                                  float b2, float eps, int32_t* step, float wd2, float g_scale) {
    __shared__ float c[2];
    const int i = step[0];                                       // (every thread, before the barrier: thread 0 writes it after the last one)
    if (threadIdx.x == 0) adam_corrections(b1, b2, i, c[0], c[1]);
    __syncthreads();
    const float c1 = c[0], c2 = c[1];
    for (int64_t t = threadIdx.x; t < n; t += ADAM_DEV_THREADS) adam_update(w + t, g[t], m + t, v + t, lr, b1, b2, eps, c1, c2, wd2, g_scale);
    __syncthreads();
    if (threadIdx.x == 0) step[0] = i + 1;
}

}  // namespace scn

using namespace scn;

extern "C" {

int scn_readout_forward(int32_t n_slabs, int32_t ns, int32_t n_edges, int32_t c, const float* H,
                        const float* w_last, const int32_t* nbr, int32_t n_nodes, int32_t max_deg,
                        const int32_t* last_nodes, const int32_t* inc_ptr, const int32_t* inc_edge,
                        const float* inc_sign, float* bh, float* logits, float* logp, void* stream) {
    if (!H || !w_last || !nbr || !last_nodes || !inc_ptr || !inc_edge || !inc_sign || !bh || !logits || !logp)
        return SCN_ERR_BAD_ARG;
    if (n_slabs <= 0 || ns <= 0 || n_edges <= 0 || c <= 0 || n_nodes <= 0 || max_deg <= 0) return SCN_ERR_BAD_SHAPE;
    if (max_deg > RO_WIDE) return SCN_ERR_UNSUPPORTED;
    if (max_deg > RO_MAXD)
        hipLaunchKernelGGL(readout_fwd_wide_kernel, dim3(n_slabs * ns), dim3(64), 0, (hipStream_t)stream, ns, n_edges, c, H,
                           w_last, nbr, max_deg, last_nodes, inc_ptr, inc_edge, inc_sign, bh, logits, logp);
    else
        hipLaunchKernelGGL(readout_fwd_kernel, dim3(n_slabs * ns), dim3(64), 0, (hipStream_t)stream, ns, n_edges, c, H,
                           w_last, nbr, max_deg, last_nodes, inc_ptr, inc_edge, inc_sign, bh, logits, logp);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int scn_readout_backward(int32_t n_slabs, int32_t ns, int32_t n_edges, int32_t c, const float* H,
                         const float* w_last, const int32_t* nbr, int32_t n_nodes, int32_t max_deg,
                         const int32_t* last_nodes, const int32_t* inc_ptr, const int32_t* inc_edge,
                         const float* inc_sign, const int32_t* edge_nodes, const float* bh, const float* d_logp,
                         const float* logp, int32_t act, float* d_logits, float* dz, int32_t dz_is_zero,
                         float* d_w_last, void* stream) {
    if (!H || !w_last || !nbr || !last_nodes || !inc_ptr || !inc_edge || !inc_sign || !edge_nodes || !bh ||
        !d_logp || !logp || !d_logits || !dz || !d_w_last)
        return SCN_ERR_BAD_ARG;
    if (n_slabs <= 0 || ns <= 0 || n_edges <= 0 || c <= 0 || n_nodes <= 0 || max_deg <= 0) return SCN_ERR_BAD_SHAPE;
    if (max_deg > RO_WIDE) return SCN_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const int N = n_slabs * ns;
    const bool self_zero = dz_is_zero == 2 && max_deg <= RO_MAXD;          // (the kernel of wide neighbourhoods has no such form)
    if (!dz_is_zero || (dz_is_zero == 2 && !self_zero)) SCN_HIP_TRY(hipMemsetAsync(dz, 0, sizeof(float) * (size_t)N * n_edges * c, st));
    float* dl = d_logits;
    if (max_deg > RO_MAXD)
        hipLaunchKernelGGL(readout_bwd_wide_kernel, dim3(N), dim3(64), 0, st, ns, n_edges, c, H, w_last, nbr, max_deg,
                           last_nodes, inc_ptr, inc_edge, inc_sign, edge_nodes, d_logp, logp, act, dz, dl, 0);
    else
        hipLaunchKernelGGL(readout_bwd_kernel, dim3(N), dim3(self_zero ? RO_ZERO_THREADS : 64), 0, st, ns, n_edges, c, H, w_last, nbr,
                           max_deg, last_nodes, inc_ptr, inc_edge, inc_sign, edge_nodes, d_logp, logp, act, dz, dl, self_zero ? 2 : 0);
    SCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(readout_dw_kernel, dim3(1), dim3(1024), 0, st, N * max_deg, c, dl, bh, d_w_last);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int scn_readout_step(int32_t n_slabs, int32_t ns, int32_t n_edges, int32_t c, const float* H, const float* w_last, const int32_t* nbr,
                     int32_t n_nodes, int32_t max_deg, const int32_t* last_nodes, const int32_t* inc_ptr, const int32_t* inc_edge,
                     const float* inc_sign, const int32_t* edge_nodes, const float* y, float scale, int32_t act, float* bh,
                     float* logits, float* logp, float* d_logp, float* d_logits, float* dz, int32_t dz_is_zero, float* zero_buf,
                     int64_t zero_n, void* stream) {
    if (!H || !w_last || !nbr || !last_nodes || !inc_ptr || !inc_edge || !inc_sign || !edge_nodes || !y || !bh || !logits || !logp ||
        !d_logp || !d_logits || !dz || (zero_n > 0 && !zero_buf))
        return SCN_ERR_BAD_ARG;
    if (n_slabs <= 0 || ns <= 0 || n_edges <= 0 || c <= 0 || n_nodes <= 0 || max_deg <= 0 || zero_n < 0) return SCN_ERR_BAD_SHAPE;
    // the fast form on a buffer kept all-zero: wide neighbourhoods, wide rows and the self-zeroing form of small complexes stay with
    // the separate launches
    if (max_deg > RO_MAXD || c > 64 || dz_is_zero != 1) return SCN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(readout_step_kernel, dim3(n_slabs * ns), dim3(64), 0, (hipStream_t)stream, ns, n_edges, c, H, w_last, nbr, max_deg,
                       last_nodes, inc_ptr, inc_edge, inc_sign, edge_nodes, y, scale, act, bh, logits, logp, d_logp, d_logits, dz,
                       zero_buf, zero_n);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int scn_readout_clear_dz(int32_t n_slabs, int32_t ns, int32_t n_edges, int32_t c, const int32_t* nbr, int32_t n_nodes,
                         int32_t max_deg, const int32_t* last_nodes, const int32_t* inc_ptr, const int32_t* inc_edge,
                         const int32_t* edge_nodes, float* dz, void* stream) {
    if (!nbr || !last_nodes || !inc_ptr || !inc_edge || !edge_nodes || !dz) return SCN_ERR_BAD_ARG;
    if (n_slabs <= 0 || ns <= 0 || n_edges <= 0 || c <= 0 || n_nodes <= 0 || max_deg <= 0) return SCN_ERR_BAD_SHAPE;
    if (max_deg > RO_WIDE) return SCN_ERR_UNSUPPORTED;
    if (max_deg > RO_MAXD)
        hipLaunchKernelGGL(readout_bwd_wide_kernel, dim3(n_slabs * ns), dim3(64), 0, (hipStream_t)stream, ns, n_edges, c, nullptr,
                           nullptr, nbr, max_deg, last_nodes, inc_ptr, inc_edge, nullptr, edge_nodes, nullptr, nullptr, 0, dz,
                           nullptr, 1);
    else
        hipLaunchKernelGGL(readout_bwd_kernel, dim3(n_slabs * ns), dim3(64), 0, (hipStream_t)stream, ns, n_edges, c, nullptr,
                           nullptr, nbr, max_deg, last_nodes, inc_ptr, inc_edge, nullptr, edge_nodes, nullptr, nullptr, 0, dz,
                           nullptr, 1);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int scn_keep_mask(int32_t n, int32_t ns, const int32_t* node, int32_t n_nodes, const int32_t* top_ptr, const int32_t* top_blk,
                  int32_t n_blocks, uint32_t* mask, void* stream) {
    if (!node || !top_ptr || !top_blk || !mask) return SCN_ERR_BAD_ARG;
    if (n <= 0 || ns <= 0 || n_nodes <= 0 || n_blocks <= 0) return SCN_ERR_BAD_SHAPE;
    const int n_slabs = (n + ns - 1) / ns, words = (n_slabs + 31) / 32;
    hipStream_t st = (hipStream_t)stream;
    SCN_HIP_TRY(hipMemsetAsync(mask, 0, sizeof(uint32_t) * (size_t)n_blocks * words, st));
    hipLaunchKernelGGL(keep_mask_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, st, n, ns, node, n_nodes, top_ptr, top_blk, n_blocks,
                       words, mask, nullptr, nullptr, 0u);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int scn_keep_mask_units(int32_t n, int32_t ns, const int32_t* node, int32_t n_nodes, const int32_t* top_ptr, const int32_t* top_blk,
                        int32_t n_blocks, uint32_t* mask, uint32_t* units, int64_t capacity, void* stream) {
    if (!units) return scn_keep_mask(n, ns, node, n_nodes, top_ptr, top_blk, n_blocks, mask, stream);
    if (!node || !top_ptr || !top_blk || !mask) return SCN_ERR_BAD_ARG;
    if (n <= 0 || ns <= 0 || n_nodes <= 0 || n_blocks <= 0) return SCN_ERR_BAD_SHAPE;
    const int n_slabs = (n + ns - 1) / ns, words = (n_slabs + 31) / 32;
    const int64_t n_words = (int64_t)n_blocks * words;
    if (n_words > INT32_MAX) return SCN_ERR_UNSUPPORTED;                  // (an entry and the count are 32-bit)
    if (capacity < n_words) return SCN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    // one memset clears the mask and the SCN_UNIT_COUNTERS words behind it; the first of them counts this mask's entries
    SCN_HIP_TRY(hipMemsetAsync(mask, 0, sizeof(uint32_t) * (size_t)(n_words + SCN_UNIT_COUNTERS), st));
    hipLaunchKernelGGL(keep_mask_kernel<true>, dim3((n + 255) / 256), dim3(256), 0, st, n, ns, node, n_nodes, top_ptr, top_blk, n_blocks,
                       words, mask, units, mask + n_words, (uint32_t)std::min<int64_t>(capacity, INT32_MAX));
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int scn_mask_hop(int32_t n_blocks, int32_t words, const int32_t* adj_ptr, const int32_t* adj_blk, const uint32_t* in, uint32_t* out,
                 void* stream) {
    if (!adj_ptr || !adj_blk || !in || !out || in == out) return SCN_ERR_BAD_ARG;
    if (n_blocks <= 0 || words <= 0) return SCN_ERR_BAD_SHAPE;
    const int64_t n = (int64_t)n_blocks * words;
    hipLaunchKernelGGL(mask_hop_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_blocks, words,
                       adj_ptr, adj_blk, in, out, nullptr, nullptr, 0u);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int scn_mask_hop_units(int32_t n_blocks, int32_t words, const int32_t* adj_ptr, const int32_t* adj_blk, const uint32_t* in, uint32_t* out,
                       uint32_t* units, uint32_t* unit_count, int64_t capacity, void* stream) {
    if (!units && !unit_count) return scn_mask_hop(n_blocks, words, adj_ptr, adj_blk, in, out, stream);
    if (!adj_ptr || !adj_blk || !in || !out || in == out || !units || !unit_count) return SCN_ERR_BAD_ARG;
    if (n_blocks <= 0 || words <= 0) return SCN_ERR_BAD_SHAPE;
    const int64_t n = (int64_t)n_blocks * words;
    if (n > INT32_MAX) return SCN_ERR_UNSUPPORTED;                        // (an entry and the count are 32-bit)
    if (capacity < n) return SCN_ERR_WORKSPACE;
    hipLaunchKernelGGL(mask_hop_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_blocks, words,
                       adj_ptr, adj_blk, in, out, units, unit_count, (uint32_t)std::min<int64_t>(capacity, INT32_MAX));
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int64_t scn_cone_masks_max_words(void) { return SCN_CONE_MASKS_MAX_WORDS; }

int scn_cone_masks(int32_t n_mb, const scn_cone_mb* mb, int32_t ns, int32_t n_nodes, int32_t n_blocks, const int32_t* top_ptr,
                   const int32_t* top_blk, const int32_t* adj_ptr, const int32_t* adj_blk, int32_t L, void* stream) {
    return cone_masks_run<ConeNoVisits>(n_mb, mb, nullptr, ns, n_nodes, n_blocks, top_ptr, top_blk, adj_ptr, adj_blk, L, nullptr, nullptr,
                                        stream);
}

int scn_cone_masks_visits(int32_t n_mb, const scn_cone_mb* mb, uint32_t* const* visits, int32_t ns, int32_t n_nodes, int32_t n_blocks,
                          const int32_t* top_ptr, const int32_t* top_blk, const int32_t* adj_ptr, const int32_t* adj_blk, int32_t L,
                          const int32_t* const* visit_ptr, const int32_t* const* visit_blk, void* stream) {
    return cone_masks_run<ConeVisitArgs>(n_mb, mb, visits, ns, n_nodes, n_blocks, top_ptr, top_blk, adj_ptr, adj_blk, L, visit_ptr,
                                         visit_blk, stream);
}

int scn_node_readout_forward(int32_t n_slabs, int32_t ns, int32_t n_nodes, const float* nodes_out,
                             const int32_t* nbr, int32_t max_deg, const int32_t* last_nodes, float* logits,
                             float* logp, void* stream) {
    if (!nodes_out || !nbr || !last_nodes || !logits || !logp) return SCN_ERR_BAD_ARG;
    if (n_slabs <= 0 || ns <= 0 || n_nodes <= 0 || max_deg <= 0) return SCN_ERR_BAD_SHAPE;
    if (max_deg > RO_WIDE) return SCN_ERR_UNSUPPORTED;
    if (max_deg > RO_MAXD)
        hipLaunchKernelGGL(node_readout_fwd_wide_kernel, dim3(n_slabs * ns), dim3(64), 0, (hipStream_t)stream, ns, n_nodes,
                           nodes_out, nbr, max_deg, last_nodes, logits, logp);
    else
        hipLaunchKernelGGL(node_readout_fwd_kernel, dim3(n_slabs * ns), dim3(64), 0, (hipStream_t)stream, ns, n_nodes,
                           nodes_out, nbr, max_deg, last_nodes, logits, logp);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int scn_node_readout_backward(int32_t n_slabs, int32_t ns, int32_t n_nodes, const float* nodes_out,
                              const int32_t* nbr, int32_t max_deg, const int32_t* last_nodes, const float* d_logp,
                              const float* logp, int32_t act, float* dz, void* stream) {
    if (!nodes_out || !nbr || !last_nodes || !d_logp || !logp || !dz) return SCN_ERR_BAD_ARG;
    if (n_slabs <= 0 || ns <= 0 || n_nodes <= 0 || max_deg <= 0) return SCN_ERR_BAD_SHAPE;
    if (max_deg > RO_WIDE) return SCN_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const int N = n_slabs * ns;
    SCN_HIP_TRY(hipMemsetAsync(dz, 0, sizeof(float) * (size_t)N * n_nodes, st));
    if (max_deg > RO_MAXD)
        hipLaunchKernelGGL(node_readout_bwd_wide_kernel, dim3(N), dim3(64), 0, st, ns, n_nodes, nodes_out, nbr, max_deg,
                           last_nodes, d_logp, logp, act, dz);
    else
        hipLaunchKernelGGL(node_readout_bwd_kernel, dim3(N), dim3(64), 0, st, ns, n_nodes, nodes_out, nbr, max_deg,
                           last_nodes, d_logp, logp, act, dz);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int scn_scatter_flows(int32_t n_slabs, int32_t ns, int32_t n_edges, int64_t n_entries, const int32_t* sample_of,
                      const int32_t* edge_idx, const float* val, float* x, void* stream) {
    if (n_slabs <= 0 || ns <= 0 || n_edges <= 0 || n_entries < 0) return SCN_ERR_BAD_SHAPE;
    if (!x || (n_entries > 0 && (!sample_of || !edge_idx || !val))) return SCN_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    SCN_HIP_TRY(hipMemsetAsync(x, 0, sizeof(float) * (size_t)n_slabs * n_edges * ns, st));
    if (n_entries) {
        hipLaunchKernelGGL(scatter_flows_kernel, dim3((unsigned)((n_entries + 255) / 256)), dim3(256), 0, st, ns,
                           n_edges, n_entries, sample_of, edge_idx, val, x);
        SCN_LAUNCH_CHECK();
    }
    return SCN_OK;
}

// Host-only: one batch of ragged flows, last nodes and targets into the caller's (pinned) staging words -- what a graph-replayed step
// copies to the device in ONE transfer.  Plain loops: the same assembly in NumPy was 85 us of a 155 us optimiser step on the
// reference's own configuration (a dozen array calls on ~1000 elements each).
int64_t scn_host_stage_batch(int32_t m, const int32_t* traj, int32_t n_total, const int64_t* ptr, const int32_t* edge, const float* val,
                             const int32_t* last_nodes, const float* y, int32_t d, double total, int32_t e_cap,
                             int32_t n_cap, int32_t* out) {
    if (m < 0 || n_total < 0 || d <= 0 || e_cap <= 0 || n_cap <= 0 || !(total > 0.0)) return SCN_ERR_BAD_SHAPE;
    if (!out || (m > 0 && (!traj || !ptr || !edge || !val || !last_nodes || !y))) return SCN_ERR_BAD_ARG;
    if (m > n_cap) return SCN_ERR_UNSUPPORTED;
    for (int32_t j = 0; j < m; ++j)
        if (traj[j] < 0 || traj[j] >= n_total) return SCN_ERR_BAD_ARG;          // an index outside the data set: nothing is read
    int64_t k = 0;
    for (int32_t j = 0; j < m; ++j) k += ptr[traj[j] + 1] - ptr[traj[j]];
    if (k > e_cap) return SCN_ERR_UNSUPPORTED;
    const size_t n_words = (size_t)3 * e_cap + n_cap + (size_t)n_cap * d;
    std::memset(out, 0, n_words * sizeof(int32_t));
    int32_t* sample = out;
    int32_t* eidx = out + e_cap;
    float* v = (float*)(out + 2 * (size_t)e_cap);
    int32_t* last = out + 3 * (size_t)e_cap;
    float* yo = (float*)(out + 3 * (size_t)e_cap + n_cap);
    int64_t o = 0;
    for (int32_t j = 0; j < m; ++j) {
        const int32_t n = traj[j];
        for (int64_t t = ptr[n]; t < ptr[n + 1]; ++t, ++o) {
            sample[o] = j;
            eidx[o] = edge[t];
            v[o] = val[t];
        }
        last[j] = last_nodes[n];
        for (int32_t c = 0; c < d; ++c) yo[(size_t)j * d + c] = (float)((double)y[(size_t)n * d + c] / total);
    }
    return k;
}

int scn_logits_sum_log_softmax(int32_t n_traj, int32_t max_deg, int32_t n_parts, const float* const* logits_parts, float* logits,
                               float* logp, void* stream) {
    if (n_traj <= 0 || max_deg <= 0 || n_parts <= 0 || n_parts > 4) return SCN_ERR_BAD_SHAPE;
    if (!logits_parts || !logits || !logp) return SCN_ERR_BAD_ARG;
    LogitParts L{};
    for (int k = 0; k < n_parts; ++k) {
        if (!logits_parts[k]) return SCN_ERR_BAD_ARG;
        L.p[k] = logits_parts[k];
    }
    hipLaunchKernelGGL(logits_sum_log_softmax_kernel, dim3(n_traj), dim3(64), 0, (hipStream_t)stream, max_deg, n_parts, L, logits, logp);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int scn_masked_ce(int64_t n, const float* logp, const float* y, float scale, float* d_logp, double* loss, void* stream) {
    if (n <= 0) return SCN_ERR_BAD_SHAPE;
    if (!logp || !y || !d_logp || !loss) return SCN_ERR_BAD_ARG;
    hipLaunchKernelGGL(masked_ce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, n, logp, y, scale, d_logp, loss);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int scn_masked_ce_begin(int64_t n, const float* logp, const float* y, float scale, float* d_logp, double* loss, int32_t overwrite,
                        float* zero_buf, int64_t zero_n, void* stream) {
    if (n <= 0 || zero_n < 0) return SCN_ERR_BAD_SHAPE;
    if (!logp || !y || !d_logp || !loss || (zero_n > 0 && !zero_buf)) return SCN_ERR_BAD_ARG;
    hipLaunchKernelGGL(masked_ce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, n, logp, y, scale, d_logp, loss, overwrite ? 1 : 0,
                       zero_buf, zero_n);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int scn_adam_step(int64_t n, float* w, const float* g, float* m, float* v, float lr, float b1, float b2, float eps,
                  int32_t step_i, float weight_decay, float g_scale, void* stream) {
    if (n <= 0 || step_i < 0) return SCN_ERR_BAD_SHAPE;
    if (!w || !g || !m || !v) return SCN_ERR_BAD_ARG;
    float c1, c2;
    adam_corrections(b1, b2, step_i, c1, c2);            // (as the kernels that read the index from device memory: the same bits)
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, w, g, m,
                       v, lr, b1, b2, eps, c1, c2, 2.f * weight_decay, g_scale);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int scn_adam_step_dev(int64_t n, float* w, const float* g, float* m, float* v, float lr, float b1, float b2, float eps,
                      int32_t* step_dev, float weight_decay, float g_scale, void* stream) {
    if (n <= 0) return SCN_ERR_BAD_SHAPE;
    if (n > SCN_ADAM_DEV_MAX) return SCN_ERR_UNSUPPORTED;
    if (!w || !g || !m || !v || !step_dev) return SCN_ERR_BAD_ARG;
    hipLaunchKernelGGL(adam_dev_kernel, dim3(1), dim3(ADAM_DEV_THREADS), 0, (hipStream_t)stream, n, w, g, m, v, lr, b1, b2, eps,
                       step_dev, 2.f * weight_decay, g_scale);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

}  // extern "C"
