/*
 * scone_hip.h -- C-ABI of libscone_hip.so: the MI355X (gfx950) implementation of SCoNe's
 * Hodge-Laplacian convolution hot path.
 *
 * The reference (nglaze00/SCoNe_GCN) has no FFI: the path is plain Python/JAX.  Each entry point below
 * names the reference code it replaces (TE = trajectory_analysis/trajectory_experiments.py,
 * STM = trajectory_analysis/scone_trajectory_model.py).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every function returns an int status: 0 = SCN_OK, negative = error (scn_error_string()).
 *     No C++ exception crosses this boundary.
 *   - "device" pointers are HIP device memory owned by the CALLER (PyTorch-ROCm tensors in the host
 *     mirror); the library never allocates per call.  Handles own only the device copies of the index /
 *     value arrays made at create time and are immutable afterwards (shareable across streams).
 *   - all launches go to the caller's stream (hipStream_t passed as void*; NULL = default stream) and
 *     never synchronise.
 *
 * Activation layout ("flow slabs"): fp32 [n_slabs][n_rows][ns][c] row-major.  A slab holds ns
 * trajectories; row r of slab s is the contiguous piece of ns*c floats at ((s*n_rows + r)*ns)*c.
 * The reference's batched (N, E, C) tensor (vmap axis 0, STM:256) maps to slab = n / ns, sample = n % ns.
 */
#ifndef SCONE_HIP_H
#define SCONE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCN_OK               0
#define SCN_ERR_BAD_ARG     -1
#define SCN_ERR_BAD_SHAPE   -2
#define SCN_ERR_HIP         -3
#define SCN_ERR_UNSUPPORTED -4
#define SCN_ERR_NOMEM       -5
#define SCN_ERR_WORKSPACE   -6
#define SCN_ERR_INTERNAL    -7   /* a self-check of the library failed (scn_plan_gather_stats: the block layout lost or moved an entry) */

/* activation codes (TE:124-134) */
#define SCN_ACT_NONE        0
#define SCN_ACT_TANH        1   /* scone   TE:149 */
#define SCN_ACT_RELU        2   /* bunch   TE:195 */
#define SCN_ACT_LEAKY_RELU  3   /* ebli    TE:167, slope 0.01, x >= 0 */

#define SCN_MAX_GROUPS 3
#define SCN_MAX_SLOTS  4

int         scn_version(void);
const char* scn_error_string(int status);
/* last HIP error text captured by a failing call on this thread ("" if none) */
const char* scn_last_hip_error(void);

/* ---------------------------------------------------------------------------------------------------
 * Shift-convolution operator: everything that feeds ONE output level of one layer.
 *
 *   out[s,r,n,:] = act( sum_over_slots  ( sum_j val_slot[r,j] * src_g[s, col[r,j], n, :] ) @ W_slot )
 *
 * A group g is one source tensor + one CSR pattern (n_rows x n_cols) carrying 1 or 2 value arrays and,
 * optionally, an identity shift.  Weight slots are numbered group by group: [identity][val0][val1].
 *   scone / ebli layer (TE:145-147 / 163-165): 1 group, identity + {S_lower, S_upper} on their shared
 *       pattern -> slots (W[3i], W[3i+1], W[3i+2]).
 *   bunch node / edge / face level (TE:184-192): 2 / 3 / 2 groups with 1 value array each.
 * Host arrays are copied at create time.
 * --------------------------------------------------------------------------------------------------- */
typedef struct scn_conv_s* scn_conv_t;

typedef struct {
    int32_t        n_cols;    /* rows of this group's source tensor */
    int32_t        identity;  /* 1: also apply the identity shift (needs n_cols == n_rows) */
    int32_t        n_vals;    /* 0, 1 or 2 value arrays on the pattern (0 only with identity) */
    int32_t        reserved;
    int64_t        nnz;
    const int32_t* rowptr;    /* host, n_rows + 1 */
    const int32_t* col;       /* host, nnz, ascending within a row */
    const float*   val0;      /* host, nnz (or NULL when n_vals == 0) */
    const float*   val1;      /* host, nnz (or NULL when n_vals < 2) */
} scn_group_desc;

int scn_conv_create(int32_t n_rows, int32_t n_groups, const scn_group_desc* groups, scn_conv_t* out);
/* Same, with a layout hint: block_start[r] != 0 (host, n_rows bytes, or NULL) forces a block of the LDS-blocked plan to
 * begin at row r (the plan may still cut more often).  Produced by scn_plan_refine_order for the row order it returns. */
int scn_conv_create_blocked(int32_t n_rows, int32_t n_groups, const scn_group_desc* groups,
                            const uint8_t* block_start, scn_conv_t* out);
int scn_conv_destroy(scn_conv_t conv);
int scn_conv_n_slots(scn_conv_t conv);
/* rows per LDS-staged block and mean staged source rows per block of the blocked plan (0 if none) */
int scn_conv_plan_info(scn_conv_t conv, int32_t* n_blocks, float* mean_sources_per_row);

/* Forward of one output level (replaces the body of the layer loops TE:144-149, 162-167, 181-195).
 *   src[g]  device [n_slabs][n_cols_g][ns][c_in[g]]
 *   W[slot] device [c_in(group of slot)][c_out] row-major
 *   out     device [n_slabs][n_rows][ns][c_out]                                                  */
int scn_conv_forward(scn_conv_t conv, int32_t n_slabs, int32_t ns,
                     const float* const* src, const int32_t* c_in,
                     const float* const* W, int32_t c_out, int32_t act,
                     float* out, void* stream);

/* The same with a tensor of partial pre-activations added before the activation:
 *   out[s,r,n,:] = act( partial[s,r,n,:] + sum_over_slots (...) @ W_slot )      partial: device [n_slabs][n_rows][ns][c_out]
 * `partial` may be `out` itself (in place).  This is how a layer wider than 32 channels adds up its (input block, output block)
 * pairs of 32 channels (-hidden_layers takes any width, TE:103-110) without a summation pass of its own: the first pair of an output
 * block runs scn_conv_forward with SCN_ACT_NONE, the last one this entry point with the layer's activation.  Served for one group,
 * c_in = c_out = 32, ns = 4 on an LDS-blocked plan; SCN_ERR_UNSUPPORTED otherwise. */
int scn_conv_forward_accumulate(scn_conv_t conv, int32_t n_slabs, int32_t ns,
                                const float* const* src, const int32_t* c_in,
                                const float* const* W, int32_t c_out, int32_t act,
                                const float* partial, float* out, void* stream);

/* Backward of one INPUT level (what jax.grad generates for the same loops, STM:307).  `conv_t` is the
 * operator whose slots are the TRANSPOSED shifts feeding this input level (for scone's symmetric
 * L_lower / L_upper it is the forward object itself).
 *   dz[g]    device [n_slabs][n_cols_g][ns][c_dz[g]]   grad w.r.t. the pre-activation of output level g
 *   W[slot]  device [c_aux][c_dz(group of slot)]        the FORWARD weights (used transposed)
 *   aux      device [n_slabs][n_rows][ns][c_aux]        this level's forward input (= previous layer's output)
 *   dx       device [n_slabs][n_rows][ns][c_aux] or NULL:
 *               dx = ( sum_slots G_slot @ W_slot^T ) * act'(aux)    with G_slot the gathered dz
 *   dW[slot] device [c_aux][c_dz]   dW_slot += sum_{s,r,n} aux[s,r,n,:]^T G_slot[s,r,n,:]   (deterministic order)
 *   workspace: device scratch of at least scn_conv_backward_workspace() bytes                       */
size_t scn_conv_backward_workspace(scn_conv_t conv_t, int32_t n_slabs, int32_t ns,
                                   const int32_t* c_dz, int32_t c_aux);
int scn_conv_backward(scn_conv_t conv_t, int32_t n_slabs, int32_t ns,
                      const float* const* dz, const int32_t* c_dz,
                      const float* const* W, const float* aux, int32_t c_aux, int32_t act,
                      float* dx, float* const* dW,
                      void* workspace, size_t workspace_bytes, void* stream);

/* The same with a partial input gradient added:  dx = dx_partial + ( sum_slots G_slot @ W_slot^T ) * act'(aux)
 * (dx_partial: device [n_slabs][n_rows][ns][c_aux]; may be `dx` itself).  The backward counterpart of scn_conv_forward_accumulate: the
 * input gradient of an input block of a layer wider than 32 channels is the sum over the layer's output blocks (act' of the layer
 * below is a common factor).  Served for one group, c_dz = c_aux = 32, ns = 4 on an LDS-blocked plan; SCN_ERR_UNSUPPORTED otherwise. */
int scn_conv_backward_accumulate(scn_conv_t conv_t, int32_t n_slabs, int32_t ns,
                                 const float* const* dz, const int32_t* c_dz,
                                 const float* const* W, const float* aux, int32_t c_aux, int32_t act,
                                 const float* dx_partial, float* dx, float* const* dW,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* The two Hodge shifts alone: ya = val0-operator * x, yb = val1-operator * x on group 0 of `conv`
 * (the L_down X / L_up X products of TE:146-147 without the dense part; the SpMM GB/s metric).
 *   x, ya, yb device [n_slabs][rows][k]; yb may be NULL for a single-operator product.               */
int scn_spmm_dual(scn_conv_t conv, int32_t n_slabs, int32_t k,
                  const float* x, float* ya, float* yb, void* stream);

/* Dense contraction over already-gathered terms of one Bunch level (TE:184-195 once the S_k X products exist):
 *   forward : out[p,:] = act( sum_k G[k][p,:] @ W[k] ),  G[k] device [n_points][c_in[k]], W[k] device [c_in[k]][c_out]
 *   backward: dx[p,:] = ( sum_k G[k][p,:] @ W[k]^T ) * act'(aux[p,:]) ; dW[k] += sum_p aux[p,:]^T G[k][p,:]
 *             with G[k] = S_k^T dZ device [n_points][c[k]], W[k] device [c_aux][c[k]] (forward weights), aux = this
 *             level's forward input [n_points][c_aux]; dx may be NULL; deterministic reduction order.
 * n_points counts every (slab, row, trajectory) of the level; n_terms <= 3 (<= 6 when every term is one channel wide). */
int scn_dense_terms_forward(int64_t n_points, int32_t n_terms, const float* const* G, const int32_t* c_in,
                            const float* const* W, int32_t c_out, int32_t act, float* out, void* stream);
size_t scn_dense_terms_backward_workspace(int64_t n_points, int32_t n_terms, const int32_t* c, int32_t c_aux);
int scn_dense_terms_backward(int64_t n_points, int32_t n_terms, const float* const* G, const int32_t* c,
                             const float* const* W, const float* aux, int32_t c_aux, int32_t act, float* dx,
                             float* const* dW, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Readout (TE:151-152 with Bconds_func TE:298-303, B1_jax TE:288, nbrhoods TE:279):
 *   logits[n,d] = sum_{e incident to v} sign(v,e) * (H[e,n,:] . w_last),  v = nbr[last[n]][d];  v = -1 -> 0
 *   logp = logits - logsumexp_d(logits)    over ALL D entries, padding included.
 * inc_* is B1 (optionally flipped, TE:291) as node-major CSR on device.
 * max_deg (the neighbourhood width D = the largest node degree, TE:279) up to 1024: one slot per lane up to 64, LDS-resident slot
 * arrays beyond (hub nodes); SCN_ERR_UNSUPPORTED above 1024.  The same holds for the node readout of the Bunch model below.
 * --------------------------------------------------------------------------------------------------- */
int scn_readout_forward(int32_t n_slabs, int32_t ns, int32_t n_edges, int32_t c,
                        const float* H, const float* w_last,
                        const int32_t* nbr, int32_t n_nodes, int32_t max_deg,
                        const int32_t* last_nodes,
                        const int32_t* inc_ptr, const int32_t* inc_edge, const float* inc_sign,
                        float* bh /* [N][max_deg][c]: Bcond(last) @ H, kept for the backward */,
                        float* logits, float* logp, void* stream);

/* Backward of the readout + log-softmax, fused with the last layer's activation derivative:
 *   d_logits = d_logp - exp(logp) * sum_d d_logp
 *   dz[e,n,:] = (sum_v sign(v,e) d_logits[n,d(v)]) * w_last * act'(H[e,n,:])    (zeros elsewhere)
 *   d_w_last += sum_n sum_d d_logits[n,d] * bh[n,d,:]          (fixed summation order)               */
int scn_readout_backward(int32_t n_slabs, int32_t ns, int32_t n_edges, int32_t c,
                         const float* H, const float* w_last,
                         const int32_t* nbr, int32_t n_nodes, int32_t max_deg,
                         const int32_t* last_nodes,
                         const int32_t* inc_ptr, const int32_t* inc_edge, const float* inc_sign,
                         const int32_t* edge_nodes, /* [n_edges][2] endpoints (tail, head) */
                         const float* bh, const float* d_logp, const float* logp, int32_t act,
                         float* d_logits /* [N][max_deg] out */, float* dz,
                         int32_t dz_is_zero /* 1: caller guarantees dz is all zeros (skips the memset of the dense tensor);
                                               2: dz may hold anything and the launch zeroes it itself, every trajectory's wave its own
                                                  column first (small complexes: no fill over the buffer) */,
                         float* d_w_last, void* stream);

/* Writes zeros to exactly the dz entries scn_readout_backward fills for these last_nodes, so a buffer handed in with
 * dz_is_zero = 1 is all-zero again once the layer above has consumed it (a few hundred rows instead of a full memset). */
int scn_readout_clear_dz(int32_t n_slabs, int32_t ns, int32_t n_edges, int32_t c,
                         const int32_t* nbr, int32_t n_nodes, int32_t max_deg, const int32_t* last_nodes,
                         const int32_t* inc_ptr, const int32_t* inc_edge, const int32_t* edge_nodes,
                         float* dz, void* stream);

/* Bunch readout (TE:198-203): logits[n,d] = nodes_out[nbr[last[n]][d]] with -1 wrapping to the last node. */
int scn_node_readout_forward(int32_t n_slabs, int32_t ns, int32_t n_nodes,
                             const float* nodes_out, const int32_t* nbr, int32_t max_deg,
                             const int32_t* last_nodes, float* logits, float* logp, void* stream);
int scn_node_readout_backward(int32_t n_slabs, int32_t ns, int32_t n_nodes,
                              const float* nodes_out, const int32_t* nbr, int32_t max_deg,
                              const int32_t* last_nodes, const float* d_logp, const float* logp,
                              int32_t act, float* dz, void* stream);

/* The first two Bunch layers without a 32-channel gather (bunch_func, TE:179-195): the model starts from [0, flow, 0], so layer
 * one's output of every level is relu of ONE rank-one term, H1_j[p][:] = relu(g_j[p] w_j) with g_j = S x one channel wide, and
 *   relu(g w) = max(g, 0) relu(w) + min(g, 0) min(w, 0)      =>      (S_k H1_j) W_k = (S_k g_j^+) (relu(w_j) W_k) + (S_k g_j^-) (min(w_j, 0) W_k).
 * scn_split_sign:     g_pos = max(g, 0), g_neg = min(g, 0) elementwise (n floats).
 * scn_fold1_forward:  a_pos[c2] = relu(w1)[c1] @ W2[c1][c2],  a_neg = min(w1, 0) @ W2   -- the rank-one weights of layer two's
 *                     expansion (scn_dense_terms_forward over the shifted scalars S_k g^+, S_k g^-).
 * scn_fold1_backward: given u_pos[c2] = sum_p (S_k g^+)[p] dZ2[p][:] and u_neg likewise (scn_dense_terms_backward with dZ2 as aux),
 *                     dW2[a][c] += relu(w1[a]) u_pos[c] + min(w1[a], 0) u_neg[c],
 *                     dw1[a]    += [w1[a] > 0] (u_pos @ W2^T)[a] + [w1[a] < 0] (u_neg @ W2^T)[a]      (relu'(0) = 0, as everywhere). */
int scn_split_sign(int64_t n, const float* g, float* g_pos, float* g_neg, void* stream);

/* out[i] = act(terms[0][i] + ... + terms[n_terms-1][i]), n floats (a multiple of 4, 16-byte aligned tensors), 1 <= n_terms <= 4, summed
 * in term order; out may be terms[0].  Hidden widths above 32 (-hidden_layers, TE:103-110): a layer of scone_func / ebli_func
 * (TE:143-149) runs as its (input block, output block) pairs of 32 channels on the fused kernels; this adds the partial
 * pre-activations of an output block (forward) and the partial input gradients of an input block (backward, act = none). */
int scn_sum_act(int64_t n, int32_t n_terms, const float* const* terms, int32_t act, float* out, void* stream);
int scn_fold1_forward(const float* w1, const float* W2, int32_t c1, int32_t c2, float* a_pos, float* a_neg, void* stream);
int scn_fold1_backward(const float* w1, const float* W2, const float* u_pos, const float* u_neg, int32_t c1, int32_t c2,
                       float* dW2, float* dw1, void* stream);

/* Scatter ragged edge flows into a zeroed slab tensor [n_slabs][n_edges][ns][1] (the flows_in input,
 * SDG:327-344): x[slab(n)][idx][n % ns] += val (repeated (trajectory, edge) entries accumulate, like the reference's
 * f[k] += 1).  sample_of[i] gives the trajectory of entry i. */
int scn_scatter_flows(int32_t n_slabs, int32_t ns, int32_t n_edges, int64_t n_entries,
                      const int32_t* sample_of, const int32_t* edge_idx, const float* val,
                      float* x, void* stream);

/* HOST-ONLY helper of the launch-amortised step (nothing is launched, no device pointer is touched): assemble one batch for
 * scn_scatter_flows + the readout / loss in the caller's staging words (typically pinned memory, copied to the device in one transfer):
 *   out = [sample_of: e_cap][edge: e_cap][val: e_cap floats][last_nodes: n_cap][y / total: n_cap x d floats], unused words 0
 * from the ragged flows (ptr [N + 1], edge / val per entry; path_to_flow, SDG:327-344), last_nodes [N] and targets y [N][d] of the
 * whole data set of n_total trajectories and the batch's trajectory indices traj [m].  Returns the number of flow entries written,
 * SCN_ERR_UNSUPPORTED when the batch does not fit (m > n_cap or more than e_cap entries), SCN_ERR_BAD_ARG when an index lies outside
 * [0, n_total) (nothing is read through it), or another negative status. */
int64_t scn_host_stage_batch(int32_t m, const int32_t* traj, int32_t n_total, const int64_t* ptr, const int32_t* edge, const float* val,
                             const int32_t* last_nodes, const float* y, int32_t d, double total, int32_t e_cap,
                             int32_t n_cap, int32_t* out);

/* Layers whose second shift is the square of the first (Ebli / SNN: S_lower = L1, S_upper = L1^2, TE:155-167, 251-253) on
 * complexes where the rows of the square no longer fit the LDS-blocked plan.  `conv` holds S alone (identity + ONE value
 * array); the caller forms y = S x (forward) or g1 = S^T dz (backward) with scn_spmm_dual and these calls do the rest:
 *   forward :  out = act(x W[0] + y W[1] + (S y) W[2])                                    x0 = x, x = y below
 *   backward:  dx = (dz W[0]^T + g1 W[1]^T + (S^T g1) W[2]^T) * act'(aux),  dW[k] += aux^T (dz | g1 | S^T g1)
 * All tensors [n_slabs][n_rows][ns][channels]; served for channels = 32 and 16 (16: two slabs per visit, like the plain layers;
 * SCN_ERR_UNSUPPORTED / workspace 0 otherwise). */
int scn_conv_forward_power(scn_conv_t conv, int32_t n_slabs, int32_t ns, const float* x0, const float* x,
                           const float* const* W, int32_t channels, int32_t act, float* out, void* stream);
size_t scn_conv_backward_power_workspace(scn_conv_t conv_t, int32_t n_slabs, int32_t ns, int32_t channels);
int scn_conv_backward_power(scn_conv_t conv_t, int32_t n_slabs, int32_t ns, const float* dz, const float* g1,
                            const float* const* W, const float* aux, int32_t channels, int32_t act, float* dx,
                            float* const* dW, void* workspace, size_t workspace_bytes, void* stream);

/* Zero-skipping mode.  Activations of this path have no bias terms, so a layer's output is exactly zero wherever the
 * one-hop closure of its input's support does not reach; a trajectory batch on a large complex leaves most (block, slab)
 * work items all-zero.  A work list names the items that may be non-zero: listed plan blocks (scn_conv_plan_blocks gives
 * their row ranges) and, per block, the slabs to process.  The *_list entry points compute exactly these items and touch
 * nothing else, so the output / gradient buffers must be all-zero outside them on entry (keep persistent zeroed buffers and
 * wipe the listed items with scn_clear_list after use).  Results equal the dense calls.  All arrays are DEVICE pointers.
 * Served by the LDS-blocked C = 32 kernels (and the first layer); other shapes return SCN_ERR_UNSUPPORTED. */
typedef struct scn_work_list {
    int32_t n_work;          /* listed blocks */
    const int32_t* block;    /* [n_work]     plan block index */
    const int32_t* ptr;      /* [n_work + 1] offsets into slab */
    const int32_t* slab;     /* slabs of each listed block, ascending */
} scn_work_list;

/* first row of every plan block (host array of n_blocks + 1 entries; n_blocks from scn_conv_plan_info) */
int scn_conv_plan_blocks(scn_conv_t conv, int32_t* row0_out);
int scn_conv_forward_list(scn_conv_t conv, int32_t n_slabs, int32_t ns, const float* const* src, const int32_t* c_in,
                          const float* const* W, int32_t c_out, int32_t act, float* out, const scn_work_list* wl,
                          void* stream);
int scn_conv_backward_list(scn_conv_t conv_t, int32_t n_slabs, int32_t ns, const float* const* dz, const int32_t* c_dz,
                           const float* const* W, const float* aux, int32_t c_aux, int32_t act, float* dx,
                           float* const* dW, void* workspace, size_t workspace_bytes, const scn_work_list* wl,
                           void* stream);
/* zero the listed items of a [n_slabs][n_rows][ns][channels] tensor */
int scn_clear_list(scn_conv_t conv, int32_t ns, int32_t channels, float* tensor, const scn_work_list* wl, void* stream);

/* First layer (c_in = 1) fast path.
 * scn_conv_forward_first = scn_conv_forward for one 1-channel input, which also stores the shifted input
 *   y[n_slabs][n_rows][ns][4] = (x, S_val0 x, S_val1 x, 0)  -- the three scalars per point the kernel forms anyway, as
 *   16-byte records.
 * scn_conv_dw_first: weight gradient of that layer (no input gradient) with the shift on the 1-channel side,
 *   dW_slot[0][c] += sum_p y[p][slot] * dz[p][c]   (= what jax.grad of TE:144-149 yields for weights[0:3], STM:307):
 *   dz is read exactly once, coalesced.  Pass the y saved by the forward, or y = NULL and x: it is then recomputed into
 *   the workspace.  `conv` is the FORWARD operator (identity + 2 value arrays) in both calls.
 *   x   device [n_slabs][n_rows][ns][1]      dz  device [n_slabs][n_rows][ns][c_dz]     dW[3] device [1][c_dz], accumulated
 * Both return SCN_ERR_UNSUPPORTED (workspace query: 0) when the operator has no blocked plan or the width is not 16 / 32;
 * callers then use scn_conv_forward / scn_conv_backward. */
int scn_conv_forward_first(scn_conv_t conv, int32_t n_slabs, int32_t ns, const float* x, const float* const* W,
                           int32_t c_out, int32_t act, float* out, float* y_out,
                           const scn_work_list* wl /* NULL: dense */, void* stream);
size_t scn_conv_dw_first_workspace(scn_conv_t conv, int32_t n_slabs, int32_t ns, int32_t c_dz);
int scn_conv_dw_first(scn_conv_t conv, int32_t n_slabs, int32_t ns, const float* x, const float* y, const float* dz,
                      int32_t c_dz, float* const* dW, void* workspace, size_t workspace_bytes,
                      const scn_work_list* wl /* NULL: dense; a list needs y */, void* stream);

/* The first layer's output H1 need not exist in memory.  With out = NULL scn_conv_forward_first writes only y (dense launches),
 * and the layer that follows is computed from y and the first layer's weight rows:
 *   H1[p][c] = act(y[p][0] W_first[0][c] + y[p][1] W_first[1][c] + y[p][2] W_first[2][c])    (16 bytes per point instead of 128)
 * is rebuilt inside the kernels, bit for bit what scn_conv_forward_first stores.
 * scn_conv_forward_from_y                = scn_conv_forward on that H1 (channels = 32, dense launches),
 * scn_conv_backward_fused_first_from_y   = scn_conv_backward_fused_first without `aux` (same workspace, channels = 32).
 * SCN_ERR_UNSUPPORTED for other shapes: store H1 and use the calls above. */
int scn_conv_forward_from_y(scn_conv_t conv, int32_t n_slabs, int32_t ns, const float* y, const float* const* W_first,
                            const float* const* W, int32_t channels, int32_t act, float* out, void* stream);
int scn_conv_backward_fused_first_from_y(scn_conv_t conv_t, int32_t n_slabs, int32_t ns, const float* dz, const float* const* W,
                                         const float* const* W_first, int32_t channels, int32_t act, const float* y,
                                         float* const* dW, float* const* dW_first, void* workspace, size_t workspace_bytes,
                                         const scn_work_list* wl /* NULL: dense */, void* stream);

/* The LAST layer's output is read by the readout alone, and only on the edges incident to a neighbour of each trajectory's last
 * node (scn_readout_forward / scn_readout_backward): a few dozen rows per trajectory.  The *_keep forwards VISIT only the (plan
 * block, slab) items of a keep mask: at 32 channels an item whose bit is clear is not staged, gathered or contracted (at 16 channels,
 * slab pairs, it is computed and dropped), and in either case no row outside the kept items is written; a kept item is computed as
 * the plain calls compute it.  Which items are kept depends on the last nodes, never on a value.
 * scn_keep_mask: leaf i < n belongs to slab i / ns and stands on node[i] (the readout's last_nodes); with the `top` table of
 *   scn_field_lists (node v -> T(v), the plan blocks holding a row the readout of v reads)
 *     mask[n_blocks][words], words = ceil(n_slabs / 32), n_slabs = ceil(n / ns):
 *     bit s & 31 of mask[b][s >> 5] is set iff some leaf i of slab s has b in T(node[i]).
 *   The call zeroes the mask and sets the bits on `stream` (atomic OR; the result does not depend on the order): no allocation, no
 *   synchronisation, no host read.  A node outside [0, n_nodes) is a caller's error that is only guarded against (nothing is read
 *   through it); so is a block outside [0, n_blocks).
 * scn_conv_forward_keep / scn_conv_forward_from_y_keep = scn_conv_forward / scn_conv_forward_from_y with such a mask (device,
 *   geometry as above for the call's n_slabs): the rows of every kept (block, slab) of `out` hold the bits the plain call writes,
 *   every other row of `out` is LEFT UNTOUCHED -- it holds whatever the buffer held.  NOT READ (32 channels): the input of the
 *   items that no kept item stages (item (b', s) is staged by the kept items (b, s) with b' in A(b), the `adj` table of
 *   scn_field_lists).  keep = NULL: every row is stored (the plain call).  With a mask: one group, c_in = c_out = 32 or 16 (from y: 32) on the LDS-blocked plan, and at most 64 slabs per
 *   workgroup of the launch grid (any n_slabs <= 64); SCN_ERR_UNSUPPORTED otherwise, before any launch. */
int scn_keep_mask(int32_t n, int32_t ns, const int32_t* node, int32_t n_nodes, const int32_t* top_ptr, const int32_t* top_blk,
                  int32_t n_blocks, uint32_t* mask, void* stream);
int scn_conv_forward_keep(scn_conv_t conv, int32_t n_slabs, int32_t ns, const float* const* src, const int32_t* c_in,
                          const float* const* W, int32_t c_out, int32_t act, float* out, const uint32_t* keep /* NULL: every row */,
                          void* stream);
int scn_conv_forward_from_y_keep(scn_conv_t conv, int32_t n_slabs, int32_t ns, const float* y, const float* const* W_first,
                                 const float* const* W, int32_t channels, int32_t act, float* out,
                                 const uint32_t* keep /* NULL: every row */, void* stream);

/* The mirror on the backward side: the readout's gradient dz of the LAST layer is non-zero only on the rows the readout reads
 * (scn_readout_backward writes exactly those), so the top layer's backward stages dz only where it was written.  Every
 * (block, slab) item is still visited and dx is still written in full: this is not the zero-skipping mode; which items are staged
 * depends on the last nodes, never on a value.
 * scn_mask_hop: one hop out from a mask of scn_keep_mask's geometry, with the `adj` table of scn_field_lists (block b -> A(b), the
 *   plan blocks block b's rows stage): out[b][w] = OR over b' in A(b) of in[b'][w], for w < words.  in != out.  Every word of `out`
 *   is written by one plain store on `stream`: no atomics, no allocation, no synchronisation, no host read.  A block outside
 *   [0, n_blocks) is only guarded against.  With in = scn_keep_mask's mask, bit (b, s) of out is set wherever some source block of
 *   b holds a row the readout of slab s touches: the SOURCE mask of the backward.
 * scn_conv_backward_dzmask = scn_conv_backward with such a source mask.  CONTRACT: every (block, slab) item of dz[0] whose bit in
 *   the mask that was hopped is clear holds only +-0.  Under it dx, dW and the use of the workspace are bit for bit those of
 *   scn_conv_backward (dx = NULL included).  NOT READ: aux of the items whose bit in dzmask is clear, and dz of the items that no
 *   item with a set bit stages (item (b', s) is staged by the items (b, s) with b' in A(b)).  dzmask = NULL: the
 *   plain call.  With a mask: one group, c_dz = c_aux = 32 on the LDS-blocked plan, dx 16-byte aligned, and at most 64 slabs per
 *   workgroup of the launch grid (any n_slabs <= 64); SCN_ERR_UNSUPPORTED otherwise, before any launch. */
int scn_mask_hop(int32_t n_blocks, int32_t words, const int32_t* adj_ptr, const int32_t* adj_blk, const uint32_t* in, uint32_t* out,
                 void* stream);
int scn_conv_backward_dzmask(scn_conv_t conv_t, int32_t n_slabs, int32_t ns, const float* const* dz, const int32_t* c_dz,
                             const float* const* W, const float* aux, int32_t c_aux, int32_t act, float* dx, float* const* dW,
                             void* workspace, size_t workspace_bytes, const uint32_t* dzmask /* NULL: plain call */, void* stream);

/* The readout's cone.  The argument above does not stop at the top layer: H_l is read by nothing outside M_{L-l} = hop^{L-l}(M0)
 * (M0 = scn_keep_mask's mask, hop = scn_mask_hop), and dZ_l is zero outside it whatever the data are.  The calls below run a layer
 * on such a set only; which items run depends on the last nodes, never on a value.  Masks have scn_keep_mask's geometry for the
 * call's n_slabs; all need the LDS-blocked plan and ns = 4, and (except scn_clear_mask) at most 64 slabs per workgroup of the launch
 * grid (any n_slabs <= 64): SCN_ERR_UNSUPPORTED otherwise, before any launch.
 * scn_conv_backward_visit = scn_conv_backward that VISITS only the items of the mask `visit` (V), on scn_conv_backward's launch
 *   grid and in its slab order.  CONTRACT: every (block, slab) item of dz[0] that some item of V stages (item (b', s) is staged by
 *   (b, s) with b' in A(b), the `adj` table of scn_field_lists) either was written by the producer of dz or holds only +0, and every
 *   item outside V stages only +0 -- with dz zero outside a mask M, V = scn_mask_hop(M) is such a set.  Under it and finite weights dW
 *   and the use of the workspace are bit for bit scn_conv_backward's on the same dz, and so is dx on V; every other row of dx is LEFT
 *   UNTOUCHED (dx = NULL: none is written).  NOT READ: aux of the items outside V, and dz of the items no item of V stages.
 *   NON-FINITE WEIGHTS: scn_conv_backward_dzmask widens its mask to all ones under a NaN / Inf weight so that dx matches the plain
 *   call; this call cannot (it would write rows its caller keeps zero) and visits V regardless.  What holds then: with V non-empty,
 *   every entry of dW the plain call makes non-finite is non-finite here too (a visited tile contracts zero rows with the Inf).
 *   One group, c_dz = c_aux = 32, dense launches; SCN_ERR_UNSUPPORTED for every other width, SCN_ERR_BAD_ARG for visit = NULL.
 * scn_conv_backward_fused_first_from_y_visit = scn_conv_backward_fused_first_from_y likewise (no dx exists): dW and dW_first bit for
 *   bit under the same contract and finite weights, the same statement under non-finite ones.  NOT READ: y of the items outside V,
 *   dz of the items no item of V stages.  channels = 32, dense launches.
 * scn_conv_shifted_input_keep = scn_conv_forward_first with out = NULL on the items of `keep`: the records y of every kept item are
 *   that call's bits, every other row of y_out is LEFT UNTOUCHED.  x is the input and is read wherever a kept item stages it.
 * scn_clear_mask: +0 over the rows of every item (b, s) whose bit is set in `mask` of a [n_slabs][n_rows][ns][channels] tensor (16-byte
 *   aligned), nothing else is written: plain vector stores, no atomics.  The mask-driven twin of scn_clear_list -- it returns a
 *   pooled all-zero gradient buffer to that state after scn_conv_backward_visit wrote it on `mask`. */
int scn_conv_backward_visit(scn_conv_t conv_t, int32_t n_slabs, int32_t ns, const float* const* dz, const int32_t* c_dz,
                            const float* const* W, const float* aux, int32_t c_aux, int32_t act, float* dx, float* const* dW,
                            void* workspace, size_t workspace_bytes, const uint32_t* visit, void* stream);
int scn_conv_backward_fused_first_from_y_visit(scn_conv_t conv_t, int32_t n_slabs, int32_t ns, const float* dz, const float* const* W,
                                               const float* const* W_first, int32_t channels, int32_t act, const float* y,
                                               float* const* dW, float* const* dW_first, void* workspace, size_t workspace_bytes,
                                               const uint32_t* visit, void* stream);
int scn_conv_shifted_input_keep(scn_conv_t conv, int32_t n_slabs, int32_t ns, const float* x, float* y_out, const uint32_t* keep,
                                void* stream);
/* The two visiting backwards run their units as a pipeline: a unit's prologue fetches the next unit's source rows and its last visit
 * stages the next unit's first slab (csrc/scn_blk_bwd.inc).  scn_conv_visit_prefetch sets that for the launches that follow, for the
 * whole process (on != 0: on, the default; 0: every unit starts with its full prologue; negative: no change), and returns the setting
 * before the call.  Outputs are bit for bit the same either way: a switch for tests and A/B runs. */
int scn_conv_visit_prefetch(int32_t on);
/* With the pipeline on, a unit's top also takes the block's header, its tile widths and the next unit's source range from a packed
 * 32-byte record per block, which the workgroup's window scan has left in LDS for its first 64 live entries (an entry past them: one
 * 32-byte load), and issues all of its loads under one wait (csrc/scn_blk_record.h, csrc/scn_blk_bwd.inc).  scn_conv_visit_records
 * sets that in the same way (on != 0: on, the default; 0: the header from the plan's separate arrays; negative: no change) and
 * returns the setting before the call.  Outputs are bit for bit the same either way. */
int scn_conv_visit_records(int32_t on);
int scn_conv_visit_records_cap(void);   /* the table's entries per scan (64) */
int scn_clear_mask(scn_conv_t conv, int32_t n_slabs, int32_t ns, int32_t channels, float* tensor, const uint32_t* mask, void* stream);

/* Unit lists.  A masked launch hands every workgroup a FIXED share of the plan's blocks, and the launch ends with its busiest
 * workgroup; the items of a cone lie in a few neighbouring blocks per trajectory, so the shares are uneven.  The forward-side launches
 * write items that do not depend on the workgroup that computes them, so they may take their units from one device-wide list of the
 * mask's non-empty words instead: workgroup g of G takes entries g, g + G, g + 2 G, ...  (The visiting backwards sum dW in visit
 * order and keep their shares.)
 * A unit list of a mask[n_blocks][words]: uint32 entries b * words + w, one for every NON-ZERO word mask[b][w], each exactly once, in
 *   no particular order, and their number in a device counter.  capacity (entries the caller's `units` holds) must be at least
 *   n_blocks * words: SCN_ERR_WORKSPACE otherwise, before any launch; SCN_ERR_UNSUPPORTED where n_blocks * words exceeds 2^31 - 1.
 * scn_keep_mask_units = scn_keep_mask that also writes the mask's list.  `mask` then has SCN_UNIT_COUNTERS more words behind its
 *   n_blocks * words, which the call's one memset clears with the mask: word 0 of them receives the count, the others are left zero
 *   for the caller (the counters of the masks hopped from this one).  units = NULL: scn_keep_mask, to the letter (no extra words).
 * scn_mask_hop_units = scn_mask_hop that also writes the list of `out`; *unit_count must be zero on entry (device).  units =
 *   unit_count = NULL: scn_mask_hop, to the letter.  Neither call adds a launch, a memset or a synchronisation.
 * scn_conv_forward_keep_units / scn_conv_forward_from_y_keep_units / scn_conv_shifted_input_keep_units = the calls without _units
 *   with the list of their mask `keep`: the same rows written with the same bits, whatever the order of the entries.  CONTRACT: the
 *   list names every non-zero word of `keep` for the call's n_slabs exactly once (a word left out is not visited, a word named twice
 *   is computed twice).  The list is used where the launch grid has one slab range (n_slabs <= 64 and no slab split); any other launch
 *   walks the workgroups' fixed shares as the call without a list does -- never an error that call would not return.  units =
 *   unit_count = NULL: the call without _units, to the letter; one of them NULL: SCN_ERR_BAD_ARG. */
#define SCN_UNIT_COUNTERS 4
int scn_keep_mask_units(int32_t n, int32_t ns, const int32_t* node, int32_t n_nodes, const int32_t* top_ptr, const int32_t* top_blk,
                        int32_t n_blocks, uint32_t* mask, uint32_t* units /* NULL: scn_keep_mask */, int64_t capacity, void* stream);
int scn_mask_hop_units(int32_t n_blocks, int32_t words, const int32_t* adj_ptr, const int32_t* adj_blk, const uint32_t* in, uint32_t* out,
                       uint32_t* units /* NULL: scn_mask_hop */, uint32_t* unit_count, int64_t capacity, void* stream);
int scn_conv_forward_keep_units(scn_conv_t conv, int32_t n_slabs, int32_t ns, const float* const* src, const int32_t* c_in,
                                const float* const* W, int32_t c_out, int32_t act, float* out, const uint32_t* keep,
                                const uint32_t* units /* NULL: static shares */, const uint32_t* unit_count, void* stream);
int scn_conv_forward_from_y_keep_units(scn_conv_t conv, int32_t n_slabs, int32_t ns, const float* y, const float* const* W_first,
                                       const float* const* W, int32_t channels, int32_t act, float* out, const uint32_t* keep,
                                       const uint32_t* units /* NULL: static shares */, const uint32_t* unit_count, void* stream);
int scn_conv_shifted_input_keep_units(scn_conv_t conv, int32_t n_slabs, int32_t ns, const float* x, float* y_out, const uint32_t* keep,
                                      const uint32_t* units /* NULL: static shares */, const uint32_t* unit_count, void* stream);

/* The masks of a whole step in one launch.  The chain above -- scn_keep_mask_units, then L - 1 scn_mask_hop_units -- depends only on a
 * micro-batch's last nodes, and every micro-batch's last nodes are on the device when a step begins.
 * scn_cone_masks builds that chain for n_mb micro-batches at once, one workgroup each, the mask being read in LDS.  For micro-batch i
 *   (mb[i], a HOST array of device pointers; n > 0 leaves, slab i / ns as in scn_keep_mask, words_i = ceil(ceil(n / ns) / 32),
 *   n_words_i = n_blocks * words_i):
 *     masks    [L][stride]      M0 = scn_keep_mask's mask of (node, n), M_k = scn_mask_hop(M_{k-1}) with the `adj` table, bit for bit;
 *     units    [L][stride]      the unit list of M_k in its first counters[k] entries, ASCENDING; entries at or past the count are not
 *                               written; of a mask only its n_words_i words are;
 *     counters [SCN_UNIT_COUNTERS]   counters[k] = the number of non-zero words of M_k for k < L, 0 for k >= L.
 *   Every word of every mask and every counter is written whatever the buffers held: no memset, no global atomic, no allocation, no
 *   synchronisation, no host read; the launch can be captured.  The guards of scn_keep_mask and scn_mask_hop hold (a node outside
 *   [0, n_nodes), a block outside [0, n_blocks) in either table: nothing is read or written through it).  More than
 *   SCN_CONE_MASKS_MAX_MB micro-batches go out as several launches.
 *   SCN_ERR_UNSUPPORTED, before anything is launched or written, for L > SCN_UNIT_COUNTERS and where some n_words_i exceeds
 *   SCN_CONE_MASKS_MAX_WORDS (one mask has to fit a workgroup's LDS; also what scn_cone_masks_max_words() returns) or 2^31 - 1. */
#define SCN_CONE_MASKS_MAX_WORDS 39936   /* 39 x 1024: 156 KB of a compute unit's 160 */
#define SCN_CONE_MASKS_MAX_MB 64         /* micro-batches per launch (the table travels in the kernel's arguments) */
typedef struct {
    const int32_t* node;     /* device: the micro-batch's last nodes */
    int32_t n;               /* ... and their number */
    int32_t stride;          /* words from one mask (and list) to the next, at least n_words_i: SCN_ERR_WORKSPACE below, L > 1 */
    uint32_t* masks;         /* device, the three outputs */
    uint32_t* units;
    uint32_t* counters;
} scn_cone_mb;
int scn_cone_masks(int32_t n_mb, const scn_cone_mb* mb, int32_t ns, int32_t n_nodes, int32_t n_blocks, const int32_t* top_ptr,
                   const int32_t* top_blk, const int32_t* adj_ptr, const int32_t* adj_blk, int32_t L, void* stream);
int64_t scn_cone_masks_max_words(void);
/* Visit masks.  dZ_L is non-zero only on the rows R0 the readout's backward writes, so layer l's backward gathers non-zero values only
 * on R_k = P^k R0, k = L - l + 1 (P: the pattern its rows read, diagonal included): a (block, slab) item of M_k with no row in R_k
 * stages only +0, and a visiting backward may leave it out.  V_k = the items holding a row of R_k, a subset of M_k, is a keep mask
 * against a table of its own, T_k: node v -> the blocks holding a row of P^k rows(v) (rows(v): behind `top`; the caller builds T_k).
 * scn_cone_masks_visits = scn_cone_masks -- the same masks, lists and counters, bit for bit -- whose launch also writes, for micro-batch
 *   i, visits[i] [L - 1][stride]: V_1 .. V_{L-1}, V_k = scn_keep_mask's mask of (node, n) against (visit_ptr[k - 1], visit_blk[k - 1])
 *   (HOST arrays of L - 1 device tables, n_nodes + 1 and visit_ptr[.][n_nodes] entries; visits: a HOST array of n_mb device pointers;
 *   none of the three is read for L = 1).  Every word of every V_k is written: no memset; no lists; no launch more than scn_cone_masks.
 *   The same guards and the same refusals, before anything is launched or written. */
int scn_cone_masks_visits(int32_t n_mb, const scn_cone_mb* mb, uint32_t* const* visits, int32_t ns, int32_t n_nodes, int32_t n_blocks,
                          const int32_t* top_ptr, const int32_t* top_blk, const int32_t* adj_ptr, const int32_t* adj_blk, int32_t L,
                          const int32_t* const* visit_ptr, const int32_t* const* visit_blk, void* stream);

/* Diagnostic, like scn_conv_plan_blocks; no step uses it.  The masked launches above do not walk a workgroup's units one at a time:
 * ahead of the block loop a workgroup fetches the blocks and the mask windows of its units in batches and keeps, in order, the units
 * whose window is non-zero.  scn_window_scan_probe runs that same device helper on grid_x workgroups (a multiple of 8, at least 8)
 * for the slab range [slab0, slab0 + n_it) of a mask of scn_keep_mask's geometry (1 <= n_it <= 64, slab0 < n_slabs) and writes what
 * each workgroup g would visit: out_count[g] = the length of its sequence, out_block / out_window [g * cap + i] = the plan block and
 * the window (bit j = slab slab0 + j, cut to n_it bits, never zero) of its i-th entry for i < min(out_count[g], cap).
 * unit_block (NULL: not wanted) receives the launch's unit -> block table [n_blocks] (the cost-balanced assignment of that grid, or the
 * identity where the grid has none): workgroup g owns the units first + k * (grid_x / 8) < last of XCD range g % 8. */
int scn_window_scan_probe(scn_conv_t conv, int32_t n_slabs, const uint32_t* mask, int32_t grid_x, int32_t slab0, int32_t n_it, int32_t cap,
                          int32_t* out_block, uint64_t* out_window, int32_t* out_count, int32_t* unit_block, void* stream);

/* Backward of the layer that FOLLOWS the first one, fused with the first layer's weight gradient (what jax.grad of TE:144-149
 * yields for weights[0:6], STM:307, in one pass):
 *   this layer :  dW[slot] += aux^T G_slot                       (as scn_conv_backward; aux = the first layer's output)
 *   first layer:  dW_first[slot][0][c] += sum_p y[p][slot] * dx[p][c],   dx = (sum_slots G_slot W_slot^T) * act'(aux)
 * dx -- the gradient w.r.t. the first layer's pre-activation, whose only consumer is that weight gradient -- stays in
 * registers and is never written: no [n_slabs][n_rows][ns][channels] tensor, no second pass over it.
 * `conv_t` as in scn_conv_backward; y from scn_conv_forward_first; channels = 32 (SCN_ERR_UNSUPPORTED / workspace 0
 * otherwise: use scn_conv_backward + scn_conv_dw_first).  A work list names the items of dz's support, as usual. */
size_t scn_conv_backward_fused_first_workspace(scn_conv_t conv_t, int32_t n_slabs, int32_t ns, int32_t channels);
int scn_conv_backward_fused_first(scn_conv_t conv_t, int32_t n_slabs, int32_t ns, const float* dz, const float* const* W,
                                  const float* aux, int32_t channels, int32_t act, const float* y, float* const* dW,
                                  float* const* dW_first, void* workspace, size_t workspace_bytes,
                                  const scn_work_list* wl /* NULL: dense */, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Fused Bunch (SCCONV) layer, TE:173-195: the seven shifts S_ab as ONE square operator on the concatenated row space
 * [nodes | edges | faces] (an index space only: the three level tensors stay separate allocations).  Entry (r, c) carries
 * TERM = the level of column c; row r has CLASS = its own level; level_row0[l] = first concatenated index of level l
 * (level_row0[0] = 0, level_row0[3] = n_rows).  Weights are addressed [class][term] (9 pointers, NULL = the class has no such
 * term: nodes have no face term, faces no node term).
 *   scn_terms_forward :  out_l = act( sum_j (S_{j->l} x_j) W[l][j] )   -- one launch for the three levels of a layer
 *       x[j]   device [n_slabs][rows_j][ns][32] or NULL (level identically zero)
 *       out[l] device [n_slabs][rows_l][ns][32] or NULL (level not wanted: skipped)
 * Served for ns = 4, 32 -> 32 channels (SCN_ERR_UNSUPPORTED otherwise: use the per-shift scn_spmm_dual + scn_dense_terms_*).
 * The handle is a scn_conv_t (scn_conv_destroy frees it).
 * --------------------------------------------------------------------------------------------------- */
int scn_terms_create(int32_t n_rows, const int32_t* rowptr, const int32_t* col, const float* val, const uint8_t* term,
                     const int32_t* level_row0 /* [4] */,
                     const uint8_t* merged /* [n_rows]: level of the i-th simplex along ONE locality curve through all three
                                              levels (each level's rows in their own order): blocks are patches along it */,
                     const int32_t* bins /* [3]: rows of each level a block may hold; multiples of rows_per_wave, sum <= 64; 0 = that level's rows belong to no block (its output is never asked for) */,
                     int32_t rows_per_wave /* 4: plan for scn_terms_forward, 8: for scn_terms_backward */, scn_conv_t* out);
int scn_terms_forward(scn_conv_t op, int32_t n_slabs, int32_t ns, const float* const* x /* [3] */,
                      const float* const* W /* [9] = [class][term], each [32][32] */, int32_t channels, int32_t act,
                      float* const* out /* [3] */, void* stream);

/* Backward of the fused Bunch layer on the TRANSPOSED operator (rows = the layer's INPUT rows of every level, terms = the levels
 * a row feeds; a plan created with rows_per_wave = 8):
 *   dx_l = ( sum_j (S_{l->j}^T dz_j) W[l][j]^T ) * act'(aux_l),    dW[l][j] += aux_l^T (S_{l->j}^T dz_j)
 *   dz[j]  device [n_slabs][rows_j][ns][32] or NULL (no gradient reaches level j)
 *   aux[l] device: the layer's forward input of level l, or NULL (level was identically zero: nothing is computed for it)
 *   dx[l]  device or NULL (input gradient of level l not wanted; its weight gradients are still accumulated)
 *   W / dW: [class l][term j] = the FORWARD weight of the shift from level l to level j ([32][32], used transposed) / its gradient
 *           (accumulated, fixed summation order), NULL where the shift does not exist. */
size_t scn_terms_backward_workspace(scn_conv_t op_t, int32_t n_slabs, int32_t ns, int32_t channels);
int scn_terms_backward(scn_conv_t op_t, int32_t n_slabs, int32_t ns, const float* const* dz /* [3] */,
                       const float* const* W /* [9] */, const float* const* aux /* [3] */, int32_t channels, int32_t act,
                       float* const* dx /* [3] */, float* const* dW /* [9] */, void* workspace, size_t workspace_bytes,
                       void* stream);
/* The same backward for the layer that FOLLOWS the 1-channel first layer of bunch_func (TE:179-195): its input gradient is the
 * gradient of the first layer's pre-activation and is needed for the first layer's weight gradient only, so it is contracted
 * with the first layer's shifted input inside the kernel and never written:
 *   dW_first[l][c] += sum_p y_l[p] * dx_l[p][c],   y_l = S_{1->l} x, device [n_slabs][rows_l][ns] (one float per point) or NULL
 *   dW_first[l] device [32] (the (1, 32) weight of the shift into level l) or NULL.  dW as above; same workspace size. */
int scn_terms_backward_fused_first(scn_conv_t op_t, int32_t n_slabs, int32_t ns, const float* const* dz /* [3] */,
                                   const float* const* W /* [9] */, const float* const* aux /* [3] */, int32_t channels,
                                   int32_t act, const float* const* y /* [3] */, float* const* dW /* [9] */,
                                   float* const* dW_first /* [3] */, void* workspace, size_t workspace_bytes, void* stream);

/* Host-only layout helper (no device work, no reference counterpart: the reference's dense operators, TE:240-257, have
 * no storage order).  For a SQUARE CSR pattern (rows and columns share one index space, e.g. L_lower in device order)
 * returns order[new] = old that sorts the rows of every block the plan would cut by descending entry count, so the
 * 8-row groups a wave walks in lock-step are padded less, and block_start[new] = 1 where those blocks begin.
 * identity != 0: the operator also reads the row itself. */
int scn_plan_refine_order(int32_t n, const int32_t* rowptr, const int32_t* col, int32_t identity, int32_t* order,
                          uint8_t* block_start);

/* Host-only diagnostic (no device work, no reference counterpart): simulated LDS cost of one gather pass over the block plan
 * of a SQUARE operator (pattern as for scn_plan_refine_order; val1, nnz floats or NULL, marks the second operator's entries;
 * block_start as for scn_conv_create_blocked or NULL).  out4[0] = lane-group reads (one per quad of rows and entry position),
 * out4[1] = their LDS cycles with the sources in row order and the entries in CSR order, out4[2] = with the plan's layout
 * (slot colours + entry order, csrc/scn_blk_layout.inc; out4[2] == out4[0] means no bank conflict is left), out4[3] = blocks.
 * Every block's layout is also CHECKED: each row's entries placed exactly once inside its quad's width, second-operator entries
 * inside the leading positions, slots a permutation of the sources -- SCN_ERR_INTERNAL otherwise. */
int scn_plan_gather_stats(int32_t n, const int32_t* rowptr, const int32_t* col, const float* val1, int32_t identity,
                          const uint8_t* block_start, int64_t* out4);

/* The gradient step of a scone_func model (TE:137-152 + the loss of STM:42-56) on a SMALL complex in ONE launch -- the reference's own
 * problem sizes (TE:86-90: |E| = 1001, batch 100).  One workgroup per trajectory keeps that trajectory's activations in LDS through
 * every layer, the readout, the cross-entropy and the whole backward (csrc/scn_small.hip); a second launch sums the per-trajectory
 * weight-gradient partials in trajectory order (bitwise reproducible).  Equivalent to
 *   scn_conv_forward_first, scn_conv_forward x (L - 1), scn_readout_forward, scn_masked_ce, scn_readout_backward,
 *   scn_conv_backward x (L - 2), scn_conv_backward_fused_first
 * on the same buffers:  dW[k] += d/dW[k] of  scale * sum_n <logp_n, y_n>,   loss[0] += scale * sum_n <logp_n, y_n>
 * (overwrite != 0: "=" instead of "+=" for both -- the first micro-batch of a step then needs no zeroing launch before it).
 *   conv / conv_t : the operator (identity + S_lower + S_upper on a shared pattern) and its transpose (the same handle for symmetric shifts)
 *   x [n_slabs][n_edges][ns][1], last_nodes [n_slabs*ns], y [n_slabs*ns][max_deg] (zero rows = padding trajectories)
 *   W / dW : 3 * n_layers + 1 matrices in the reference's order (TE:139-152), first layer (1, hidden), last (hidden, 1)
 *   max_items : caller's bound on sum_d (incident edges of neighbour d) over the neighbourhood of any last node
 * Served (scn_small_step_supported): hidden = 16, 2 <= n_layers <= 6, max_deg <= 64, max_items <= 512 and 128 * |E| + 64 KB of LDS
 * within 160 KB (|E| <= ~1100); SCN_ERR_UNSUPPORTED otherwise -- the caller then runs the layer-by-layer entry points.
 * Like every launch here it neither allocates nor copies nor synchronises: the handle's entry pack (col, val_lower, val_upper per
 * entry) is built by scn_conv_create* for every operator of this shape and size, so the FIRST call on a fresh handle may already be
 * captured into a HIP graph (tests/test_gpu_small_step.py).
 * Paired form: when |E| > 384 (at least two blocks of 128 rows) and 2 * n_traj <= the device's CUs, TWO workgroups share a trajectory:
 * alternating 128-row blocks each, full activations in both LDS, rows handed over through memory after every layer (agent-scope stores,
 * a flag per phase; the wait is bounded -- a partner that never arrives makes the loss and the weight gradients NaN, it cannot hang).  Results are those of the
 * single form up to the order of the weight-gradient sums (2 N partials instead of N), still bitwise reproducible.  The launch assumes
 * it has the device to itself for its ~60 us (all workgroups resident together); scn_small_step_pairing(1) turns the form off
 * process-wide (0: back on, the default).  The workspace size covers both forms. */
int scn_small_step_pairing(int32_t mode);
/* The form a scn_small_step launch of n_traj (= n_slabs * ns) trajectories on this pair of handles takes, from the host function the
 * launch itself selects its kernel instance and LDS layout with.  out[0 .. SCN_SMALL_LAYOUT_FIELDS) (n_out >= that; all zero when
 * out[0] is):
 *   [0] supported (operator and size only; n_layers, hidden, max_deg, max_items are scn_small_step_supported's)
 *   [1] waves per workgroup (12 up to 24 row tiles, else 8)   [2] 16-row tiles per wave   [3] instance: tiles a wave keeps resident
 *   [4] paired (scn_small_step_pairing and the device's CU count included)
 *   [5] n_ovf, [6] n_ovf_t: operator entries past a row's twelfth, of conv and conv_t
 *   [7] ovf_lds: the layout has room for the longer list   [8] y_lds: and for the first layer's shifted input
 *   [9] ovf_in_kernel: the instance reads the tails from the list in LDS (else from memory)
 *   [10] same_t: conv_t is conv   [11] lds_bytes of the launch */
#define SCN_SMALL_LAYOUT_FIELDS 12
int scn_small_step_layout(scn_conv_t conv, scn_conv_t conv_t, int32_t n_traj, int32_t* out, int32_t n_out);
int scn_small_step_supported(scn_conv_t conv, int32_t n_layers, int32_t hidden, int32_t max_deg, int32_t max_items);
size_t scn_small_step_workspace(int32_t n_edges, int32_t n_traj, int32_t n_layers);
int scn_small_step(scn_conv_t conv, scn_conv_t conv_t, int32_t n_slabs, int32_t ns, int32_t n_layers, int32_t hidden,
                   const float* x, const int32_t* last_nodes, const float* y, float scale, const int32_t* nbr, int32_t n_nodes,
                   int32_t max_deg, int32_t max_items, const int32_t* inc_ptr, const int32_t* inc_edge, const float* inc_sign,
                   const float* const* W, int32_t act, float* const* dW, double* loss, int32_t overwrite, void* workspace,
                   size_t workspace_bytes, void* stream);
/* The same step when the batch is ONE micro-batch on ONE rank, ending with the optimiser step: dW[k] = gradient, loss[0] = loss
 * (the overwrite form), and the launch that sums the gradient applies scn_adam_step's update (g_scale = 1) to the weights, which must
 * be ONE flat buffer w_flat with W[k] pointing into it in list order (m_flat / v_flat alike; SCN_ERR_BAD_ARG otherwise).  The step index
 * comes from step_dev[0] as for scn_adam_step_dev (step_dev[1] is scratch: the index in flight); step_dev[0] is advanced.  Bitwise the
 * weights of scn_small_step(overwrite) followed by scn_adam_step_dev. */
int scn_small_step_adam(scn_conv_t conv, scn_conv_t conv_t, int32_t n_slabs, int32_t ns, int32_t n_layers, int32_t hidden,
                        const float* x, const int32_t* last_nodes, const float* y, float scale, const int32_t* nbr, int32_t n_nodes,
                        int32_t max_deg, int32_t max_items, const int32_t* inc_ptr, const int32_t* inc_edge, const float* inc_sign,
                        const float* const* W, int32_t act, float* const* dW, double* loss, void* workspace, size_t workspace_bytes,
                        float* w_flat, float* m_flat, float* v_flat, float lr, float b1, float b2, float eps, int32_t* step_dev,
                        float weight_decay, void* stream);

/* Readout of a last layer kept as channel blocks (hidden widths above 32): logits are linear in H, so the blocks' logits
 * (scn_readout_forward per block with its rows of W_last) are added and normalised here:
 *   logits[n,:] = sum_k logits_parts[k][n,:],   logp = logits - logsumexp_d(logits)   (all D entries, padding included: TE:151-152)
 * n_parts <= 4; logits may be logits_parts[0]. */
int scn_logits_sum_log_softmax(int32_t n_traj, int32_t max_deg, int32_t n_parts, const float* const* logits_parts,
                               float* logits, float* logp, void* stream);

/* Masked cross-entropy of one micro-batch (the data term of STM:54 and its gradient w.r.t. the log-probabilities):
 *   d_logp[i] = y[i] * scale   (scale = -1 / number of trajectories in the GLOBAL batch; padding rows have y = 0)
 *   loss[0]  += sum_i logp[i] * d_logp[i]    (fp64 accumulator on the device, fixed summation order)
 * n = trajectories x max_deg entries of logp / y / d_logp. */
int scn_masked_ce(int64_t n, const float* logp, const float* y, float scale, float* d_logp, double* loss, void* stream);
/* The same as the FIRST loss launch of an optimiser step: overwrite != 0 SETS loss[0] instead of adding to it, and zero_buf (or NULL)
 * -- the flat weight-gradient buffer the backward launches that follow accumulate into, zero_n floats -- is zeroed by the same launch
 * (on the reference's own problem sizes a step is ~15 launches of 5-15 us: two fill launches are a tenth of it). */
int scn_masked_ce_begin(int64_t n, const float* logp, const float* y, float scale, float* d_logp, double* loss,
                        int32_t overwrite, float* zero_buf, int64_t zero_n, void* stream);

/* The tail of a micro-batch in two launches instead of nine (csrc/scn_readout.hip, csrc/scn_step_epilogue.inc).
 *
 * scn_readout_step = scn_readout_forward, the scaling d_logp = y * scale of scn_masked_ce_begin and scn_readout_backward's d_logits
 *   and dz in ONE launch, one wave per trajectory; every output has the separate launches' bits.  dz must be a buffer that is
 *   all-zero (dz_is_zero = 1; every other value is SCN_ERR_UNSUPPORTED, as are max_deg > 64 and c > 64: the caller runs the separate
 *   launches).  zero_buf / zero_n as in scn_masked_ce_begin: zeroed by workgroup 0; nothing else in the launch touches it.  NOT done
 *   here: the loss sum and the readout's weight gradient -- they are jobs of scn_step_epilogue.
 *
 * scn_step_epilogue runs everything a micro-batch deferred, each job the body of its stand-alone kernel on the workgroups that launch
 *   had (a workgroup finds its job by its index, csrc/scn_step_ranges.h; no workgroup waits for another), each result its bits:
 *     loss         loss[0] = overwrite ? s : loss[0] + s, s summed as scn_masked_ce does (loss = NULL: absent)
 *     readout_dw   d_w_last += sum dl x bh as scn_readout_backward's second launch (rd_d_w = NULL: absent)
 *     reduce[k]    the weight-gradient reduce of a backward that left its partials in its workspace (the _partial entries below)
 *     first        the first layer's reduce of scn_conv_backward_fused_first_from_y_visit_partial (first_form: 0 absent, 1: 32 channels)
 *     rc_*         scn_readout_clear_dz (rc_dz = NULL: absent; max_deg <= 64)
 *     clear[k]     scn_clear_mask of one tensor
 *   More than SCN_EPI_MAX_REDUCES / SCN_EPI_MAX_CLEARS jobs, or a job no stand-alone launch would take: an error before any launch.
 *   conv: the operator whose plan the masked clears walk (may be NULL without a masked clear).
 *
 * scn_conv_backward_visit_partial / scn_conv_backward_fused_first_from_y_visit_partial = the entries without the suffix, less their
 *   reduce launches: the workspace keeps the partial sums ([n_wg][c_aux][3 c_dz] at its head; the fused-first form [n_wg][96] behind
 *   [n_wg][3 ch ch]) until a scn_step_epilogue on the same stream has run, and *n_wg_out is the launch's workgroup count. */
#define SCN_EPI_MAX_REDUCES 4
#define SCN_EPI_MAX_CLEARS 4
typedef struct {
    const float* partial;           /* [n_wg][c_aux][3 * c_dz] */
    int32_t n_wg, c_aux, c_dz;
    float* dW[3];
} scn_epi_reduce;
typedef struct {
    float* tensor;                  /* [n_slabs][n_rows][ns][channels], 16-byte aligned */
    const uint32_t* mask;
    int32_t n_slabs, ns, channels;
} scn_epi_clear;
typedef struct {
    /* loss */
    int64_t loss_n; const float* logp; const float* y; float scale; double* loss; int32_t overwrite;
    /* readout_dw */
    int32_t rd_nd, rd_c; const float* rd_dl; const float* rd_bh; float* rd_d_w;
    /* reduces */
    int32_t n_reduce; scn_epi_reduce reduce[SCN_EPI_MAX_REDUCES];
    int32_t first_form; const float* first_partial; int32_t first_n_wg; float* first_dW[3];
    /* the readout gradient's clear */
    int32_t rc_n_slabs, rc_ns, rc_n_edges, rc_c, rc_max_deg; const int32_t* rc_nbr; const int32_t* rc_last_nodes;
    const int32_t* rc_inc_ptr; const int32_t* rc_inc_edge; const int32_t* rc_edge_nodes; float* rc_dz;
    /* masked clears */
    int32_t n_clear; scn_epi_clear clear[SCN_EPI_MAX_CLEARS];
} scn_step_epilogue_desc;
int scn_readout_step(int32_t n_slabs, int32_t ns, int32_t n_edges, int32_t c, const float* H, const float* w_last, const int32_t* nbr,
                     int32_t n_nodes, int32_t max_deg, const int32_t* last_nodes, const int32_t* inc_ptr, const int32_t* inc_edge,
                     const float* inc_sign, const int32_t* edge_nodes, const float* y, float scale, int32_t act, float* bh,
                     float* logits, float* logp, float* d_logp, float* d_logits, float* dz, int32_t dz_is_zero, float* zero_buf,
                     int64_t zero_n, void* stream);
int scn_step_epilogue(scn_conv_t conv, const scn_step_epilogue_desc* desc, void* stream);
/* The two reduces a backward runs behind its kernel, as launches of their own (what the epilogue's jobs are tested against):
 * dW[slot][ca][cc] += sum over n_wg partials [c_aux][3 * c_dz] (a NULL slot is skipped), and the first layer's dW[slot][cc] += sum over
 * n_wg partials [96] (form 1: 32 channels; 2: the slab-pair form, 16). */
int scn_dw_reduce(const float* partial, int32_t n_wg, int32_t c_aux, int32_t c_dz, float* const* dW, void* stream);
int scn_dw_first_reduce(const float* partial, int32_t n_wg, int32_t form, float* const* dW, void* stream);
int scn_conv_backward_visit_partial(scn_conv_t conv_t, int32_t n_slabs, int32_t ns, const float* const* dz, const int32_t* c_dz,
                                    const float* const* W, const float* aux, int32_t c_aux, int32_t act, float* dx, void* workspace,
                                    size_t workspace_bytes, const uint32_t* visit, int32_t* n_wg_out, void* stream);
int scn_conv_backward_fused_first_from_y_visit_partial(scn_conv_t conv_t, int32_t n_slabs, int32_t ns, const float* dz,
                                                       const float* const* W, const float* const* W_first, int32_t channels,
                                                       int32_t act, const float* y, void* workspace, size_t workspace_bytes,
                                                       const uint32_t* visit, int32_t* n_wg_out, void* stream);

/* Fused Adam + ridge step on the flat parameter buffer (jax.experimental.optimizers.adam as driven by
 * STM:300-326; ridge term of STM:54-56):   g' = g * g_scale + 2*weight_decay*w ; m,v EMA ;
 *   w -= lr * (m / (1 - b1^(i+1))) / (sqrt(v / (1 - b2^(i+1))) + eps)                                */
int scn_adam_step(int64_t n, float* w, const float* g, float* m, float* v,
                  float lr, float b1, float b2, float eps, int32_t step_i,
                  float weight_decay, float g_scale, void* stream);
/* The same update with the step index in device memory: reads i = step_dev[0], applies update i, leaves i + 1 in step_dev[0].
 * The launch's arguments do not change from step to step, so it can be captured into a HIP graph behind the gradient launches
 * (scone_trajectory_model.py does, on one rank: the plain launch after a graph replay costs ~8 us of an ~80 us step on the
 * reference's own problem sizes).  One workgroup: n <= SCN_ADAM_DEV_MAX (every model of the reference is far below),
 * SCN_ERR_UNSUPPORTED beyond.  Bitwise the same weights as scn_adam_step(step_i = i). */
#define SCN_ADAM_DEV_MAX 65536
int scn_adam_step_dev(int64_t n, float* w, const float* g, float* m, float* v,
                      float lr, float b1, float b2, float eps, int32_t* step_dev,
                      float weight_decay, float g_scale, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Multi-hop prediction (STM:110-206): the steps between the batched forwards of a greedy rollout or of a probability tree.
 * Step tables (built on the host from the caller's nbrhoods and E_lookup, row-major [n_nodes][d]): step_node = the neighbour in
 * slot j of node v (-1: none), step_edge = the DEVICE row of the edge that step crosses (-1: the pair has no edge), step_sign = the
 * flow value the step sets there (+1 / -1).  deg[v] = number of slots of v that hold a neighbour.  Flow slabs are [S][n_rows][ns][1].
 *
 * scn_hop_select: per trajectory i < n, choice[i] = np.argmax of logp[i][0..d) after slots j >= limit are set to fill (-100 in
 *   STM:116-117; first maximum, a NaN counts as the maximum); limit = n_limit[i], or deg[cur[i]] when n_limit is NULL.  With step_edge == NULL nothing else
 *   happens (final hop).  Otherwise u = step_node[cur[i]][choice[i]] goes to next_node[i] (if not NULL), x[i / ns][e][i % ns] is SET
 *   to step_sign (if x is not NULL, e = step_edge), and with advance != 0 cur[i] = last[i] = u.  A slot without an edge writes
 *   nothing and lowers err[0] to i (atomicMin: the caller initialises it to INT32_MAX).  x holds at least n trajectories. */
int scn_hop_select(int32_t n, int32_t d, const float* logp, const int32_t* n_limit, float fill, const int32_t* deg, int32_t* cur,
                   int32_t* last, int32_t n_nodes, const int32_t* step_node, const int32_t* step_edge, const float* step_sign,
                   int32_t n_rows, int32_t ns, float* x, int32_t advance, int32_t* choice, int32_t* next_node, int32_t* err,
                   void* stream);
/* scn_tree_expand: level h -> h + 1 of a probability tree.  Leaf l (root[l], node[l], prob[l], path_row / path_sign [l][h]) with
 *   log-probabilities logp[l][0..d) gets one child per slot j < deg[node[l]], written at c = offset[l] + j (the exclusive scan of
 *   deg[node], leaf-major and slot-minor): c_root = root[l], c_node = step_node[v][j], c_prob = prob[l] * exp(logp[l][j]),
 *   c_path = path + (step_edge[v][j], step_sign[v][j]) ([c][h + 1]).  A slot without an edge lowers err[0] to l * d + j. */
int scn_tree_expand(int32_t n_leaves, int32_t h, int32_t d, const int32_t* root, const int32_t* node, const float* prob,
                    const int32_t* path_row, const float* path_sign, const float* logp, const int32_t* offset, const int32_t* deg,
                    int32_t n_nodes, const int32_t* step_node, const int32_t* step_edge, const float* step_sign, int32_t n_rows,
                    int32_t n_children, int32_t* c_root, int32_t* c_node, float* c_prob, int32_t* c_path_row, float* c_path_sign,
                    int32_t* err, void* stream);
/* scn_tree_slabs: input slabs x [n_slabs][n_rows][4][1] (16-byte aligned) of n_leaves <= 4 n_slabs leaves: column l = the column
 *   of trajectory root[l] < n_roots of the resident root slabs root_x, then the leaf's path entries SET in level order (the last
 *   write wins; an edge already in the root flow is overwritten).  Columns past n_leaves are zero.  ns must be 4. */
int scn_tree_slabs(int32_t n_leaves, int32_t n_slabs, int32_t h, const int32_t* root, const int32_t* path_row, const float* path_sign,
                   int32_t n_roots, const float* root_x, int32_t n_rows, int32_t ns, float* x, void* stream);
/* scn_tree_target: final level.  out[r] = (sum of prob[l] * exp(logp[l][j]) over the leaves l in [leaf_ptr[r], leaf_ptr[r + 1]) and
 *   slots j < deg[node[l]] with step_node[node[l]][j] == target[r]) / (number of such terms); NaN when there is none (0 / 0,
 *   STM:199-204).  One wave per root, fixed summation order, no atomics: bitwise repeatable. */
int scn_tree_target(int32_t n_roots, const int32_t* leaf_ptr, const int32_t* node, const float* prob, const float* logp, int32_t d,
                    const int32_t* deg, int32_t n_nodes, const int32_t* step_node, const int32_t* target, float* out, void* stream);
/* scn_beam_step: level h -> h + 1 of a beam search.  Entries are root-major with a fixed stride: entry (r, k), k < w_in, of the input
 *   level sits at r * w_in + k and carries node, score (the fp32 sum of the log-probabilities along its path) and, for h > 0, its
 *   path as h (device row, value) pairs (the path_row / path_sign layout of scn_tree_expand); node = -1 marks a dead entry (fewer
 *   than w_in paths exist), and logp[(r * w_in + k)][0..d) is the forward's output for it.  The candidates of root r are every (k, j)
 *   with k live and j < deg[node]; each scores score[k] + logp[k][j] (one fp32 add).  The best w_out of them go to r * w_out + 0 ..
 *   w_out - 1 in this total order: a NaN score before every number (the np.argmax rule of scn_hop_select), then the higher score,
 *   and among equal scores the lower k, then the lower j.  Child o gets c_root = r, c_node = step_node[v][j], c_score, c_parent = k,
 *   c_slot = j and -- unless c_path_row is NULL (final level) -- the parent's path plus (step_edge[v][j], step_sign[v][j])
 *   ([r * w_out + o][h + 1]).  Where fewer than w_out candidates exist the rest are written dead: c_root = c_node = c_parent =
 *   c_slot = -1, c_score = -inf, path rows -1 (scn_tree_slabs writes a zero column for root -1 and skips a row of -1).  Every
 *   candidate of a live entry whose pair has no edge (step_edge < 0 or >= n_rows, or step_node < 0) lowers err[0] to
 *   (r * w_in + k) * d + j (atomicMin; the caller initialises it to INT32_MAX), selected or not.  Such a candidate still takes
 *   its place in the order and, if selected, is written as the tables give it: c_root = r with c_node possibly -1 and a path row
 *   that is -1 or >= n_rows (scn_tree_slabs skips such a row; an entry with node -1 is dead at the next level) -- the caller
 *   reads err and discards the level.  A node id outside [0, n_nodes) other than the -1 of a dead entry is a caller's error the
 *   library only guards against: the entry is treated as dead, nothing is read through it and err is not lowered.  One wave per root, no float
 *   atomics: bitwise repeatable.  The outputs must not overlap the inputs.  w_in, w_out <= SCN_BEAM_MAX (SCN_ERR_UNSUPPORTED
 *   beyond), any d. */
#define SCN_BEAM_MAX 256
int scn_beam_step(int32_t n_roots, int32_t w_in, int32_t w_out, int32_t h, int32_t d, const int32_t* node, const float* score,
                  const int32_t* path_row, const float* path_sign, const float* logp, const int32_t* deg, int32_t n_nodes,
                  const int32_t* step_node, const int32_t* step_edge, const float* step_sign, int32_t n_rows, int32_t* c_root,
                  int32_t* c_node, float* c_score, int32_t* c_parent, int32_t* c_slot, int32_t* c_path_row, float* c_path_sign,
                  int32_t* err, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Sampled paths (Monte-Carlo multi-hop prediction): S samples per root walk the model's own next-node distribution.  A level keeps
 * one entry per DISTINCT path with the number of samples on it, in the layout of the probability tree: entries sorted by root,
 * leaf_ptr[n_roots + 1] the entries of each root (local index k = l - leaf_ptr[r]), an entry = node, score (the fp32 sum of the
 * log-probabilities along its path, one add per hop), its path as h (device row, value) pairs, logp[l][0..d) the forward's output.
 * entry_of[r][s] is the local entry of sample s of root r, -1 for a dropped sample (level 0: all zeros, one entry per root).
 *
 * scn_sample_uniform (host): *u = the uniform of (seed, root r, sample s, hop h): Philox4x32-10 with counter (r, s, h, 0) and key
 *   (seed & 0xffffffff, seed >> 32), u = (out[0] >> 8) * 2^-24 in [0, 1).  The kernels draw the same number: it depends on
 *   (seed, r, s, h) and on nothing else.
 * The slot rule of a sample in an entry on node v with lim = deg[v] live slots: m = the maximum of logp[0..lim) by the rule of
 *   scn_hop_select (first maximum, a NaN counts as the maximum).  If inv_T is +inf (temperature 0) or m is NaN or +-inf, the slot
 *   is that argmax.  Otherwise w_j = expf((logp_j - m) * inv_T) (one fp32 subtract, one fp32 multiply), c_j the fp32 running sum
 *   in slot order, and the slot is the first j with c_j > u * c_{lim-1}; if none (rounding at the top end), the last j with
 *   w_j > 0.  deg[v] == 0 or v outside [0, n_nodes): the sample is dropped and nothing is read through v.
 * scn_sample_draw: level h, one workgroup per root.  pick[r][s] = k * d + j (k = entry_of[r][s], j by the slot rule with the
 *   uniform of (seed, r, s, h)), -1 for a dropped sample; n_child[r] = the number of distinct picks of root r.  Every slot
 *   j < deg of every entry on a valid node whose pair has no edge (step_edge < 0 or >= n_rows, or step_node < 0) lowers err[0] to
 *   (global entry index) * d + j (atomicMin; the caller initialises it to INT32_MAX), drawn or not: the word does not depend on
 *   the seed.
 * scn_sample_expand: child_ptr = the exclusive scan of n_child (the caller's; its total n_children sizes the outputs).  The
 *   children of root r go to child_ptr[r] + rank in ascending pick order (lower parent, then lower slot): c_root = r, c_node =
 *   step_node[v][j], c_score = score[k] + logp[k][j] (one fp32 add), c_parent = k, c_slot = j, c_count = the samples with that pick
 *   and -- unless c_path_row is NULL (final level) -- the parent's path plus (step_edge[v][j], step_sign[v][j]) ([c][h + 1]).
 *   entry_of_next[r][s] = the rank of pick[r][s], -1 for -1.  A child across a pair without an edge is written as the tables give
 *   it (see scn_beam_step); the caller reads err and discards the level.
 * Both: max_entries is the caller's bound on the entries of one root (a root with more, or a leaf_ptr outside [0, n_leaves], is a
 *   caller's error the library only guards against: the excess is ignored and samples in it are dropped).  Integer LDS atomics
 *   only, no float atomics: the same inputs give the same bytes.  The outputs must not overlap the inputs.  Limits
 *   (SCN_ERR_UNSUPPORTED beyond): n_samples <= SCN_SAMPLE_MAX, max_entries * d <= SCN_SAMPLE_PAIRS_MAX (the bits of the (entry,
 *   slot) bitmap a workgroup keeps in LDS: 4096 entries of 32 slots), n_leaves * d and n_roots * n_samples below 2^31 - 1.  n_roots
 *   == 0 returns SCN_OK. */
#define SCN_SAMPLE_MAX 4096
#define SCN_SAMPLE_PAIRS_MAX 131072
int scn_sample_uniform(uint64_t seed, int32_t root, int32_t sample, int32_t hop, float* u);
int scn_sample_draw(int32_t n_roots, int32_t n_samples, int32_t max_entries, int32_t n_leaves, int32_t h, int32_t d, uint64_t seed,
                    float inv_T, const int32_t* leaf_ptr, const int32_t* node, const float* logp, const int32_t* entry_of,
                    const int32_t* deg, int32_t n_nodes, const int32_t* step_node, const int32_t* step_edge, int32_t n_rows,
                    int32_t* pick, int32_t* n_child, int32_t* err, void* stream);
int scn_sample_expand(int32_t n_roots, int32_t n_samples, int32_t max_entries, int32_t n_leaves, int32_t h, int32_t d,
                      const int32_t* leaf_ptr, const int32_t* node, const float* score, const int32_t* path_row, const float* path_sign,
                      const float* logp, const int32_t* pick, const int32_t* child_ptr, int32_t n_children, int32_t n_nodes,
                      const int32_t* step_node, const int32_t* step_edge, const float* step_sign, int32_t* c_root, int32_t* c_node,
                      float* c_score, int32_t* c_parent, int32_t* c_slot, int32_t* c_count, int32_t* c_path_row, float* c_path_sign,
                      int32_t* entry_of_next, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Field-of-view work lists of a multi-hop level, built on the device.  The readout of a leaf reads the last layer only on the
 * edges around the leaf's node, and every layer below needs one more hop of the operator's pattern: with the two block-level CSR
 * tables (host-built once per plan, then device arrays; block indices ascending in every row)
 *   top: node  -> T(v), the plan blocks holding a row the readout of node v reads,
 *   adj: block -> A(b), the plan blocks holding a source row some row of block b stages, b itself included,
 * the lists of the leaves of slab s are  list_L(s) = union of T(node of leaf),  list_l(s) = A(list_{l+1}(s)),  l = L - 1 .. 0.
 * list_l, l >= 1, is the forward work list of layer l and list_0 the blocks of the input that layer 1 stages.  A listed item of
 * layer l + 1 stages rows of listed items of layer l only, so the listed items hold the dense values and nothing else is read.
 *
 * scn_field_lists: leaf i < n belongs to slab i / ns and stands on node[i]; a node < 0 (dead beam entry, padding) contributes
 *   nothing, a node >= n_nodes is a caller's error that is only guarded against (nothing is read through it).  Per level
 *   l < n_levels (n_levels = L + 1: level n_levels - 1 is the top, level 0 the input) the output is a scn_work_list in CANONICAL
 *   order -- listed blocks ascending, blocks without a slab left out, each block's slabs ascending -- in block[l][n_blocks],
 *   ptr[l][n_blocks + 1], slab[l][cap], and counts[l] = (n_work, items).  counts stays on the device (the caller copies it back
 *   once per call).  A level whose items exceed cap gets its counts and nothing else; an empty level likewise.  Integer work only,
 *   no atomics, all launches on `stream`, no allocation and no synchronisation; the same inputs give the same bytes.
 *   SCN_ERR_UNSUPPORTED (workspace query: 0) when n_blocks * n_slabs * n_levels reaches 2^27 - 1, n_slabs = ceil(n / ns) (at least 1).
 * scn_tree_slabs_list: scn_tree_slabs restricted to the items of `wl` (a level-0 list in canonical order, blocks of `conv`'s plan):
 *   for every listed (block, slab) all rows of the block get the slab's 4 columns -- the root's column of root_x, then those of the
 *   leaf's path entries whose (block of the row, slab) is listed, in level order (the last write wins).  Nothing else of x is
 *   written: x may be an UNINITIALISED scratch buffer, because the first layer run with the level-1 list of the same call stages
 *   rows of level-0 items only.  n_rows must be conv's row count, ns 4. */
size_t scn_field_lists_workspace(int32_t n_blocks, int32_t n_slabs, int32_t n_levels);
int scn_field_lists(int32_t n, int32_t ns, const int32_t* node, int32_t n_nodes, const int32_t* top_ptr, const int32_t* top_blk,
                    int32_t n_blocks, const int32_t* adj_ptr, const int32_t* adj_blk, int32_t n_levels, int32_t* block, int32_t* ptr,
                    int32_t* slab, int64_t cap, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int scn_tree_slabs_list(scn_conv_t conv, int32_t n_leaves, int32_t n_slabs, int32_t h, const int32_t* root, const int32_t* path_row,
                        const float* path_sign, int32_t n_roots, const float* root_x, int32_t n_rows, int32_t ns, float* x,
                        const scn_work_list* wl, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * The k-th order Markov baseline (markov_model.py, MM:9-112) on a direct-addressed integer count table.  The graph is the padded
 * neighbour table nbr[n_nodes][d] (a node's neighbours ascending and left-aligned, -1 behind them) with deg[n_nodes] real
 * neighbours per node; slot(a, b) is the position of b in nbr[a][0 .. deg[a]).  A walk of `order` nodes (v0 .. v_{k-1}) is the state
 *     s = ((v0 * d + slot(v0, v1)) * d + slot(v1, v2)) ... * d + slot(v_{k-2}, v_{k-1})           (order 1: s = v0)
 * and counts[rows][d] (int32, rows = n_nodes * d^(order-1)) holds in counts[s][j] how often the walk was followed by the neighbour
 * in slot j of its last node.  MM's weights are counts[s][j] / sum_j counts[s][j]; a state nobody visited is an all-zero row.
 * Orders 1 .. SCN_MARKOV_MAX_ORDER are served while rows * d < 2^31 - 1; SCN_ERR_UNSUPPORTED otherwise, before any launch.
 * Walks and prefixes are ragged: ptr[n + 1] and nodes[ptr[n]], both int32 (so fewer than 2^31 - 1 nodes in all).  n == 0 returns SCN_OK.
 * The err word (the caller initialises it to INT32_MAX) is lowered (atomicMin) to the flat position t in `nodes` of the first
 * consecutive pair (nodes[t], nodes[t + 1]) of one walk that the call reads and that is no edge of the graph or has an id outside
 * [0, n_nodes) -- for an order-1 prefix, whose window has no pair, to the position of its last node if that id is out of range.
 * Nothing is read through such an id.  The prefix calls read the last `order` nodes of a prefix and nothing before them.
 * Integer atomics only, one launch per call on `stream`, no allocation, no synchronisation: the same inputs give the same bytes.
 *
 * scn_markov_table_rows (host): rows of the table, or the negative status above (SCN_ERR_BAD_SHAPE for n_nodes or d <= 0).
 * scn_markov_count: for every walk and every i < len - order: counts[state(walk[i : i + order])][slot(walk[i + order - 1],
 *   walk[i + order])] += 1 (MM:47-51).  It accumulates: the caller zeroes the table.  A walk with len <= order counts nothing, and
 *   so does a window that contains an offending pair.  One wave per walk.
 * scn_markov_rollout: MM:58-93 for all hops in one launch, one wave per prefix i.  At hop h the state is that of the last `order`
 *   nodes (the prefix's, then the predictions'), v the last of them, the row counts[s][0 .. deg[v]); the maxima are the slots equal
 *   to the row's maximum (an all-zero row ties all deg[v] slots, as MM:62-72 does on equal probabilities); with m maxima the
 *   prediction is the ((u24 * m) >> 24)-th of them in slot order, u24 the 24-bit integer behind scn_sample_uniform(seed, i, 0, h).
 *   pred[i][h] = that neighbour's id, n_tied[i][h] = m (MM's was_random: m > 1).  A prefix shorter than `order` predicts nothing
 *   (MM:85 tests the original length): pred = -1, n_tied = 0 at every hop; likewise a prefix with an offending pair, and every hop
 *   from a node of degree 0 on.  hops >= 1.
 * scn_markov_two_target: MM:95-112.  t = the slot of target[i] at the prefix's last node v, o = (u24 * (deg[v] - 1)) >> 24 from the
 *   uniform of (seed, i, 1, 0); the other neighbour is slot o + (o >= t).  score[i] = 1, 0.5 or 0 by comparing the two counts,
 *   other[i] = that neighbour's id.  A target that is no neighbour of v lowers err_target[0] (INT32_MAX at the start) to i.  That
 *   row, a short or offending prefix and a last node with a single neighbour (np.random.choice([]) raises in MM:104) get score 0
 *   and other -1.
 * scn_markov_probs: probs[i][j] (fp64, [n][d]) = (double)counts[s][j] / (double)(sum of the row) -- the bits Python's division
 *   gives -- and 0 where the row is empty, j >= deg[v] or the prefix is short or offending.
 * scn_markov_path_scores: the teacher-forced score of every node of every path, one record per node position in arrays parallel to
 *   path_nodes: prob (fp64), rank, total [T].  The record at t = path_ptr[p] + q describes the prediction of u = nodes[t] from the q
 *   nodes before it, v = nodes[t - 1] the last of them, j = slot(v, u).  The row is counts[state(nodes[t - order .. t - 1])] for
 *   q >= order and the all-zero row for a shorter prefix (scn_markov_probs' rule); c_j' its entries for j' < deg[v]; total = their
 *   sum; prob = ((double)c_j + alpha) / ((double)total + alpha * (double)deg[v]), every operation rounded on its own, where that
 *   denominator is positive and 0 otherwise -- alpha = 0: the bits of scn_markov_probs at slot j; alpha > 0: additive smoothing over
 *   the real neighbours, 1 / deg[v] for an unseen or short state; rank = the number of j' < deg[v] with c_j' > c_j, or c_j' == c_j
 *   and j' < j (scn_path_score's order: rank 0 is the first maximum).  The record's window is the pairs (nodes[r], nodes[r + 1]) for
 *   r = max(t - order, path_ptr[p]) .. t - 1; a pair of one path that is no edge or has an id outside the graph lowers err to its r,
 *   and every record whose window holds such a pair, like every record at q = 0 (which predicts nothing), is prob 0, rank -1, total
 *   0.  alpha negative or NaN is SCN_ERR_BAD_ARG.  One wave per path, 64 positions a pass; the lanes walk their rows themselves, so
 *   a neighbourhood may be wider than a wave.  The library cannot read path_ptr: paths that hold no node at all (T == 0) are the
 *   call with path_nodes, prob, rank and total all NULL, which returns SCN_OK without a launch, as n_paths == 0 does. */
#define SCN_MARKOV_MAX_ORDER 4
int scn_markov_table_rows(int32_t n_nodes, int32_t d, int32_t order);
int scn_markov_count(int32_t n_paths, const int32_t* path_ptr, const int32_t* path_nodes, int32_t order, int32_t n_nodes, int32_t d,
                     const int32_t* nbr, const int32_t* deg, int32_t* counts, int32_t* err, void* stream);
int scn_markov_rollout(int32_t n, const int32_t* prefix_ptr, const int32_t* prefix_nodes, int32_t order, int32_t hops, uint64_t seed,
                       int32_t n_nodes, int32_t d, const int32_t* nbr, const int32_t* deg, const int32_t* counts, int32_t* pred,
                       int32_t* n_tied, int32_t* err, void* stream);
int scn_markov_two_target(int32_t n, const int32_t* prefix_ptr, const int32_t* prefix_nodes, int32_t order, uint64_t seed,
                          const int32_t* target, int32_t n_nodes, int32_t d, const int32_t* nbr, const int32_t* deg,
                          const int32_t* counts, float* score, int32_t* other, int32_t* err, int32_t* err_target, void* stream);
int scn_markov_probs(int32_t n, const int32_t* prefix_ptr, const int32_t* prefix_nodes, int32_t order, int32_t n_nodes, int32_t d,
                     const int32_t* nbr, const int32_t* deg, const int32_t* counts, double* probs, int32_t* err, void* stream);
int scn_markov_path_scores(int32_t n_paths, const int32_t* path_ptr, const int32_t* path_nodes, int32_t order, double alpha,
                           int32_t n_nodes, int32_t d, const int32_t* nbr, const int32_t* deg, const int32_t* counts, double* prob,
                           int32_t* rank, int32_t* total, int32_t* err, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * The variable-order Markov baseline: the count rows of every order 1 .. max_order <= SCN_MARKOV_HASH_MAX_ORDER in one open-addressed
 * hash table, read with back-off to the longest context the table holds.  Graph, walks, states, the err word and the slot order are
 * those of scn_markov_* above.  The key of a walk of k nodes with state s is (uint64)(k - 1) << 59 | s; all-ones is the empty slot.
 * The caller allocates everything: keys[capacity] (uint64, filled with all-ones; capacity a power of two), row_of[capacity] (int32),
 * counts[n_states][d] (int32, zeroed), n_states[1] and n_states_per_order[max_order] (zeroed), err[1] and overflow[1] (INT32_MAX).
 * Before any launch: max_order outside 1 .. SCN_MARKOV_HASH_MAX_ORDER or n_nodes * d^(max_order - 1) >= 2^59 is SCN_ERR_UNSUPPORTED,
 * a capacity that is no power of two, backoff outside {0, 1} and min_count < 1 are SCN_ERR_BAD_ARG; n == 0 returns SCN_OK.
 * A slot is probed at mix(key) & (capacity - 1) and linearly on (wrapping); every probe loop ends after `capacity` slots.  No thread
 * ever waits for another: a slot that holds a key never changes again.  Integer atomics only; row numbers may differ from run to
 * run, no other output does.
 *
 * scn_markov_hash_check (host): the status above for a table of that shape.
 * scn_markov_hash_insert: for every walk, every order k <= max_order and every i < len - k, claims a slot for the key of
 *   walk[i : i + k] (64-bit compare-and-swap).  A window that holds an offending pair, the pair to its next node included, inserts
 *   nothing at any order and lowers err.  A key that finds every slot taken by other keys lowers overflow[0] to its walk's number.
 *   One wave per walk.
 * scn_markov_hash_number: row_of[slot] = a number in [0, n_states) of its own for every slot that holds a key and -1 for the others;
 *   n_states[0] += the keys, n_states_per_order[k - 1] += those of order k.  One thread per slot; capacity < 2^31.
 * scn_markov_hash_count: insert's walk with a lookup: counts[row][slot(walk[i + k - 1], walk[i + k])] += 1.  It accumulates.  A key
 *   the table does not hold counts nothing.
 * The readers are scn_markov_rollout / _two_target / _probs / _path_scores with the row chosen by the context: a position with len
 *   nodes before it (in a window of the last min(len, max_order), which is all the call reads) takes, with backoff = 1, the largest
 *   k <= min(max_order, len) whose key is in the table with a row total (over the deg[v] slots of the last node v) >= min_count;
 *   with backoff = 0 only k = max_order is tried, and a prefix shorter than max_order is short as in scn_markov_*.  used_order = that
 *   k, or 0 where no order qualifies -- the row is then the all-zero row (it ties all neighbours in a rollout, is 0.5 in the 2-target
 *   test, 0 in probs and uniform under alpha > 0) -- and 0 for every row that is short, empty or offending.  The next node never
 *   takes part in the choice.  With backoff = 0 and min_count = 1 every other output has the bits of its scn_markov_* sibling on the
 *   table of order max_order.  used_order is [n][hops] for the rollout (which chooses again at every hop, from the prefix and its own
 *   predictions), [n] for two_target and probs, [T] for path_scores.  One key per wave in rollout and probs, per thread in
 *   two_target; in path_scores lane t looks up the keys of its own position, longest first. */
#define SCN_MARKOV_HASH_MAX_ORDER 8
int scn_markov_hash_check(int32_t n_nodes, int32_t d, int32_t max_order, int64_t capacity);
int scn_markov_hash_insert(int32_t n_paths, const int32_t* path_ptr, const int32_t* path_nodes, int32_t max_order, int32_t n_nodes,
                           int32_t d, const int32_t* nbr, const int32_t* deg, uint64_t* keys, int64_t capacity, int32_t* err,
                           int32_t* overflow, void* stream);
int scn_markov_hash_number(const uint64_t* keys, int64_t capacity, int32_t max_order, int32_t* row_of, int32_t* n_states,
                           int32_t* n_states_per_order, void* stream);
int scn_markov_hash_count(int32_t n_paths, const int32_t* path_ptr, const int32_t* path_nodes, int32_t max_order, int32_t n_nodes,
                          int32_t d, const int32_t* nbr, const int32_t* deg, const uint64_t* keys, const int32_t* row_of,
                          int64_t capacity, int32_t n_states, int32_t* counts, int32_t* err, void* stream);
int scn_markov_hash_rollout(int32_t n, const int32_t* prefix_ptr, const int32_t* prefix_nodes, int32_t max_order, int32_t backoff,
                            int32_t min_count, int32_t hops, uint64_t seed, int32_t n_nodes, int32_t d, const int32_t* nbr,
                            const int32_t* deg, const uint64_t* keys, const int32_t* row_of, int64_t capacity, const int32_t* counts,
                            int32_t* pred, int32_t* n_tied, int32_t* used_order, int32_t* err, void* stream);
int scn_markov_hash_two_target(int32_t n, const int32_t* prefix_ptr, const int32_t* prefix_nodes, int32_t max_order, int32_t backoff,
                               int32_t min_count, uint64_t seed, const int32_t* target, int32_t n_nodes, int32_t d, const int32_t* nbr,
                               const int32_t* deg, const uint64_t* keys, const int32_t* row_of, int64_t capacity, const int32_t* counts,
                               float* score, int32_t* other, int32_t* used_order, int32_t* err, int32_t* err_target, void* stream);
int scn_markov_hash_probs(int32_t n, const int32_t* prefix_ptr, const int32_t* prefix_nodes, int32_t max_order, int32_t backoff,
                          int32_t min_count, int32_t n_nodes, int32_t d, const int32_t* nbr, const int32_t* deg, const uint64_t* keys,
                          const int32_t* row_of, int64_t capacity, const int32_t* counts, double* probs, int32_t* used_order,
                          int32_t* err, void* stream);
int scn_markov_hash_path_scores(int32_t n_paths, const int32_t* path_ptr, const int32_t* path_nodes, int32_t max_order, int32_t backoff,
                                int32_t min_count, double alpha, int32_t n_nodes, int32_t d, const int32_t* nbr, const int32_t* deg,
                                const uint64_t* keys, const int32_t* row_of, int64_t capacity, const int32_t* counts, double* prob,
                                int32_t* rank, int32_t* total, int32_t* used_order, int32_t* err, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * The harmonic projection baseline (projection_model.py, PM:58-126), everything in fp64.  The pieces of a conjugate-gradient solve of
 * A X = B for k <= SCN_PROJECT_MAX_K columns at once -- X, R, P, AP are [n][k] row-major -- whose step lengths are taken on the device,
 * one per column, from per-workgroup partial sums that every consumer adds up in the same fixed order (no floating-point atomics: the
 * same inputs give the same bits); the Gram product A^T B; and the prediction of a batch in one launch.  A wave covers 64 / k rows of
 * an [n][k] array with one lane per (row, column); k need not be a power of two.  k outside 1 .. SCN_PROJECT_MAX_K is
 * SCN_ERR_UNSUPPORTED before any launch; n == 0 returns SCN_OK without a launch.  Nothing is allocated, nothing synchronises.
 *
 * scn_project_parts (host): the workgroups W <= SCN_PROJECT_MAX_PARTS that scn_csr_apply_f64 and the two updates run for (n, k): their
 *   partial-sum buffers are [W][k].  scn_gram_parts(n): the same for scn_gram_f64, whose buffer is [W][ka * kb].
 * scn_csr_apply_f64: y = A x for the CSR operator (rowptr[n_rows + 1], col -- int32, inside [0, n_rows) -- and val), and
 *   parts[w][c] = the sum over the rows of workgroup w of x[r][c] y[r][c] (in CG: p.Ap).
 * scn_cg_update_xr: alpha[c] = rr[c] / sum_w pap_parts[w][c]; x += alpha p, r -= alpha ap; rr_parts[w][c] = partial sums of r.r.  A
 *   column is frozen (alpha = 0, its x and r keep their bits) once it was found converged or when its denominator is not positive.
 *   first != 0: alpha = 0 for every column (pap_parts, p and ap are not read): the call that takes r0.r0.
 * scn_cg_update_p: rr_new[c] = sum_w rr_parts[w][c]; a column with rr_new <= tol^2 rr0 is frozen from here on (this covers rr0 = 0, so
 *   a column that starts converged never divides 0 by 0); beta[c] = rr_new / rr, 0 when frozen; p = r + beta p.  first != 0: rr0 =
 *   rr_new and p = r.  It leaves rr_new for the next step and two words: flags[2 K + SCN_CG_FLAG_ALL_FROZEN] = 1 when every column is
 *   frozen, and flags[2 K + SCN_CG_FLAG_ITERATIONS], which the caller sets to -1, = the `it` of the call that first found them so
 *   (K = SCN_PROJECT_MAX_K).  state holds SCN_CG_STATE_DOUBLES doubles (rr by parity of it [2][K], rr0 [K]), flags SCN_CG_FLAG_WORDS
 *   int32 (zero at the start but for the -1).  The sequence: xr(it = 0, first), p(it = 0, first), then for it = 1, 2, ...: apply(p ->
 *   ap), xr(it), p(it); the host reads the all-frozen word whenever it likes.
 * scn_gram_f64: out[ka][kb] = a^T b for a [n][ka], b [n][kb] (two launches: partial sums per workgroup, then their sum in order).
 * scn_project_predict: one wave per trajectory i.  c = V^T f over the entries flow_idx / flow_val [flow_ptr[i], flow_ptr[i + 1]) (device
 *   edge ids; any number of entries, none included), V [n_edges][k] in device edge order, k = 0 .. SCN_PROJECT_MAX_K (0: a complex
 *   without holes).  For every edge e at the node last[i] (inc_ptr / inc_edge / inc_sign: the node-major incidence table, inc_sign =
 *   B1[node, e]) with other endpoint j (edge_nodes[n_edges][2]): logits[i][slot(j)] = B1[j, e] (V[e, :] . c), slot(j) the position of j
 *   in nbr[last[i]][0 .. deg); every other slot of the d keeps logit 0 and enters the soft-max (PM:86-96).  probs[i][d] = the soft-max
 *   over all d slots, argmax[i] = its first maximum (PM:108).  err (INT32_MAX at the start) is lowered to a row whose last node or
 *   edge id lies outside the complex or whose tables disagree; such an entry adds nothing.
 * scn_project_two_target: PM:110-126 on probs [n][d]: t = target[i] (a slot), the other slot is o + (o >= t) with o = (u24 *
 *   (n_nbrs[i] - 1)) >> 24 from the uniform of (seed, i, 1, 0); score[i] = 1, 0.5 or 0, other[i] = that slot.  n_nbrs[i] < 2 (PM:119
 *   raises there) or a target outside [0, d) lowers err to i: score 0, other -1.
 * scn_project_path_scores: the teacher-forced score of every node of every path (path_ptr[n_paths + 1] / path_nodes[T], int32) on the
 *   tables of scn_project_predict, one record per node position in arrays parallel to path_nodes: logp, mass (fp64), rank [T] and,
 *   unless NULL, coef [T][k].  Step i of a path goes from a = nodes[ptr + i - 1] to b = nodes[ptr + i] over the edge e_i in a's
 *   incidence row whose other endpoint is b, with the sign B1[b, e_i] = -inc_sign of e_i at a; none found (or an id outside the
 *   complex) lowers err (INT32_MAX at the start) to the flat position of a.  The record at t = path_ptr[p] + q, q >= 1, predicts
 *   nodes[t] from the q nodes before it: c_t = sum_{i=1}^{q-1} sign_i V[e_i, :], every column added in step order starting from +0 (a
 *   repeated edge counts twice, a backtrack cancels; no flow is built), coef[t][:] = c_t; the logits are scn_project_predict's at
 *   last = nodes[t - 1] with c = c_t, the slots without an edge at 0 and inside the soft-max over all d; logp = the logit at the slot
 *   of nodes[t] minus the logsumexp over the d slots; rank = the real neighbours before it by (higher logit, lower slot); mass = log
 *   of the soft-max's sum over the real neighbours.  k = 0 and q = 1 are c = 0: logp = -log d, rank = the slot taken.  The record at
 *   q = 0, and every record from a step on that was not found, is logp 0, rank -1, mass 0, coef 0.  One wave per path, 64 positions
 *   a pass, the running sums carried from pass to pass in the lanes c < k.  The incidence rows and the neighbour table must agree
 *   (scn_project_predict checks that; here d minus the edges at the node is the number of zero slots).  Paths that hold no node at
 *   all (T == 0) are the call with path_nodes, logp, rank and mass all NULL: SCN_OK without a launch, as for n_paths == 0. */
#define SCN_PROJECT_MAX_K 32
#define SCN_PROJECT_MAX_PARTS 1024
#define SCN_CG_STATE_DOUBLES (3 * SCN_PROJECT_MAX_K)
#define SCN_CG_FLAG_WORDS (2 * SCN_PROJECT_MAX_K + 2)
#define SCN_CG_FLAG_ALL_FROZEN 0
#define SCN_CG_FLAG_ITERATIONS 1
int scn_project_parts(int64_t n_rows, int32_t k);
int scn_gram_parts(int64_t n);
int scn_csr_apply_f64(int32_t n_rows, int32_t k, const int32_t* rowptr, const int32_t* col, const double* val, const double* x, double* y,
                      double* parts, void* stream);
int scn_cg_update_xr(int64_t n, int32_t k, int32_t it, int32_t first, const double* pap_parts, const double* p, const double* ap, double* x,
                     double* r, double* state, int32_t* flags, double* rr_parts, void* stream);
int scn_cg_update_p(int64_t n, int32_t k, int32_t it, int32_t first, double tol, const double* rr_parts, const double* r, double* p,
                    double* state, int32_t* flags, void* stream);
int scn_gram_f64(int64_t n, int32_t ka, int32_t kb, const double* a, const double* b, double* parts, double* out, void* stream);
int scn_project_predict(int32_t n, int32_t k, int32_t n_edges, const double* v, const int32_t* flow_ptr, const int32_t* flow_idx,
                        const double* flow_val, const int32_t* last, int32_t n_nodes, const int32_t* inc_ptr, const int32_t* inc_edge,
                        const float* inc_sign, const int32_t* edge_nodes, int32_t d, const int32_t* nbr, const int32_t* deg, double* logits,
                        double* probs, int32_t* argmax, int32_t* err, void* stream);
int scn_project_path_scores(int32_t n_paths, const int32_t* path_ptr, const int32_t* path_nodes, int32_t k, int32_t n_edges,
                            const double* v, int32_t n_nodes, const int32_t* inc_ptr, const int32_t* inc_edge, const float* inc_sign,
                            const int32_t* edge_nodes, int32_t d, const int32_t* nbr, const int32_t* deg, double* logp, int32_t* rank,
                            double* mass, double* coef /* [T][k], may be NULL */, int32_t* err, void* stream);
int scn_project_two_target(int32_t n, int32_t d, uint64_t seed, const double* probs, const int32_t* target, const int32_t* n_nbrs,
                           float* score, int32_t* other, int32_t* err, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Synthetic trajectories (synthetic_data_gen.generate_random_walks, SDG:178-243): batched single-source shortest paths on one sparse
 * graph, and the assembly of a walk from three of them.  Every array is device memory.  The graph is the undirected adjacency as CSR,
 * adj_ptr[n_nodes + 1] / adj with the columns of a row ascending and every edge present in both rows; adj_w (fp64, one weight per
 * entry, the same in both rows, >= 0) or NULL for unit weights (the reference's hop metric).  The library cannot look into device
 * arrays: the caller owns these properties (scone_gcn_amd/synthetic_data_gen.py checks them on the host before the upload); a column
 * outside [0, n_nodes) is skipped, never followed.
 *
 * scn_sssp_paths: job j has source[j] and n_targets (1 .. SCN_SSSP_MAX_TARGETS) targets target[j][t], -1 = no target (an id outside
 *   [0, n_nodes) counts as none; a source outside reaches nothing).  A tentative distance is the bit pattern of an fp64, ordered as an
 *   unsigned 64-bit integer and lowered by a 64-bit atomic minimum; the frontier is relaxed generation by generation (unit weights:
 *   level-synchronous breadth-first search; weights: label-correcting) to THE fixed point dist[v] = min_u fl(dist[u] + w(u, v)).
 *   pred[v] = the smallest-index neighbour u with fl(dist[u] + w(u, v)) == dist[v] exactly, so trees and paths do not depend on the
 *   order of execution.
 *     path [n_jobs][n_targets][path_cap]: the nodes from the source to the target, both included; entries past the length are not written.
 *     path_len [n_jobs][n_targets]: > 0 the length; 0 no target; -1 unreachable; -2 longer than path_cap (nothing is written);
 *       -3 on every target of a job whose frontier was not empty after n_nodes generations (not reachable with weights >= 0).
 *     dist_out [n_jobs][n_targets], optional: the distance of a reached target (path_len > 0 or -2), +inf otherwise.
 *     dist_all, pred_all [n_jobs][n_nodes], optional (64-bit indexing): the whole tree; +inf / -1 where unreachable, pred[source] = -1.
 *       Without them a job ends as soon as its targets are final.
 *     n_gen [n_jobs], optional: generations the job ran.
 *   One 256-thread workgroup owns one job at a time in one of the n_slots slots of the workspace (scn_sssp_slot_bytes(n_nodes) bytes
 *   each, 8-byte aligned); min(n_jobs, n_slots) workgroups run, workgroup g takes the jobs g, g + grid, ...; none waits on another.
 *   SCN_ERR_BAD_ARG for a null array, n_targets or path_cap or n_slots out of range, SCN_ERR_WORKSPACE for fewer than n_slots slots.
 * scn_walk_assemble: attempt a takes job 2 a = (v_1 -> v_begin, v_1 -> v_2) and job 2 a + 1 = (v_2 -> v_end, none) of a
 *   scn_sssp_paths call with n_targets = 2: walk[a] = reverse(path(v_1 -> v_begin))[:-1] + path(v_1 -> v_2)[:-1] + path(v_2 -> v_end)
 *   (SDG:236-238), walk [n][walk_cap], walk_len[a] = its length, or 0 where a segment's path_len is not positive, where the walk is
 *   longer than walk_cap (nothing is written) or where it visits a node twice (SDG:239; an LDS hash set of the walk's ids).
 *   walk_cap <= SCN_WALK_MAX, SCN_ERR_UNSUPPORTED beyond. */
#define SCN_SSSP_MAX_TARGETS 2
#define SCN_WALK_MAX 16384
size_t scn_sssp_slot_bytes(int32_t n_nodes);
int scn_sssp_paths(int32_t n_nodes, const int32_t* adj_ptr, const int32_t* adj, const double* adj_w, int32_t n_jobs, const int32_t* source,
                   const int32_t* target, int32_t n_targets, int32_t path_cap, int32_t* path, int32_t* path_len, double* dist_out,
                   double* dist_all, int32_t* pred_all, int32_t* n_gen, void* workspace, size_t workspace_bytes, int32_t n_slots,
                   void* stream);
int scn_walk_assemble(int32_t n, const int32_t* path, const int32_t* path_len, int32_t path_cap, int32_t* walk, int32_t* walk_len,
                      int32_t walk_cap, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Teacher-forced scoring of node paths (Scone_GCN.path_step_log_probs): the steps around the batched forwards that give the model's
 * log-probability of every node of a path given the nodes before it.  Paths are ragged like the Markov calls: path_ptr[n_paths + 1]
 * and path_nodes[path_ptr[n_paths]], int32, on the device; position t is a flat index into path_nodes.  The step tables are those of
 * the multi-hop calls above ([n_nodes][d]: step_node, step_edge = the DEVICE row, step_sign; deg[n_nodes]); the host builds them by its
 * rule "flow": slots as the readout numbers them, the edge of the sorted pair, +1 where v < u (times the readout's flips).
 * All three calls: every launch on `stream`, nothing allocated, nothing synchronises, no float atomics (the same inputs give the same
 * bytes), n == 0 returns SCN_OK without a launch, SCN_ERR_BAD_SHAPE / SCN_ERR_BAD_ARG for a shape or pointer that cannot be served,
 * before any launch.  Paths may have any length.
 *
 * scn_path_steps: once per call, one wave per path.  A position t whose successor t + 1 lies in the same path is the step
 *   v = nodes[t] -> u = nodes[t + 1]; the outputs are flat arrays parallel to path_nodes:
 *     slot[t]      the first j < deg[v] with step_node[v][j] == u;
 *     row[t]       step_edge[v][slot[t]];
 *     run[t]       the sum of step_sign over the steps t' <= t of the same path with row[t'] == row[t], added in step order: the value
 *                  that edge's flow has after step t (repeated edges accumulate, like path_to_flow's +=, SDG:327-344);
 *     next_same[t] the smallest t' > t of the same path with row[t'] == row[t], else INT32_MAX.
 *   The last position of every path (no step) gets slot = row = -1, run = 0, next_same = INT32_MAX.  An id outside [0, n_nodes), a pair
 *   that is no neighbour or a row outside [0, n_rows) lowers err[0] to t (atomicMin: the caller initialises it to INT32_MAX); nothing is
 *   read through the bad id and the step gets slot = row = -1, run = 0, next_same = INT32_MAX.  A path of length 0 writes nothing.
 * scn_path_slabs: one chunk of items.  Item i < n_items is (item_path[i], item_len[i] = k >= 1): the first k nodes of that path.  x
 *   [n_slabs][n_rows][4][1] (16-byte aligned, n_items <= 4 n_slabs, ns must be 4: SCN_ERR_UNSUPPORTED otherwise): column i = the flow
 *   of that prefix, columns at or past n_items zero.  x is zero except where a step t of the prefix (path_ptr[p] <= t < path_ptr[p] + k
 *   - 1) with row[t] >= 0 is the last one of the prefix on its row -- next_same[t] >= path_ptr[p] + k - 1 -- which SETS
 *   x[i / 4][row[t]][i % 4] = run[t] (an explicit 0 where the steps cancelled).  No two writers touch one word.  Two launches: the
 *   zero fill, then one wave per item.  An item with a path outside [0, n_paths) or k outside [1, length] is a caller's error that
 *   is only guarded against: its column stays zero.  n_items == 0 writes nothing.
 * scn_path_score: the same chunk behind the forward, logp [n_items][d].  With t = path_ptr[p] + k - 1 the position of the prefix's
 *   last node v, j* = slot[t] and lim = deg[v] (clamped to [0, d]):
 *     step_logp[i] = logp[i][j*] (the bits);
 *     step_rank[i] = the number of slots j < lim that come before j* in the order of scn_beam_step / scn_hop_select: a NaN before every
 *                    number, then the higher value, then the lower slot -- 0 exactly when scn_hop_select with limit deg[v] chooses j*;
 *     step_mass[i] = log sum_{j < lim} exp(logp[i][j]), the mass the model leaves on real neighbours (the padded slots keep logit 0
 *                    inside its logsumexp, TE:288), as m + logf(sum_j expf(logp_j - m)) with m the first slot of that order, one fp32
 *                    subtract per slot and an fp32 running sum in slot order; m itself when it is a NaN or +-inf.
 *   An item with j* < 0 (the prefix ends its path, or a bad step), or guarded against as above, gets NaN / -1 / NaN.  One thread per
 *   item.  SCN_ERR_UNSUPPORTED when n_items * d reaches 2^31 - 1.
 * scn_path_stage: one micro-batch of a training step on whole paths (Scone_GCN.path_grad_step): the items of scn_path_slabs staged
 *   into the three tensors a step reads, in buffers the caller keeps from step to step.  The conventions of the three calls above.
 *   x [n_slabs][n_rows][4][1] ends up bitwise what scn_path_slabs leaves for the same items.  n_prev < 0: the buffer holds anything and
 *   gets the dense zero fill first.  n_prev >= 0 (n_prev <= 4 n_slabs): the buffer holds exactly what an earlier call for the n_prev
 *   items prev_item_path / prev_item_len left, zero elsewhere; only the words those items wrote (the same predicate: row[t] >= 0,
 *   next_same[t] >= end) are reset to +0, at the cost of the prefixes' lengths, never of n_slabs * n_rows.  The reset is ordered before
 *   the writes by SEPARATE LAUNCHES on `stream`: the fill or the reset (one wave per previous item), then one wave per column
 *   i < 4 n_slabs.  No two waves of a launch touch one word; no atomics.
 *   last_nodes [4 n_slabs]: path_nodes[path_ptr[p] + k - 1] for a valid item; 0 for padding (i >= n_items) and guarded items.
 *   y [4 n_slabs][d]: every row written whole.  A valid item's row holds item_weight[i] (1 when item_weight is NULL) at slot[t],
 *   t = path_ptr[p] + k - 1, where 0 <= slot[t] < d, and zero elsewhere; rows of padding, of guarded items and of an item whose prefix
 *   ends its path (k == length: slot[t] = -1) are zero.
 *   Before any launch: SCN_ERR_BAD_SHAPE for a negative count, n_rows < 1, d < 1, n_items > 4 n_slabs or n_prev > 4 n_slabs;
 *   SCN_ERR_UNSUPPORTED for ns != 4; SCN_ERR_BAD_ARG for a null or misaligned x and for any other null array the call would read or
 *   write.  n_slabs == 0 launches nothing; n_items == 0 with n_slabs > 0 still resets, and writes zero last nodes and target rows. */
int scn_path_steps(int32_t n_paths, const int32_t* path_ptr, const int32_t* path_nodes, int32_t n_nodes, int32_t d, const int32_t* deg,
                   const int32_t* step_node, const int32_t* step_edge, const float* step_sign, int32_t n_rows, int32_t* slot,
                   int32_t* row, float* run, int32_t* next_same, int32_t* err, void* stream);
int scn_path_slabs(int32_t n_items, int32_t n_slabs, const int32_t* item_path, const int32_t* item_len, int32_t n_paths,
                   const int32_t* path_ptr, const int32_t* row, const float* run, const int32_t* next_same, int32_t n_rows, int32_t ns,
                   float* x, void* stream);
int scn_path_score(int32_t n_items, int32_t d, const int32_t* item_path, const int32_t* item_len, int32_t n_paths,
                   const int32_t* path_ptr, const int32_t* path_nodes, const int32_t* slot, const int32_t* deg, int32_t n_nodes,
                   const float* logp, float* step_logp, int32_t* step_rank, float* step_mass, void* stream);
int scn_path_stage(int32_t n_items, int32_t n_slabs, const int32_t* item_path, const int32_t* item_len, const float* item_weight,
                   int32_t n_prev, const int32_t* prev_item_path, const int32_t* prev_item_len, int32_t n_paths, const int32_t* path_ptr,
                   const int32_t* path_nodes, const int32_t* slot, const int32_t* row, const float* run, const int32_t* next_same,
                   int32_t n_rows, int32_t ns, int32_t d, float* x, int32_t* last_nodes, float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCONE_HIP_H */
