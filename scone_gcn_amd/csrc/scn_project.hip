// The harmonic projection baseline (the reference's projection_model.py, PM:58-126) in fp64: the pieces of a block conjugate-gradient
// solve of L1 X = L1 R for k <= 32 probe columns at once (the operator applied to [n, k] row-major arrays, the two vector updates with
// their step lengths taken on the device from per-workgroup partial sums), the Gram product that orthonormalises what is left of the
// probes, and the prediction of a whole batch in one launch.  Every sum is taken in a fixed order -- per lane over a grid-stride loop,
// per workgroup through LDS, over the workgroups by every consumer in the same order -- and there is no floating-point atomic: the same
// inputs give the same bits, and every workgroup of an update kernel derives the same step length.
#include "scn_internal.h"

namespace {

constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;
constexpr int KMAX = SCN_PROJECT_MAX_K;
constexpr int GRAM_ROWS = 64;       // rows of A and B a workgroup of gram_partial_kernel stages at a time

// A wave covers 64 / k rows, lane l = (row l / k, column l % k) of them: its rows of an [n, k] array are one contiguous read.
struct Lanes {
    int k, rpw, rs, c;      // rows per wave; this lane's row in the wave and column (idle: rs >= rpw)
    int64_t row0, stride;   // first row of this wave and the rows all waves of the grid cover in one pass
    __device__ __forceinline__ Lanes(int k_) : k(k_) {
        const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
        rpw = WAVE / k;
        rs = lane / k;
        c = lane % k;
        row0 = ((int64_t)blockIdx.x * WAVES + wave) * rpw;
        stride = (int64_t)gridDim.x * WAVES * rpw;
    }
    __device__ __forceinline__ bool idle() const { return rs >= rpw; }
};

// The workgroup's sum of one value per lane, by column: the lanes (wave, row) of a column in ascending order.  Written by thread c < k.
__device__ __forceinline__ void block_column_sums(const Lanes& L, double v, double* __restrict__ out) {
    __shared__ double s_lane[THREADS];
    __shared__ double s_wave[WAVES * KMAX];
    s_lane[threadIdx.x] = L.idle() ? 0.0 : v;
    __syncthreads();
    if ((int)threadIdx.x < WAVES * L.k) {
        const int w = threadIdx.x / L.k, c = threadIdx.x % L.k;
        double a = 0.0;
        for (int r = 0; r < L.rpw; ++r) a += s_lane[w * WAVE + r * L.k + c];
        s_wave[w * KMAX + c] = a;
    }
    __syncthreads();
    if ((int)threadIdx.x < L.k) {
        double a = 0.0;
        for (int w = 0; w < WAVES; ++w) a += s_wave[w * KMAX + threadIdx.x];
        out[threadIdx.x] = a;
    }
}

// Column sums of parts[n_parts][k], the same order in every workgroup that calls it: eight strided runs, then the eight in order.
// s_tot[c] holds the sum of column c after the call (c < k).
__device__ __forceinline__ void reduce_parts(const double* __restrict__ parts, int n_parts, int k, double* s_tot) {
    __shared__ double s_run[8 * KMAX];
    const int g = threadIdx.x / KMAX, c = threadIdx.x % KMAX;      // THREADS = 8 * KMAX
    double a = 0.0;
    if (c < k)
        for (int b = g; b < n_parts; b += 8) a += parts[(size_t)b * k + c];
    s_run[g * KMAX + c] = a;
    __syncthreads();
    if ((int)threadIdx.x < k) {
        double t = 0.0;
        for (int q = 0; q < 8; ++q) t += s_run[q * KMAX + threadIdx.x];
        s_tot[threadIdx.x] = t;
    }
    __syncthreads();
}

__global__ __launch_bounds__(THREADS) void csr_apply_kernel(int n_rows, int k, const int32_t* __restrict__ rowptr,
                                                            const int32_t* __restrict__ col, const double* __restrict__ val,
                                                            const double* __restrict__ x, double* __restrict__ y,
                                                            double* __restrict__ parts) {
    const Lanes L(k);
    double dot = 0.0;
    if (!L.idle())
        for (int64_t r = L.row0 + L.rs; r < n_rows; r += L.stride) {
            double a = 0.0;
            for (int j = rowptr[r], j1 = rowptr[r + 1]; j < j1; ++j) a = fma(val[j], x[(size_t)col[j] * k + L.c], a);
            y[(size_t)r * k + L.c] = a;
            dot = fma(x[(size_t)r * k + L.c], a, dot);
        }
    block_column_sums(L, dot, parts + (size_t)blockIdx.x * k);
}

// state: rr[2][KMAX] (r.r before and after the step, by parity), rr0[KMAX]; flags: frozen[KMAX] (read by the x / r update), frozen after
// the step length was taken [KMAX] (read by the p update), then the two words SCN_CG_FLAG_*.
struct CgState {
    double* state;
    int32_t* flags;
    __device__ __forceinline__ double* rr(int parity) const { return state + parity * KMAX; }
    __device__ __forceinline__ double* rr0() const { return state + 2 * KMAX; }
    __device__ __forceinline__ int32_t* frozen_in() const { return flags; }
    __device__ __forceinline__ int32_t* frozen_mid() const { return flags + KMAX; }
};

// x += alpha p, r -= alpha Ap, partial sums of r.r.  alpha[c] = rr[c] / (p.Ap)[c]; 0 for a frozen column and where p.Ap is not
// positive (the column is frozen from here on).  first: alpha = 0 everywhere (the call that only takes r0.r0).
__global__ __launch_bounds__(THREADS) void cg_update_xr_kernel(int64_t n, int k, int it, int first, const double* __restrict__ pap_parts,
                                                              int n_parts, const double* __restrict__ p, const double* __restrict__ ap,
                                                              double* __restrict__ x, double* __restrict__ r, CgState st,
                                                              double* __restrict__ rr_parts) {
    __shared__ double s_tot[KMAX];
    __shared__ double s_alpha[KMAX];
    if (!first) reduce_parts(pap_parts, n_parts, k, s_tot);
    if ((int)threadIdx.x < k) {
        const int c = threadIdx.x;
        double alpha = 0.0;
        int frozen = 0;
        if (!first) {
            const double den = s_tot[c];
            frozen = st.frozen_in()[c] != 0 || !(den > 0.0);
            if (!frozen) alpha = st.rr(it & 1)[c] / den;
        }
        s_alpha[c] = alpha;
        if (blockIdx.x == 0) st.frozen_mid()[c] = frozen;
    }
    __syncthreads();
    const Lanes L(k);
    double dot = 0.0;
    if (!L.idle()) {
        const double alpha = s_alpha[L.c];
        for (int64_t row = L.row0 + L.rs; row < n; row += L.stride) {
            const size_t i = (size_t)row * k + L.c;
            if (alpha != 0.0) {                                  // a frozen column keeps its bits (and never meets an Inf * 0)
                x[i] = fma(alpha, p[i], x[i]);
                r[i] = fma(-alpha, ap[i], r[i]);
            }
            const double ri = r[i];
            dot = fma(ri, ri, dot);
        }
    }
    block_column_sums(L, dot, rr_parts + (size_t)blockIdx.x * k);
}

// p = r + beta p with beta[c] = rr_new[c] / rr[c]; a column whose rr_new <= tol^2 rr0 is frozen (beta = 0) from here on.  first: rr0 =
// rr_new, p = r.  Workgroup 0 leaves rr_new under the other parity, the flags for the next step, and the two words.
__global__ __launch_bounds__(THREADS) void cg_update_p_kernel(int64_t n, int k, int it, int first, double tol2,
                                                             const double* __restrict__ rr_parts, int n_parts,
                                                             const double* __restrict__ r, double* __restrict__ p, CgState st) {
    __shared__ double s_tot[KMAX];
    __shared__ double s_beta[KMAX];
    __shared__ int s_frozen[KMAX];
    reduce_parts(rr_parts, n_parts, k, s_tot);
    if ((int)threadIdx.x < k) {
        const int c = threadIdx.x;
        const double rr_new = s_tot[c];
        const double rr0 = first ? rr_new : st.rr0()[c];
        const int frozen = st.frozen_mid()[c] != 0 || !(rr_new > tol2 * rr0);
        s_beta[c] = (first || frozen) ? 0.0 : rr_new / st.rr(it & 1)[c];
        s_frozen[c] = frozen;
        if (blockIdx.x == 0) {
            st.rr((it + 1) & 1)[c] = rr_new;
            if (first) st.rr0()[c] = rr0;
            st.frozen_in()[c] = frozen;
        }
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int all = 1;
        for (int c = 0; c < k; ++c) all &= s_frozen[c];
        int32_t* words = st.flags + 2 * KMAX;
        words[SCN_CG_FLAG_ALL_FROZEN] = all;
        if (all && words[SCN_CG_FLAG_ITERATIONS] < 0) words[SCN_CG_FLAG_ITERATIONS] = it;
    }
    const Lanes L(k);
    if (!L.idle()) {
        const double beta = s_beta[L.c];
        for (int64_t row = L.row0 + L.rs; row < n; row += L.stride) {
            const size_t i = (size_t)row * k + L.c;
            p[i] = beta != 0.0 ? fma(beta, p[i], r[i]) : r[i];
        }
    }
}

// parts[b][ka][kb] = A^T B over the rows of workgroup b: GRAM_ROWS rows of both staged in LDS, thread t owns the entries t, t + 256, ...
__global__ __launch_bounds__(THREADS) void gram_partial_kernel(int64_t n, int ka, int kb, const double* __restrict__ a,
                                                              const double* __restrict__ b, double* __restrict__ parts) {
    __shared__ double s_a[GRAM_ROWS * KMAX];
    __shared__ double s_b[GRAM_ROWS * KMAX];
    double acc[KMAX * KMAX / THREADS] = {0.0, 0.0, 0.0, 0.0};
    const int n_out = ka * kb;
    for (int64_t r0 = (int64_t)blockIdx.x * GRAM_ROWS; r0 < n; r0 += (int64_t)gridDim.x * GRAM_ROWS) {
        const int rows = (int)(n - r0 < GRAM_ROWS ? n - r0 : GRAM_ROWS);
        for (int i = threadIdx.x; i < rows * ka; i += THREADS) s_a[i] = a[(size_t)r0 * ka + i];
        for (int i = threadIdx.x; i < rows * kb; i += THREADS) s_b[i] = b[(size_t)r0 * kb + i];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < KMAX * KMAX / THREADS; ++q) {
            const int e = threadIdx.x + q * THREADS;
            if (e < n_out) {
                const int i = e / kb, j = e % kb;
                double s = acc[q];
                for (int r = 0; r < rows; ++r) s = fma(s_a[r * ka + i], s_b[r * kb + j], s);
                acc[q] = s;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < KMAX * KMAX / THREADS; ++q) {
        const int e = threadIdx.x + q * THREADS;
        if (e < n_out) parts[(size_t)blockIdx.x * n_out + e] = acc[q];
    }
}

__global__ __launch_bounds__(THREADS) void gram_sum_kernel(int n_parts, int n_out, const double* __restrict__ parts,
                                                          double* __restrict__ out) {
    const int e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= n_out) return;
    double s = 0.0;
    for (int b = 0; b < n_parts; ++b) s += parts[(size_t)b * n_out + e];
    out[e] = s;
}

struct Readout {
    const int32_t* inc_ptr;     // [n_nodes + 1]
    const int32_t* inc_edge;    // device edge ids of a node's incident edges
    const float* inc_sign;      // B1[node, edge]
    const int32_t* edge_nodes;  // [n_edges][2]
    const int32_t* nbr;         // [n_nodes][d], ascending, -1 behind
    const int32_t* deg;         // [n_nodes]
    int n_nodes, n_edges, d;
};

// One wave per trajectory (PM:80-96, 108).  err is lowered to the row whose last node or edge id lies outside the complex, or whose
// incident edge leads to no slot of the neighbour table; such an entry adds nothing.
__global__ __launch_bounds__(WAVE) void project_predict_kernel(int k, const double* __restrict__ v, const int32_t* __restrict__ ptr,
                                                              const int32_t* __restrict__ idx, const double* __restrict__ val,
                                                              const int32_t* __restrict__ last, Readout g, double* __restrict__ logits,
                                                              double* __restrict__ probs, int32_t* __restrict__ argmax, int32_t* err) {
    __shared__ double s_part[WAVE];
    __shared__ double s_c[KMAX];
    const int i = blockIdx.x, lane = threadIdx.x;
    // c = V^T f over the flow's entries: lane = (entry lane / k of a pass, column lane % k), the passes and then the lanes in order
    // (k = 0, a complex without holes: no pass, every logit stays 0)
    const int per = k > 0 ? WAVE / k : 0, slot_e = k > 0 ? lane / k : 0, q = k > 0 ? lane % k : 0;
    double a = 0.0;
    if (slot_e < per)
        for (int j = ptr[i] + slot_e, j1 = ptr[i + 1]; j < j1; j += per) {
            const int e = idx[j];
            if (e < 0 || e >= g.n_edges) {
                atomicMin(err, i);
                continue;
            }
            a = fma(val[j], v[(size_t)e * k + q], a);
        }
    s_part[lane] = slot_e < per ? a : 0.0;
    __syncthreads();
    if (lane < k) {
        double c = 0.0;
        for (int s = 0; s < per; ++s) c += s_part[s * k + lane];
        s_c[lane] = c;
    }
    double* lg = logits + (size_t)i * g.d;
    for (int j = lane; j < g.d; j += WAVE) lg[j] = 0.0;          // the padding keeps logit 0 (PM:86)
    __syncthreads();
    const int node = last[i];
    if (node < 0 || node >= g.n_nodes) {
        if (lane == 0) atomicMin(err, i);
    } else {
        const int dv = min(max(g.deg[node], 0), g.d);
        const int32_t* row = g.nbr + (size_t)node * g.d;
        for (int t = g.inc_ptr[node] + lane, t1 = g.inc_ptr[node + 1]; t < t1; t += WAVE) {
            const int e = g.inc_edge[t];
            int s = -1;
            if (e >= 0 && e < g.n_edges) {
                const int a0 = g.edge_nodes[2 * (size_t)e], a1 = g.edge_nodes[2 * (size_t)e + 1];
                const int other = a0 == node ? a1 : a0;
                for (int j = 0; j < dv; ++j)
                    if (row[j] == other) {
                        s = j;
                        break;
                    }
            }
            if (s < 0) {
                atomicMin(err, i);
                continue;
            }
            double h = 0.0;                                      // (V c)[e]
            for (int m = 0; m < k; ++m) h = fma(v[(size_t)e * k + m], s_c[m], h);
            lg[s] = -(double)g.inc_sign[t] * h;                  // B1[other, e] = -B1[node, e]
        }
    }
    __syncthreads();
    // soft-max over all d slots (PM:96), then the first maximum of the probabilities (PM:108)
    double mx = -INFINITY;
    for (int j = lane; j < g.d; j += WAVE) mx = fmax(mx, lg[j]);
    for (int o = WAVE / 2; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, WAVE));
    double sum = 0.0;
    for (int j = lane; j < g.d; j += WAVE) sum += exp(lg[j] - mx);
    for (int o = WAVE / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o, WAVE);
    double best = -1.0;
    int at = INT32_MAX;
    for (int j = lane; j < g.d; j += WAVE) {
        const double pj = exp(lg[j] - mx) / sum;
        probs[(size_t)i * g.d + j] = pj;
        if (pj > best) {
            best = pj;
            at = j;
        }
    }
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, WAVE);
        const int oa = __shfl_xor(at, o, WAVE);
        if (ob > best || (ob == best && oa < at)) {
            best = ob;
            at = oa;
        }
    }
    if (lane == 0) argmax[i] = at;
}

// PM:110-126 with the draw keyed by (seed, row): the other slot among the deg - 1 that are not the target's
__global__ __launch_bounds__(THREADS) void project_two_target_kernel(int n, int d, uint64_t seed, const double* __restrict__ probs,
                                                                    const int32_t* __restrict__ target, const int32_t* __restrict__ n_nbrs,
                                                                    float* __restrict__ score, int32_t* __restrict__ other, int32_t* err) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int t = target[i], dv = n_nbrs[i];
    float sc = 0.f;
    int ot = -1;
    if (t < 0 || t >= d || dv < 2 || dv > d) {
        atomicMin(err, i);
    } else {
        const uint32_t u24 = (uint32_t)(scn::sample_uniform(seed, i, 1, 0) * 16777216.f);   // exact: the 24 bits behind the uniform
        const int o = (int)(((uint64_t)u24 * (uint64_t)(dv - (t < dv ? 1 : 0))) >> 24);
        ot = o + ((t < dv && o >= t) ? 1 : 0);
        const double pt = probs[(size_t)i * d + t], po = probs[(size_t)i * d + ot];
        sc = pt == po ? 0.5f : (pt > po ? 1.f : 0.f);
    }
    score[i] = sc;
    other[i] = ot;
}

// (V[e, :] . c) of one record: the columns in order, one fma each
__device__ __forceinline__ double row_dot(const double* __restrict__ v, int k, int e, const double* c) {
    double h = 0.0;
    for (int m = 0; m < k; ++m) h = fma(v[(size_t)e * k + m], c[m], h);
    return h;
}

// One wave per path.  A pass takes the 64 node positions q0 .. q0 + 63: lane l looks up the step into its position (edge and sign),
// the steps' rows sign * V[e, :] go to LDS, lanes c < k turn column c into its running sum in step order -- s_c[l][:] becomes the
// coefficients of the prefix BEFORE the step of position q0 + l, the carry stays in the lane for the next pass -- and lane l finishes
// the record of its position from s_c[l][:]: two passes over the edges at the prefix's last node, the maximum first, then the sums
// and the rank (a lower slot is a lower node id: the neighbour rows ascend).  Nothing of the size of a flow is built.
__global__ __launch_bounds__(WAVE) void project_path_scores_kernel(int k, const double* __restrict__ v, const int32_t* __restrict__ ptr,
                                                                  const int32_t* __restrict__ nodes, Readout g, double* __restrict__ logp,
                                                                  int32_t* __restrict__ rank, double* __restrict__ mass,
                                                                  double* __restrict__ coef, int32_t* err) {
    __shared__ double s_c[WAVE * (KMAX + 1)];
    __shared__ int s_edge[WAVE];
    __shared__ double s_sign[WAVE];
    __shared__ int s_blank[WAVE];
    const int p = blockIdx.x, lane = threadIdx.x;
    const int t0 = ptr[p], len = ptr[p + 1] - t0;
    const int ks = k | 1;                                            // odd row stride: the lanes' rows start on different banks
    double carry = 0.0;                                              // lane c < k: column c of the steps before this pass, from +0
    bool bad_before = false;                                         // an earlier pass met a step that is no edge
    for (int q0 = 0; q0 < len; q0 += WAVE) {
        const int q = q0 + lane, t = t0 + q;
        const bool is_step = q >= 1 && q < len;
        int e = -1, a = -1, b = -1;
        double sign = 0.0;
        if (is_step) {
            a = nodes[t - 1];
            b = nodes[t];
            if (a >= 0 && a < g.n_nodes && b >= 0 && b < g.n_nodes)
                for (int x = g.inc_ptr[a], x1 = g.inc_ptr[a + 1]; x < x1; ++x) {
                    const int ex = g.inc_edge[x];
                    if (ex < 0 || ex >= g.n_edges) continue;
                    const int a0 = g.edge_nodes[2 * (size_t)ex], a1 = g.edge_nodes[2 * (size_t)ex + 1];
                    if ((a0 == a ? a1 : a0) == b) {
                        e = ex;
                        sign = -(double)g.inc_sign[x];               // B1[b, e] = -B1[a, e]
                        break;
                    }
                }
            if (e < 0) atomicMin(err, t - 1);
        }
        const unsigned long long bad = __ballot(is_step && e < 0);
        const bool blank = !is_step || bad_before || (bad & ((2ull << lane) - 1ull)) != 0;   // a bad step at or before this one
        s_edge[lane] = e;
        s_sign[lane] = sign;
        s_blank[lane] = blank ? 1 : 0;
        __syncthreads();
        for (int i = lane; i < WAVE * k; i += WAVE) {
            const int l = i / k, el = s_edge[l];
            s_c[l * ks + i % k] = el >= 0 ? s_sign[l] * v[(size_t)el * k + i % k] : 0.0;
        }
        __syncthreads();
        if (lane < k)
            for (int l = 0; l < WAVE; ++l) {
                const double step = s_c[l * ks + lane];
                s_c[l * ks + lane] = carry;
                carry += step;
            }
        __syncthreads();
        if (coef) {
            const int n_here = min(WAVE, len - q0);
            for (int i = lane; i < n_here * k; i += WAVE)
                coef[(size_t)(t0 + q0) * k + i] = s_blank[i / k] ? 0.0 : s_c[i / k * ks + i % k];
        }
        if (q < len) {
            double lp = 0.0, ms = 0.0;
            int rk = -1;
            if (!blank) {
                const double* c = s_c + lane * ks;
                const double taken = sign * row_dot(v, k, e, c);
                const int x0 = g.inc_ptr[a], x1 = g.inc_ptr[a + 1];
                int n_real = 0;
                double mx = -INFINITY;
                for (int x = x0; x < x1; ++x) {
                    const int ex = g.inc_edge[x];
                    if (ex < 0 || ex >= g.n_edges) continue;
                    mx = fmax(mx, -(double)g.inc_sign[x] * row_dot(v, k, ex, c));
                    ++n_real;
                }
                const int n_pad = g.d - n_real;                      // the padding's logits are 0 and enter the soft-max (PM:86)
                if (n_pad > 0) mx = fmax(mx, 0.0);
                double sum = 0.0;
                int before = 0;
                for (int x = x0; x < x1; ++x) {
                    const int ex = g.inc_edge[x];
                    if (ex < 0 || ex >= g.n_edges) continue;
                    const double lg = -(double)g.inc_sign[x] * row_dot(v, k, ex, c);
                    sum += exp(lg - mx);
                    const int a0 = g.edge_nodes[2 * (size_t)ex], a1 = g.edge_nodes[2 * (size_t)ex + 1];
                    const int other = a0 == a ? a1 : a0;
                    before += (lg > taken || (lg == taken && other < b)) ? 1 : 0;
                }
                double all = sum;
                if (n_pad > 0) all += (double)n_pad * exp(0.0 - mx);
                lp = taken - (mx + log(all));
                ms = log(sum / all);
                rk = before;
            }
            logp[t] = lp;
            rank[t] = rk;
            mass[t] = ms;
        }
        bad_before = bad_before || bad != 0;
        __syncthreads();
    }
}

int grid_for(int64_t n_rows, int k) {
    const int64_t per_block = (int64_t)WAVES * (WAVE / k);
    const int64_t blocks = (n_rows + per_block - 1) / per_block;
    return (int)(blocks < 1 ? 1 : (blocks > SCN_PROJECT_MAX_PARTS ? SCN_PROJECT_MAX_PARTS : blocks));
}

}  // namespace

extern "C" {

int scn_project_parts(int64_t n_rows, int32_t k) {
    if (n_rows < 0) return SCN_ERR_BAD_SHAPE;
    if (k < 1 || k > KMAX) return SCN_ERR_UNSUPPORTED;
    return grid_for(n_rows, k);
}

int scn_csr_apply_f64(int32_t n_rows, int32_t k, const int32_t* rowptr, const int32_t* col, const double* val, const double* x, double* y,
                      double* parts, void* stream) {
    if (n_rows < 0) return SCN_ERR_BAD_SHAPE;
    if (k < 1 || k > KMAX) return SCN_ERR_UNSUPPORTED;
    if (n_rows == 0) return SCN_OK;
    if (!rowptr || !col || !val || !x || !y || !parts) return SCN_ERR_BAD_ARG;
    return scn::launch_checked(csr_apply_kernel, dim3((unsigned)grid_for(n_rows, k)), dim3(THREADS), 0, (hipStream_t)stream, n_rows, k,
                               rowptr, col, val, x, y, parts);
}

int scn_cg_update_xr(int64_t n, int32_t k, int32_t it, int32_t first, const double* pap_parts, const double* p, const double* ap, double* x,
                     double* r, double* state, int32_t* flags, double* rr_parts, void* stream) {
    if (n < 0 || it < 0) return SCN_ERR_BAD_SHAPE;
    if (k < 1 || k > KMAX) return SCN_ERR_UNSUPPORTED;
    if (n == 0) return SCN_OK;
    if ((!first && (!pap_parts || !p || !ap)) || !x || !r || !state || !flags || !rr_parts) return SCN_ERR_BAD_ARG;
    const int grid = grid_for(n, k);
    return scn::launch_checked(cg_update_xr_kernel, dim3((unsigned)grid), dim3(THREADS), 0, (hipStream_t)stream, n, k, it, first, pap_parts,
                               grid, p, ap, x, r, CgState{state, flags}, rr_parts);
}

int scn_cg_update_p(int64_t n, int32_t k, int32_t it, int32_t first, double tol, const double* rr_parts, const double* r, double* p,
                    double* state, int32_t* flags, void* stream) {
    if (n < 0 || it < 0 || !(tol >= 0.0)) return SCN_ERR_BAD_SHAPE;
    if (k < 1 || k > KMAX) return SCN_ERR_UNSUPPORTED;
    if (n == 0) return SCN_OK;
    if (!rr_parts || !r || !p || !state || !flags) return SCN_ERR_BAD_ARG;
    return scn::launch_checked(cg_update_p_kernel, dim3((unsigned)grid_for(n, k)), dim3(THREADS), 0, (hipStream_t)stream, n, k, it, first,
                               tol * tol, rr_parts, grid_for(n, k), r, p, CgState{state, flags});
}

int scn_gram_parts(int64_t n) {
    if (n < 0) return SCN_ERR_BAD_SHAPE;
    const int64_t blocks = (n + GRAM_ROWS - 1) / GRAM_ROWS;
    return (int)(blocks < 1 ? 1 : (blocks > SCN_PROJECT_MAX_PARTS ? SCN_PROJECT_MAX_PARTS : blocks));
}

int scn_gram_f64(int64_t n, int32_t ka, int32_t kb, const double* a, const double* b, double* parts, double* out, void* stream) {
    if (n < 0) return SCN_ERR_BAD_SHAPE;
    if (ka < 1 || ka > KMAX || kb < 1 || kb > KMAX) return SCN_ERR_UNSUPPORTED;
    if (n == 0) return SCN_OK;
    if (!a || !b || !parts || !out) return SCN_ERR_BAD_ARG;
    const int n_parts = scn_gram_parts(n), n_out = ka * kb;
    const int st = scn::launch_checked(gram_partial_kernel, dim3((unsigned)n_parts), dim3(THREADS), 0, (hipStream_t)stream, n, ka, kb, a, b,
                                       parts);
    if (st != SCN_OK) return st;
    return scn::launch_checked(gram_sum_kernel, dim3((unsigned)((n_out + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream,
                               n_parts, n_out, parts, out);
}

int scn_project_predict(int32_t n, int32_t k, int32_t n_edges, const double* v, const int32_t* flow_ptr, const int32_t* flow_idx,
                        const double* flow_val, const int32_t* last, int32_t n_nodes, const int32_t* inc_ptr, const int32_t* inc_edge,
                        const float* inc_sign, const int32_t* edge_nodes, int32_t d, const int32_t* nbr, const int32_t* deg, double* logits,
                        double* probs, int32_t* argmax, int32_t* err, void* stream) {
    if (n < 0 || n_edges <= 0 || n_nodes <= 0 || d <= 0) return SCN_ERR_BAD_SHAPE;
    if (k < 0 || k > KMAX) return SCN_ERR_UNSUPPORTED;
    if (n == 0) return SCN_OK;
    if ((k > 0 && !v) || !flow_ptr || !last || !inc_ptr || !inc_edge || !inc_sign || !edge_nodes || !nbr || !deg || !logits || !probs ||
        !argmax || !err)
        return SCN_ERR_BAD_ARG;
    return scn::launch_checked(project_predict_kernel, dim3((unsigned)n), dim3(WAVE), 0, (hipStream_t)stream, k, v, flow_ptr, flow_idx,
                               flow_val, last, Readout{inc_ptr, inc_edge, inc_sign, edge_nodes, nbr, deg, n_nodes, n_edges, d}, logits,
                               probs, argmax, err);
}

int scn_project_path_scores(int32_t n_paths, const int32_t* path_ptr, const int32_t* path_nodes, int32_t k, int32_t n_edges,
                            const double* v, int32_t n_nodes, const int32_t* inc_ptr, const int32_t* inc_edge, const float* inc_sign,
                            const int32_t* edge_nodes, int32_t d, const int32_t* nbr, const int32_t* deg, double* logp, int32_t* rank,
                            double* mass, double* coef, int32_t* err, void* stream) {
    if (n_paths < 0 || n_edges <= 0 || n_nodes <= 0 || d <= 0) return SCN_ERR_BAD_SHAPE;
    if (k < 0 || k > KMAX) return SCN_ERR_UNSUPPORTED;
    if (n_paths == 0) return SCN_OK;
    if ((k > 0 && !v) || !path_ptr || !inc_ptr || !inc_edge || !inc_sign || !edge_nodes || !nbr || !deg || !err) return SCN_ERR_BAD_ARG;
    if (!path_nodes && !logp && !rank && !mass) return SCN_OK;       // paths without a node: T == 0, nothing to write
    if (!path_nodes || !logp || !rank || !mass) return SCN_ERR_BAD_ARG;
    return scn::launch_checked(project_path_scores_kernel, dim3((unsigned)n_paths), dim3(WAVE), 0, (hipStream_t)stream, k, v, path_ptr,
                               path_nodes, Readout{inc_ptr, inc_edge, inc_sign, edge_nodes, nbr, deg, n_nodes, n_edges, d}, logp, rank,
                               mass, coef, err);
}

int scn_project_two_target(int32_t n, int32_t d, uint64_t seed, const double* probs, const int32_t* target, const int32_t* n_nbrs,
                           float* score, int32_t* other, int32_t* err, void* stream) {
    if (n < 0 || d <= 0) return SCN_ERR_BAD_SHAPE;
    if (n == 0) return SCN_OK;
    if (!probs || !target || !n_nbrs || !score || !other || !err) return SCN_ERR_BAD_ARG;
    return scn::launch_checked(project_two_target_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0,
                               (hipStream_t)stream, n, d, seed, probs, target, n_nbrs, score, other, err);
}

}  // extern "C"
