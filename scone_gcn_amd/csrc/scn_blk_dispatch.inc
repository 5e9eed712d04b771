// host dispatch of the blocked kernels -- part of scn_blocked.hip (one translation unit; included inside namespace scn)
// ------------------------------------------------------------------------------------------------
// host dispatch
// ------------------------------------------------------------------------------------------------
static bool scone_shape(const scn_conv_s* c) {
    return c->plan.built && c->n_groups == 1 && c->g[0].identity == 1 && c->g[0].n_vals == 2;
}

// persistent grid: workgroups per CU by LDS footprint, blocks strided XCD-contiguously; small operators split slabs
// Cost-balanced STATIC assignment of blocks to workgroups for a launch with gx workgroups per slab range: workgroup j of XCD
// x visits positions b0 + j, b0 + j + stride, ... of its XCD's range (block_range); within every round of `stride` positions
// the most expensive blocks go to the workgroups that have the least so far.  Blocks of a round still run at the same time
// (halo rows stay shared in L2) and the assignment is fixed, so the weight gradient stays bitwise reproducible; the busiest
// workgroup had 2.3 % (forward) / 3.4 % (backward) more than the mean with the plain stride.
static const int32_t* balanced_assignment(const scn_conv_s* c, int gx) {   // tables are built with the plan, for every grid launch_grid can pick
#ifdef SCN_AB_NO_BALANCE                                                        // diagnostic builds (tools/ab_build.sh): plain strided assignment
    return nullptr;
#endif
    auto it = c->plan.assign_by_grid.find(gx);
    return it != c->plan.assign_by_grid.end() ? it->second : nullptr;
}

static int build_assignment(scn_conv_s* c, int gx) {
    BlockPlan& B = c->plan;
    const int nb = B.dev.n_blocks, stride = gx / 8;
    if (stride <= 0 || nb <= gx || (int)B.h_cost.size() != nb || B.assign_by_grid.count(gx)) return SCN_OK;
    std::vector<int32_t> assign(nb);
    std::vector<double> load(stride);
    std::vector<int> wg(stride), blk(stride);
    for (int x = 0; x < 8; ++x) {
        const int b0 = (int)((int64_t)nb * x / 8), last = (int)((int64_t)nb * (x + 1) / 8);
        std::fill(load.begin(), load.end(), 0.0);
        for (int r = b0; r < last; r += stride) {
            const int cnt = std::min(stride, last - r);
            for (int i = 0; i < cnt; ++i) { wg[i] = i; blk[i] = r + i; }
            std::stable_sort(wg.begin(), wg.begin() + cnt, [&](int a, int b) { return load[a] < load[b]; });
            std::stable_sort(blk.begin(), blk.begin() + cnt, [&](int a, int b) { return B.h_cost[a] > B.h_cost[b]; });
            for (int i = 0; i < cnt; ++i) {
                assign[r + wg[i]] = blk[i];
                load[wg[i]] += B.h_cost[blk[i]];
            }
        }
    }
    const int32_t* dev = nullptr;
    const int st = upload(c, assign, &dev);
    if (st == SCN_OK) B.assign_by_grid[gx] = dev;
    return st;
}

int build_assignments(scn_conv_s* c) {                      // every grid.x launch_grid can produce for this plan
    const int nb = c->plan.dev.n_blocks;
    for (int cap : {256, 512, 768})
        for (int gy = 1; gy <= 32; gy *= 2) {
            const int gx = std::max(8, std::min(cap / gy, ((nb + 7) / 8) * 8) / 8 * 8);
            const int st = build_assignment(c, gx);
            if (st != SCN_OK) return st;
        }
    return SCN_OK;
}

static dim3 launch_grid(const scn_conv_s* c, int n_slabs, size_t lds, int max_per_cu = 2) {
    const int nb = c->plan.dev.n_blocks;
    const int per_cu = (max_per_cu >= 3 && lds <= 160 * 1024 / max_per_cu) ? max_per_cu : (lds <= 80 * 1024 ? 2 : 1);
    const int cap = 256 * per_cu;
    // gx workgroups stride over the blocks (a multiple of 8: one share per XCD), gy split the slabs.  Pick the split whose
    // busiest workgroup has the least (blocks x slabs) to do: at |E| = 50k (830 blocks) 256 x 1 leaves a 4-vs-3 block tail,
    // 64 x 4 is even; at |E| = 1M the answer stays 256 x 1.
    const int nb_xcd = (nb + 7) / 8;
    long best = -1;
    int bx = 8, by = 1;
    for (int gy = 1; gy <= 32 && gy <= std::max(1, n_slabs); gy *= 2) {
        int gx = std::max(8, std::min(cap / gy, ((nb + 7) / 8) * 8) / 8 * 8);
        // a block visit costs its slabs plus about half a slab of prologue (ELL tile, DMA offsets)
        const long work = (long)((nb_xcd + gx / 8 - 1) / (gx / 8)) * (2 * ((n_slabs + gy - 1) / gy) + 1);
        const long cost = work * 64 + gy;                                                    // ties: fewer slab splits
        if (best < 0 || cost < best) { best = cost; bx = gx; by = gy; }
    }
    return dim3(bx, by);
}

constexpr FirstW NO_FIRSTW{{nullptr, nullptr, nullptr}};
constexpr KeepMask NO_KEEP{nullptr, 0};
constexpr UnitList NO_UNITS{nullptr, nullptr};

// The masked 32-channel forms and gather3_c1_keep_kernel are launched with WSCAN_LDS_BYTES more dynamic LDS than the forms without a
// mask, for the table of their window scan (scn_window_scan.inc); the grid is still picked from the plain form's footprint.
static_assert(W16_EXTRA_BYTES + W16_FIRSTW_BYTES + WSCAN_LDS_BYTES <= 160 * 1024 - (2 * BK_SRC * 512 + BK_ELL_CAP * 10 + BK_SRC * 4 + BK_R + 16) &&
              B32_EXTRA_BYTES + WSCAN_LDS_BYTES <= 160 * 1024 - (2 * BK_SRC * 512 + BK_ELL_CAP * 10 + BK_SRC * 4 + BK_R + 16),
              "the scan's table fits behind the kernels' own LDS");
// The VISIT backwards take VISIT_ROWS_BYTES more behind the table (the unit pipeline's second source-row buffer, scn_blk_bwd.inc).
// and WSCAN_HDR_BYTES behind that (the record table of their scans, scn_window_scan.inc): 163 216 of the CU's 163 840 bytes.
// Their `flags` argument carries the process-wide switches g_visit_prefetch (scn_conv_visit_prefetch) and g_visit_records
// (scn_conv_visit_records; it acts where the pipeline is on).
constexpr size_t VISIT_LDS_BYTES = WSCAN_LDS_BYTES + VISIT_ROWS_BYTES + WSCAN_HDR_BYTES;
static_assert(B32_EXTRA_BYTES + VISIT_LDS_BYTES <= 160 * 1024 - (2 * BK_SRC * 512 + BK_ELL_CAP * 10 + BK_SRC * 4 + BK_R + 16),
              "the scan's table, the second source-row buffer and the record table fit behind the backward's own LDS");
static int g_visit_prefetch = 1, g_visit_records = 1;
static int visit_flags() { return (g_visit_prefetch ? VISIT_FLAG_PREFETCH : 0) | (g_visit_records ? VISIT_FLAG_RECORDS : 0); }

// The keep mask of a launch (scn_conv_forward_keep / _from_y_keep; the source mask of scn_conv_backward_dzmask has its geometry and
// its window limit): words per block from the slab count.  A workgroup holds the bits
// of its slab range in one 64-bit window (keep_window): false where the grid hands one more than that.
static bool keep_fits(unsigned gy, int n_slabs) { return (n_slabs + (int)gy - 1) / (int)gy <= KEEP_WINDOW; }
static KeepMask keep_mask_of(const uint32_t* keep, int n_slabs) { return KeepMask{keep, (n_slabs + 31) / 32}; }
// The unit list of a forward-side masked launch (WindowWalk's list mode): served where the grid has ONE slab range of at most
// KEEP_WINDOW slabs, so that an entry's word lies inside every workgroup's window; any other launch walks its static units, with the
// same results.
static UnitList unit_list_of(const uint32_t* units, const uint32_t* count, dim3 grid, int n_slabs) {
    return units && count && grid.y == 1 && n_slabs <= KEEP_WINDOW ? UnitList{units, count} : NO_UNITS;
}

// What a launch of a blocked kernel starts from: the plan's device view with the block assignment of the chosen grid, the grid
// (a work list carries its own slab lists: no slab split then), the operator's shape.
struct BlockedLaunch {
    PlanDev P;
    dim3 grid;
    int nr, nc;
    int n_wg() const { return (int)(grid.x * grid.y); }
};
static BlockedLaunch blocked_launch(const scn_conv_s* c, int n_slabs, size_t lds, const WorkList& wl = NO_LIST, int max_per_cu = 2) {
    BlockedLaunch L{c->plan.dev, launch_grid(c, n_slabs, lds, max_per_cu), c->n_rows, c->g[0].n_cols};
    L.P.assign = balanced_assignment(c, L.grid.x);
    if (wl.block) L.grid.y = 1;
    return L;
}

// dW[k][ca][c] += the workgroups' partial sums [n_wg][c_aux][3 * cd] of a backward launch (fixed order)
static int reduce_dw(const float* partial, int n_wg, int c_aux, int cd, float* const* dW, hipStream_t st) {
    return launch_checked(blocked_dw_reduce, dim3((c_aux * 3 * cd + 63) / 64), dim3(1024), 0, st, partial, n_wg, c_aux, cd, dW[0], dW[1],
                          dW[2]);
}

bool blocked_forward_supported(const scn_conv_s* c, int ns, const int32_t* c_in, int c_out) {
    if (!scone_shape(c) || ns != BK_NS) return false;
    const int ci = c_in[0];
    return (ci == 32 && c_out == 32) || (ci == 16 && c_out == 16) || (ci == 1 && (c_out == 16 || c_out == 32));
}

int blocked_forward(scn_conv_s* c, const FwdLaunch& a) {
    const int n_slabs = a.n_slabs, ci = a.c_in;
    const float* const* W = a.W;
    const WorkList& wl = a.wl;
    hipStream_t st = a.st;
    if (a.partial && ci != 32) return SCN_ERR_UNSUPPORTED;
    if (a.keep && (a.partial || wl.block || !a.out || (ci != 32 && ci != 16))) return SCN_ERR_UNSUPPORTED;   // (the first layer is never the last)
    if (!a.out) {                                                         // first layer, shifted input only (scn_conv_forward_first with out = NULL)
        if (ci != 1 || !a.y_out || wl.block) return SCN_ERR_UNSUPPORTED;
        const size_t lds = smem_bytes(16);
        return launch_checked(gather3_c1_kernel, launch_grid(c, n_slabs, lds), dim3(BK_THREADS), lds, st, c->plan.dev, a.src, a.y_out,
                              c->n_rows, c->g[0].n_cols, n_slabs);
    }
    if (ci == 32) {                                                       // 16 waves, f16 hi + lo split
        const size_t lds = smem_bytes_c32(W16_EXTRA_BYTES);
        const BlockedLaunch L = blocked_launch(c, n_slabs, lds, wl);
        if (a.keep && !keep_fits(L.grid.y, n_slabs)) return SCN_ERR_UNSUPPORTED;
        return with_act(a.act, [&](auto A) -> int {
            constexpr int ACT = decltype(A)::value;
            if (a.keep)
                return launch_checked(fwd_c32_plain_keep<ACT>, L.grid, dim3(W16_THREADS), lds + WSCAN_LDS_BYTES, st, L.P, a.src, nullptr, W[0], W[1], W[2],
                                      a.out, L.nr, L.nc, n_slabs, wl, NO_FIRSTW, keep_mask_of(a.keep, n_slabs),
                                      unit_list_of(a.units, a.unit_count, L.grid, n_slabs));
            return launch_checked(a.partial ? fwd_c32_accum<ACT> : fwd_c32_plain<ACT>, L.grid, dim3(W16_THREADS), lds, st, L.P, a.src,
                                  a.partial, W[0], W[1], W[2], a.out, L.nr, L.nc, n_slabs, wl, NO_FIRSTW, NO_KEEP, NO_UNITS);
        });
    }
    if (ci == 16) {                                                       // 16 waves, f16 hi + lo split, two slabs per visit
        const size_t lds = smem_bytes_c32(16 + 64);
        const BlockedLaunch L = blocked_launch(c, n_slabs, lds, wl);
        if (a.keep && !keep_fits(L.grid.y, n_slabs)) return SCN_ERR_UNSUPPORTED;
        return with_act(a.act, [&](auto A) -> int {
            constexpr int ACT = decltype(A)::value;
            return launch_checked(a.keep ? fwd_c16_plain_keep<ACT> : fwd_c16_plain<ACT>, L.grid, dim3(W16_THREADS), lds, st, L.P, a.src, nullptr,
                                  W[0], W[1], W[2], a.out, L.nr, L.nc, n_slabs, wl, a.keep ? keep_mask_of(a.keep, n_slabs) : NO_KEEP);
        });
    }
    const size_t lds = smem_bytes(16, 2 * BK_R * BK_NS * 12);
    // 8-wave workgroups at 64 VGPRs and 23 KB of LDS: three per CU (4.45 -> 3.9 ms; four: 4.8)
    const BlockedLaunch L = blocked_launch(c, n_slabs, lds, wl, 3);
    return launch_checked(a.c_out == 32 ? fwd_c1_kernel<32> : fwd_c1_kernel<16>, L.grid, dim3(BK_THREADS), lds, st, L.P, a.src, W[0], W[1],
                          W[2], a.out, a.y_out, L.nr, L.nc, n_slabs, a.act, wl);
}

// The y-only launch of the first layer (blocked_forward with out = nullptr) on the items of a keep mask: gather3_c1_keep_kernel on
// the plain launch's grid.  Of the record: n_slabs, src, y_out, keep, units / unit_count, st.
int blocked_shifted_input_keep(scn_conv_s* c, const FwdLaunch& a) {
    const size_t lds = smem_bytes(16);
    const dim3 grid = launch_grid(c, a.n_slabs, lds);
    if (!keep_fits(grid.y, a.n_slabs)) return SCN_ERR_UNSUPPORTED;
    return launch_checked(gather3_c1_keep_kernel, grid, dim3(BK_THREADS), lds + WSCAN_LDS_BYTES, a.st, c->plan.dev, a.src, a.y_out, c->n_rows,
                          c->g[0].n_cols, a.n_slabs, keep_mask_of(a.keep, a.n_slabs), unit_list_of(a.units, a.unit_count, grid, a.n_slabs));
}

// Layer 2 of a stack whose first layer has one input channel, straight from the first layer's shifted-input records
// (fwd_c32_from_y): H1 is rebuilt in LDS, never stored.  Dense launches, 32 channels.
bool blocked_forward_from_y_supported(const scn_conv_s* c, int ns, int ch) {
    return scone_shape(c) && ns == BK_NS && ch == 32 && c->n_rows == c->g[0].n_cols;
}

int blocked_forward_from_y(scn_conv_s* c, const FromYLaunch& a) {
    const int n_slabs = a.n_slabs;
    const float* const* W = a.W;
    const FirstW fw{{a.W_first[0], a.W_first[1], a.W_first[2]}};
    const size_t lds = smem_bytes_c32(W16_EXTRA_BYTES + W16_FIRSTW_BYTES);
    const BlockedLaunch L = blocked_launch(c, n_slabs, lds);
    if (a.keep && !keep_fits(L.grid.y, n_slabs)) return SCN_ERR_UNSUPPORTED;
    return with_act(a.act, [&](auto A) -> int {
        constexpr int ACT = decltype(A)::value;
        if (a.keep)
            return launch_checked(fwd_c32_from_y_keep<ACT>, L.grid, dim3(W16_THREADS), lds + WSCAN_LDS_BYTES, a.st, L.P, a.y, nullptr, W[0], W[1], W[2],
                                  a.out, L.nr, L.nc, n_slabs, NO_LIST, fw, keep_mask_of(a.keep, n_slabs),
                                  unit_list_of(a.units, a.unit_count, L.grid, n_slabs));
        return launch_checked(fwd_c32_from_y<ACT>, L.grid, dim3(W16_THREADS), lds, a.st, L.P, a.y, nullptr, W[0], W[1], W[2],
                              a.out, L.nr, L.nc, n_slabs, NO_LIST, fw, NO_KEEP, NO_UNITS);
    });
}

bool blocked_backward_supported(const scn_conv_s* c, int ns, const int32_t* c_dz, int c_aux) {
    if (!scone_shape(c) || ns != BK_NS) return false;
    const int cd = c_dz[0];
    return (cd == 32 && c_aux == 32) || (cd == 16 && c_aux == 16);      // (one input channel: scn_conv_dw_first)
}

// C = 16 runs the C = 32 kernel on slab pairs (a dedicated 16 x 16-tile kernel was built in round 4 and lost: profiles/r04_bwd16_ab.txt,
// profiles/r04_bwd16_and_elastic_experiments.patch), so every form of the backward has one LDS footprint.
static size_t bwd_lds() {
    return smem_bytes_c32(B32_EXTRA_BYTES);                      // staging buffers + ELL + weight and selection fragments
}

// workgroups of a backward launch without a work list: each owns one set of weight-gradient partials in the workspace
static size_t bwd_workgroups(const scn_conv_s* c, int n_slabs) {
    const dim3 grid = launch_grid(c, n_slabs, bwd_lds());
    return (size_t)grid.x * grid.y;
}

size_t blocked_backward_workspace(const scn_conv_s* c, int n_slabs, int ns, const int32_t* c_dz, int c_aux) {
    if (!blocked_backward_supported(c, ns, c_dz, c_aux)) return 0;
    return bwd_workgroups(c, n_slabs) * c_aux * 3 * c_dz[0] * sizeof(float);
}

int blocked_backward(scn_conv_s* c, const BwdLaunch& a) {
    const int n_slabs = a.n_slabs, cd = a.c_dz, c_aux = a.c_aux;
    const float* const* W = a.W;
    const WorkList& wl = a.wl;
    float* partial = (float*)a.ws;
    const size_t lds = bwd_lds();
    const BlockedLaunch L = blocked_launch(c, n_slabs, lds, wl);
    if (a.dx_partial && (c_aux != 32 || !a.dx)) return SCN_ERR_UNSUPPORTED;
    const uint32_t* mask = a.dzmask ? a.dzmask : a.visit;
    if (mask && ((a.dzmask && a.visit) || a.dx_partial || wl.block || c_aux != 32 || cd != 32 || !keep_fits(L.grid.y, n_slabs))) return SCN_ERR_UNSUPPORTED;
    const int st_k = with_act(a.act, [&](auto A) -> int {
        constexpr int ACT = decltype(A)::value;
        if (mask)
            return launch_checked(a.dzmask ? bwd_c32_plain_dzmask<ACT> : bwd_c32_plain_visit<ACT>, L.grid, dim3(BK_THREADS),
                                  lds + (a.dzmask ? 0 : VISIT_LDS_BYTES), a.st, L.P, a.dz, nullptr, W[0], W[1], W[2], a.aux, a.dx, partial, L.nr, L.nc,
                                  n_slabs, wl, nullptr, NO_FIRSTW, keep_mask_of(mask, n_slabs), a.dzmask ? 0 : visit_flags(), a.dzmask ? nullptr : c->plan.blk_rec);
        const auto k = c_aux != 32 ? bwd_c32_pair<ACT> : (a.dx_partial ? bwd_c32_accum<ACT> : bwd_c32_plain<ACT>);
        return launch_checked(k, L.grid, dim3(BK_THREADS), lds, a.st, L.P, a.dz, a.dx_partial, W[0], W[1], W[2], a.aux, a.dx, partial, L.nr, L.nc,
                              n_slabs, wl, nullptr, NO_FIRSTW, NO_KEEP, 0, nullptr);
    });
    if (st_k != SCN_OK) return st_k;
    if (a.defer_n_wg) {
        *a.defer_n_wg = L.n_wg();
        return SCN_OK;
    }
    return reduce_dw(partial, L.n_wg(), c_aux, cd, a.dW, a.st);
}

// Backward of the layer that follows the first one, fused with the first layer's weight gradient (bwd_c32_first and its kin).
// Workspace: [this layer's dW partials][dW_first partials: 96 floats per workgroup].
bool blocked_backward_first_supported(const scn_conv_s* c, int ns, int ch) {
    return scone_shape(c) && ns == BK_NS && (ch == 32 || ch == 16);          // 16: the slab-pair form
}

size_t blocked_backward_first_workspace(const scn_conv_s* c, int n_slabs, int ns, int ch) {
    if (!blocked_backward_first_supported(c, ns, ch)) return 0;
    return bwd_workgroups(c, n_slabs) * (3 * ch * ch + 96) * sizeof(float);
}

// dW_first[slot][cc] of the slab-pair form: partial [b][slot * 32 + 16 s + cc], the two slabs s folded here (fixed order)
__device__ __forceinline__ void dw_first_reduce_pair_body(int o, int lane, const float* __restrict__ partial, int n_partials,
                                                          float* __restrict__ dW0, float* __restrict__ dW1, float* __restrict__ dW2) {
    // o = slot * 16 + cc
    const int slot = o >> 4, cc = o & 15;
    float s = 0.f;
    for (int b = lane; b < n_partials; b += 64) s += partial[(size_t)b * 96 + slot * 32 + cc] + partial[(size_t)b * 96 + slot * 32 + 16 + cc];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0) {
        float* d = slot == 0 ? dW0 : (slot == 1 ? dW1 : dW2);
        d[cc] += s;
    }
}
__global__ __launch_bounds__(64) void dw_first_reduce_pair_kernel(const float* __restrict__ partial, int n_partials,
                                                                  float* __restrict__ dW0, float* __restrict__ dW1,
                                                                  float* __restrict__ dW2) {
    dw_first_reduce_pair_body(blockIdx.x, threadIdx.x, partial, n_partials, dW0, dW1, dW2);
}

int blocked_backward_first(scn_conv_s* c, const BwdFirstLaunch& a) {
    const int n_slabs = a.n_slabs, ch = a.ch;
    const float* const* W = a.W;
    const WorkList& wl = a.wl;
    const size_t lds = bwd_lds();
    const BlockedLaunch L = blocked_launch(c, n_slabs, lds, wl);
    const int n_wg = L.n_wg();
    float* partial = (float*)a.ws;
    float* partial_first = partial + (size_t)n_wg * 3 * ch * ch;
    if (a.W_first && ch != 32) return SCN_ERR_UNSUPPORTED;
    if (a.visit && (!a.W_first || wl.block || !keep_fits(L.grid.y, n_slabs))) return SCN_ERR_UNSUPPORTED;
    const FirstW fw = a.W_first ? FirstW{{a.W_first[0], a.W_first[1], a.W_first[2]}} : NO_FIRSTW;
    int st_k = with_act(a.act, [&](auto A) -> int {
        constexpr int ACT = decltype(A)::value;
        if (a.visit)
            return launch_checked(bwd_c32_first_from_y_visit<ACT>, L.grid, dim3(BK_THREADS), lds + VISIT_LDS_BYTES, a.st, L.P, a.dz, a.y, W[0], W[1], W[2],
                                  nullptr, nullptr, partial, L.nr, L.nc, n_slabs, wl, partial_first, fw, keep_mask_of(a.visit, n_slabs), visit_flags(), c->plan.blk_rec);
        const auto k = a.W_first ? bwd_c32_first_from_y<ACT> : (ch == 32 ? bwd_c32_first<ACT> : bwd_c32_first_pair<ACT>);
        return launch_checked(k, L.grid, dim3(BK_THREADS), lds, a.st, L.P, a.dz, a.y, W[0], W[1], W[2], a.W_first ? nullptr : a.aux, nullptr, partial,
                              L.nr, L.nc, n_slabs, wl, partial_first, fw, NO_KEEP, 0, nullptr);
    });
    if (st_k == SCN_OK && a.defer_n_wg) {
        *a.defer_n_wg = n_wg;
        return SCN_OK;
    }
    if (st_k == SCN_OK) st_k = reduce_dw(partial, n_wg, ch, ch, a.dW, a.st);
    if (st_k != SCN_OK) return st_k;
    if (ch == 32)
        return launch_checked(dw_first_reduce_kernel, dim3(96), dim3(64), 0, a.st, partial_first, n_wg, 32, a.dW_first[0], a.dW_first[1],
                              a.dW_first[2]);
    return launch_checked(dw_first_reduce_pair_kernel, dim3(48), dim3(64), 0, a.st, partial_first, n_wg, a.dW_first[0], a.dW_first[1],
                          a.dW_first[2]);
}

// (with a y handed in the operator only supplies the row count and, for work lists, the block table)
bool blocked_dw_first_supported(const scn_conv_s* c, int ns, int cd) {
    return c->plan.built && c->n_groups == 1 && ns == BK_NS && (cd == 16 || cd == 32);
}

static size_t dw_first_y_bytes(const scn_conv_s* c, int n_slabs) {
    const size_t b = (size_t)n_slabs * c->n_rows * BK_NS * Y_STRIDE * sizeof(float);
    return (b + 255) / 256 * 256;
}

size_t blocked_dw_first_workspace(const scn_conv_s* c, int n_slabs, int ns, int cd) {
    if (!blocked_dw_first_supported(c, ns, cd)) return 0;
    return dw_first_y_bytes(c, n_slabs) + (size_t)DWS_BLOCKS * 3 * cd * sizeof(float);
}

// y != nullptr: the shifted input saved by the forward (scn_conv_forward_first); otherwise it is computed here into ws.
// wlp: zero-skipping work list (requires y).
int blocked_dw_first(scn_conv_s* c, int n_slabs, const float* x, const float* y, const float* dz, int cd, float* const* dW,
                     void* ws, const WorkList* wlp, hipStream_t st) {
    const PlanDev& P = c->plan.dev;
    float* partial = (float*)((char*)ws + dw_first_y_bytes(c, n_slabs));
    if (wlp && wlp->block) {
        if (!y) return SCN_ERR_BAD_ARG;
        if (cd == 32)
            hipLaunchKernelGGL(dw_first_list_kernel<32>, dim3(DWS_BLOCKS), dim3(DWS_THREADS), 0, st, P, *wlp, y, dz, partial,
                               c->n_rows);
        else
            hipLaunchKernelGGL(dw_first_list_kernel<16>, dim3(DWS_BLOCKS), dim3(DWS_THREADS), 0, st, P, *wlp, y, dz, partial,
                               c->n_rows);
        SCN_LAUNCH_CHECK();
        hipLaunchKernelGGL(dw_first_reduce_kernel, dim3(3 * cd), dim3(64), 0, st, partial, DWS_BLOCKS, cd, dW[0], dW[1], dW[2]);
        SCN_LAUNCH_CHECK();
        return SCN_OK;
    }
    if (!y) {
        if (!scone_shape(c)) return SCN_ERR_UNSUPPORTED;          // recomputing y needs identity + two value arrays
        float* Y = (float*)ws;
        const size_t lds = smem_bytes(16);
        hipLaunchKernelGGL(gather3_c1_kernel, launch_grid(c, n_slabs, lds), dim3(BK_THREADS), lds, st, P, x, Y, c->n_rows, c->g[0].n_cols,
                           n_slabs);
        SCN_LAUNCH_CHECK();
        y = Y;
    }
    const int64_t n_points = (int64_t)n_slabs * c->n_rows * BK_NS;
    if (cd == 32)
        hipLaunchKernelGGL(dw_first_stream_kernel<32>, dim3(DWS_BLOCKS), dim3(DWS_THREADS), 0, st, y, dz, partial, n_points);
    else
        hipLaunchKernelGGL(dw_first_stream_kernel<16>, dim3(DWS_BLOCKS), dim3(DWS_THREADS), 0, st, y, dz, partial, n_points);
    SCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(dw_first_reduce_kernel, dim3(3 * cd), dim3(64), 0, st, partial, DWS_BLOCKS, cd, dW[0], dW[1], dW[2]);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int blocked_clear_list(scn_conv_s* c, int ns, int ch, float* t, const WorkList* wl, hipStream_t st) {
    if (!c->plan.built || ns != BK_NS || !wl || !wl->block || (ns * ch) % 4) return SCN_ERR_UNSUPPORTED;
    if (wl->n_work == 0) return SCN_OK;
    hipLaunchKernelGGL(clear_list_kernel, dim3(std::min(wl->n_work, 2048)), dim3(256), 0, st, c->plan.dev, *wl, t, c->n_rows,
                       ns * ch);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int blocked_clear_mask(scn_conv_s* c, int n_slabs, int ns, int ch, float* t, const uint32_t* mask, hipStream_t st) {
    if (!c->plan.built || ns != BK_NS || (ns * ch) % 4 || (reinterpret_cast<uintptr_t>(t) & 15)) return SCN_ERR_UNSUPPORTED;
    return launch_checked(clear_mask_kernel, dim3(std::min(c->plan.dev.n_blocks, 2048)), dim3(256), 0, st, c->plan.dev,
                          keep_mask_of(mask, n_slabs), t, c->n_rows, n_slabs, ns * ch);
}

// scn_window_scan_probe: the walk of the masked kernels (WindowWalk) on gx workgroups, written out (window_scan_probe_kernel).
int blocked_window_scan_probe(scn_conv_s* c, int n_slabs, const uint32_t* mask, int gx, int slab0, int n_it, int cap, int32_t* out_block,
                              uint64_t* out_window, int32_t* out_count, int32_t* unit_block, hipStream_t st) {
    if (!c->plan.built) return SCN_ERR_UNSUPPORTED;
    PlanDev P = c->plan.dev;
    P.assign = balanced_assignment(c, gx);
    return launch_checked(window_scan_probe_kernel, dim3(gx), dim3(256), 0, st, P, keep_mask_of(mask, n_slabs), slab0, n_it, cap, out_block,
                          out_window, out_count, unit_block);
}

// ---- "power" layers: one operator S (identity + one value array), three terms  X0, S-input's own row, S * input ----
static bool power_shape(const scn_conv_s* c) {
    return c->plan.built && c->n_groups == 1 && c->g[0].identity == 1 && c->g[0].n_vals == 1;
}
bool blocked_power_supported(const scn_conv_s* c, int ns, int ch) {
    return power_shape(c) && ns == BK_NS && (ch == 32 || ch == 16);         // 16: on slab pairs, as the plain layers
}

size_t blocked_power_backward_workspace(const scn_conv_s* c, int n_slabs, int ns, int ch) {
    if (!blocked_power_supported(c, ns, ch)) return 0;
    return bwd_workgroups(c, n_slabs) * ch * 3 * ch * sizeof(float);
}

int blocked_power_forward(scn_conv_s* c, int n_slabs, const float* x0, const float* x, const float* const* W, int ch, int act,
                          float* out, hipStream_t st) {
    const size_t lds = ch == 32 ? smem_bytes_c32(W16_EXTRA_BYTES) : smem_bytes_c32(16 + 64);
    const BlockedLaunch L = blocked_launch(c, n_slabs, lds);
    return with_act(act, [&](auto A) -> int {
        constexpr int ACT = decltype(A)::value;
        if (ch == 16)
            return launch_checked(fwd_c16_power<ACT>, L.grid, dim3(W16_THREADS), lds, st, L.P, x, x0, W[0], W[1], W[2], out, L.nr, L.nc,
                                  n_slabs, NO_LIST, NO_KEEP);
        return launch_checked(fwd_c32_power<ACT>, L.grid, dim3(W16_THREADS), lds, st, L.P, x, x0, W[0], W[1], W[2], out, L.nr, L.nc, n_slabs,
                              NO_LIST, NO_FIRSTW, NO_KEEP, NO_UNITS);
    });
}

int blocked_power_backward(scn_conv_s* c, int n_slabs, const float* dz, const float* g1, const float* const* W,
                           const float* aux, int ch, int act, float* dx, float* const* dW, void* ws, hipStream_t st) {
    const size_t lds = bwd_lds();
    const BlockedLaunch L = blocked_launch(c, n_slabs, lds);
    float* partial = (float*)ws;
    const int st_k = with_act(act, [&](auto A) -> int {
        constexpr int ACT = decltype(A)::value;
        return launch_checked(ch == 32 ? bwd_c32_power<ACT> : bwd_c32_power_pair<ACT>, L.grid, dim3(BK_THREADS), lds, st, L.P, g1, dz, W[0],
                              W[1], W[2], aux, dx, partial, L.nr, L.nc, n_slabs, NO_LIST, nullptr, NO_FIRSTW, NO_KEEP, 0, nullptr);
    });
    return st_k != SCN_OK ? st_k : reduce_dw(partial, L.n_wg(), ch, ch, dW, st);
}

bool blocked_spmm_supported(const scn_conv_s* c, int k) {
    return c->plan.built && c->n_groups == 1 && k % 4 == 0 && k >= 4 && k <= 128;
}

int blocked_spmm(scn_conv_s* c, int n_slabs, int k, const float* x, float* ya, float* yb, hipStream_t st) {
#ifdef SCN_AB_SPMM_TWO_BUFFERS                                                  // diagnostic builds: the two-buffer kernel for every K
    const bool ring = false;
#else
    const bool ring = k == 128 || k == 64;
#endif
    if (ring) {
        const size_t lds = smem_bytes(k * 4, 16);
        const BlockedLaunch L = blocked_launch(c, n_slabs, lds);
        const auto kern = k == 128 ? (yb ? spmm_ring_dual<2> : spmm_ring_single<2>) : (yb ? spmm_ring_dual<1> : spmm_ring_single<1>);
        return launch_checked(kern, L.grid, dim3(SP_THREADS), lds, st, L.P, x, ya, yb, L.nr, L.nc, n_slabs);
    }
    // narrow operands: fold consecutive slabs into one staged piece (see dma_stage_sp) until it is 128 floats wide
#ifdef SCN_AB_SPMM_NO_BATCH                                                     // diagnostic builds: one slab per staged piece
    const int batch = 1;
#else
    const int batch = k > 32 ? 1 : std::max(1, std::min(n_slabs, 128 / k));
#endif
    const size_t lds = smem_bytes(k * 4 * batch, 16);
    const BlockedLaunch L = blocked_launch(c, (n_slabs + batch - 1) / batch, lds);      // the grid splits staged pieces, not slabs
    return launch_checked(yb ? spmm_blocked_dual : spmm_blocked_single, L.grid, dim3(SP_THREADS), lds, st, L.P, x, ya, yb, L.nr, L.nc,
                          n_slabs, k, batch);
}
