// Fused Bunch (SCCONV) layer: included at the end of namespace scn in scn_blocked.hip (shares its LDS / gather / split helpers).
//
// bunch_func (TE:173-195) applies, per layer, seven shifts S_ab between the three levels (nodes, edges, faces) and sums per
// target level:   out_l = relu( sum over source levels j of (S_{j -> l} X_j) W_{j -> l} ).
// Here the seven shifts are ONE square operator on the concatenated row space [nodes | edges | faces] ("cat" rows: an index
// space only -- the three level tensors stay separate, contiguous allocations); every entry carries its TERM = the level of its
// column, every row its CLASS = its own level.  A row has at most three terms, so the layer has the scone layer's shape --
// three gathered segments against three weight matrices -- with the weight set picked by the row's class:
//   forward :  out[r] = act( sum_j G_j[r] W[class(r)][j] ),   G_j[r] = sum over entries of row r with term j of val * X[col]
//   backward:  the same on the TRANSPOSED cat operator (rows = the layer's input rows, terms = the levels the row feeds):
//              dx = (sum_j G_j W[class][j]^T) * act'(aux),  dW[class][j] += aux^T G_j      (G_j gathered from dz)
//
// BLOCKS ARE SPATIAL PATCHES ACROSS THE LEVELS.  A row's sources sit in all three levels, so a block of one level alone
// would spend its staged sources on the other two (measured: 18 rows per 128 sources).  Instead every level keeps its own
// locality order and the caller hands in the MERGED order of the three (level of the i-th simplex along one space-filling
// curve): a block takes the next simplices along that curve -- up to bins[l] rows of level l, contiguous in level l's own
// tensor -- and its sources are the patch itself plus a one-ring halo (2.4-2.6 sources per row, 38-50 rows per block).
// Inside a block the waves are bound to levels STATICALLY (bins[] in units of the wave's rows), so a wave's MFMA tile is
// class-pure, its weight fragments and -- in the backward -- its weight-gradient accumulators never change.
//
// LDS (one workgroup per CU):  [buffer 0: 112 x 512 B][ELL slots, source rows, tables: 3 KB in the gap][buffer 1 at +64 KB]
//                              [hi / lo weight fragments of all seven matrices: 28 KB][selection fragments, backward: 2 KB][ELL values: 9 KB]
// (round 5: the two-part weight fragments take 28 KB instead of the 42 KB of the three-way split; the ELL values moved behind them and
// a block stages 112 sources instead of 104)

constexpr int TK_SRC = 112;                      // staged sources per block (the seven weight matrices take the rest of the LDS)
constexpr int TK_WSLOT_BYTES = 2 * 2 * 64 * 16;  // one matrix: [k-step / co tile][hi, lo][lane] x 8 f16
constexpr int TK_WRED_BYTES = 64;                // one word per wave (terms_weights_abs_max)
constexpr int TK_OFF_ENC = TK_SRC * 512, TK_OFF_SRC = TK_OFF_ENC + BK_ELL_CAP * 2,
              TK_OFF_TAB = TK_OFF_SRC + TK_SRC * 4, TK_OFF_BUF1 = 65536, TK_OFF_W = TK_OFF_BUF1 + TK_SRC * 512;
// L2 prefetch distance of the fused forward, in slabs past the one being staged; 0 = no prefetch (the default since the round-3
// staging fixes: with the wave's LDS-DMA instructions no longer a memory round trip apart the prefetch costs 3.5 %; it had bought
// 8 % before).  -DSCN_PF_DIST=1|2 builds bring it back for A/B runs.
#ifndef SCN_PF_DIST
#define SCN_PF_DIST 0
#endif
constexpr int TK_OFF_DUMP = TK_OFF_TAB + 128;    // where the L2-prefetch LDS-DMAs drop their 4 bytes per lane (<= 56 lanes)
static_assert(TK_OFF_DUMP + 56 * 4 <= TK_OFF_BUF1, "ELL arrays, tables and the prefetch dump live in the gap between the two staging buffers");
constexpr int TK_OFF_V = TK_OFF_W + 7 * TK_WSLOT_BYTES + 2048 + TK_WRED_BYTES;     // ELL values: behind the weight / selection fragments
constexpr int TK_LDS_BYTES = TK_OFF_V + BK_ELL_CAP * 8;
static_assert(TK_LDS_BYTES <= 160 * 1024, "weight (+ selection) fragments and the ELL values fit");

// largest |W| over the (up to seven) weight matrices of a fused Bunch layer as a bit pattern, known to every thread; ends in a barrier.
// ONE power-of-two scale serves them all (a wave's three matrices share its accumulator; see scn_blk_fwd.inc for the split).
// bad: some weight is NaN / Inf (no zero-tile early-out, see block_abs_max).
template <int NT>
__device__ __forceinline__ uint32_t terms_weights_abs_max(const float* const (&W)[9], uint32_t* red, bool& bad) {
    float m = 0.f;
    bool nf = false;
#pragma unroll
    for (int sl = 0; sl < 9; ++sl) {
        const float* Wg = W[sl];
        if (!Wg || sl == 2 || sl == 6) continue;
        for (int i = threadIdx.x; i < 32 * 32; i += NT) {
            const float v = Wg[i];
            m = fmaxf(m, fabsf(v));
            nf |= not_finite(v);
        }
    }
    return block_abs_max<NT>(m, nf, red, bad);
}

struct TermsDev {
    int32_t n_blocks;
    int32_t bins[3];             // rows of level l a block can hold (multiples of the kernel's rows per wave)
    int32_t lvl_rows[3];         // rows of each level tensor
    int32_t lvl_row0[3];         // cat index where level l begins (column indices of the operator are cat indices)
    const int32_t* blk_row0;     // [n_blocks][3] first row of the block inside level l's tensor
    const uint8_t* blk_rows;     // [n_blocks][4]  rows of level l in the block, [3] = staged sources
    const uint8_t* blk_w;        // [n_blocks][4]  padded ELL width of level l's rows, [3] unused
    const uint8_t* grp;          // [n_blocks][16][5]: off1, off2, n0, n1, n2 of every row group (4 rows forward, 8 rows backward)
    const int32_t* src_ptr;      // [n_blocks + 1]
    const int32_t* src_rows;     // staged source rows (cat indices) by slot (slot & 3 = LDS bank class, scn_blk_layout.inc)
    const int32_t* ell_ptr;      // [n_blocks]
    const uint16_t* ell_enc;
    const float2* ell_v;
};

struct TermsPtrs {               // kernel arguments by value
    const float* x[3];           // forward: the three level tensors; backward: dz of the three levels (nullptr = identically zero)
    const float* aux[3];         // backward: the layer's forward input per level
    float* out[3];               // forward: outputs; backward: dx (nullptr = not wanted: those rows are skipped)
    const float* W[9];           // [class][term], [32][32] row-major (nullptr = term absent)
    const float* y[3];           // backward, FIRST variant: the first layer's shifted 1-channel input of each level, [slab][row][4]
    float* partial_first;        //   and its per-(workgroup, wave) partial sums [n_wg][8][64]
};

// Block cut along the merged order: `merged[i]` = level of the i-th simplex along the curve (each level's rows appear in their
// own order).  group_rows = rows per wave of the kernel that will use the plan (4: forward, 8: backward).
int build_terms_plan(scn_conv_s* c, const uint8_t* term, const int32_t* lvl_row0, const uint8_t* merged, const int32_t* bins,
                     int group_rows) {
    const Group& G = c->g[0];
    const int n_rows = c->n_rows;
    // bins[l] == 0: level l's rows belong to no block (a layer whose level-l output nothing reads -- TE:198-201 only reads the
    // nodes of the last layer, so the layer before it needs no face output): the other levels get its share of a block's rows
    for (int l = 0; l < 3; ++l)
        if (bins[l] < 0 || bins[l] % group_rows) return SCN_ERR_BAD_ARG;
    if (bins[0] + bins[1] + bins[2] > BK_R || bins[0] + bins[1] + bins[2] == 0) return SCN_ERR_BAD_ARG;
    // (32-bit byte offsets inside a slab of a level's tensor, with the level in the two low bits: see the LDS-DMA words)
    if ((int64_t)n_rows * 512 >= (int64_t)1 << 32) return SCN_ERR_UNSUPPORTED;
    const int n_groups = BK_R / group_rows;
    const int binstart[3] = {0, bins[0], bins[0] + bins[1]};
    std::vector<int32_t> blk_row0, src_ptr(1, 0), src_rows, ell_ptr;
    std::vector<uint8_t> blk_rows, blk_w, grp, ell_slot;
    std::vector<float2> ell_v;
    std::vector<int32_t> mark(G.n_cols, -1), local(G.n_cols, 0), cur;
    std::vector<float> block_gather;
    cur.reserve(TK_SRC + 64);
#ifdef SCN_AB_LEGACY_LAYOUT                                   // diagnostic builds: slots in row order, entries in CSR order
    const bool optimise_layout = false;
#else
    const bool optimise_layout = true;
#endif
    LayoutProblem LP;
    std::vector<int> ent_j;                                   // entry id of the layout problem -> CSR position
    int64_t sim_positions = 0, sim_cycles = 0;
    int next_row[3] = {0, 0, 0};
    int bid = 0;
    int64_t total_src = 0;
    int pos = 0;
    while (pos < n_rows) {
        const int row0[3] = {next_row[0], next_row[1], next_row[2]};
        int cnt[3] = {0, 0, 0};
        int gw[16][3];                                        // even-padded term widths per row group (padded row index)
        for (int i = 0; i < 16; ++i) gw[i][0] = gw[i][1] = gw[i][2] = 0;
        cur.clear();
        auto level_w = [&](int l, int rows_l) {               // padded ELL width of level l's rows: max over its groups
            int w = 0;
            for (int i = 0; i < rows_l; i += group_rows) {
                const int gi = (binstart[l] + i) / group_rows;
                w = std::max(w, gw[gi][0] + gw[gi][1] + gw[gi][2]);
            }
            return w;
        };
        while (pos < n_rows) {
            const int l = merged[pos];
            if (l > 2 || next_row[l] >= lvl_row0[l + 1] - lvl_row0[l]) return SCN_ERR_BAD_ARG;
            if (bins[l] == 0) {                                 // a skipped level: its rows pass by
                ++next_row[l];
                ++pos;
                continue;
            }
            if (cnt[l] == bins[l]) break;
            const int r = lvl_row0[l] + next_row[l];
            const int j0 = G.h_rowptr[r], j1 = G.h_rowptr[r + 1];
            int add = 0, ct[3] = {0, 0, 0};
            for (int j = j0; j < j1; ++j) {
                if (mark[G.h_col[j]] != bid) ++add;
                ++ct[term[j]];
            }
            const int gi = (binstart[l] + cnt[l]) / group_rows;
            const int save[3] = {gw[gi][0], gw[gi][1], gw[gi][2]};
            for (int t = 0; t < 3; ++t) gw[gi][t] = std::max(gw[gi][t], (ct[t] + 1) & ~1);
            int ell = 0, wmax = 0;
            for (int q = 0; q < 3; ++q) {
                const int wq = level_w(q, cnt[q] + (q == l));
                wmax = std::max(wmax, wq);
                ell += wq * (cnt[q] + (q == l));
            }
            if ((int)cur.size() + add > TK_SRC || ell > BK_ELL_CAP || wmax > 254) {
                for (int t = 0; t < 3; ++t) gw[gi][t] = save[t];
                break;
            }
            for (int j = j0; j < j1; ++j)
                if (mark[G.h_col[j]] != bid) { mark[G.h_col[j]] = bid; cur.push_back(G.h_col[j]); }
            ++cnt[l];
            ++next_row[l];
            ++pos;
        }
        if (cnt[0] + cnt[1] + cnt[2] == 0) {
            if (pos >= n_rows) break;                               // only skipped rows were left
            return SCN_ERR_UNSUPPORTED;                             // a single row does not fit a block
        }
        std::sort(cur.begin(), cur.end());
        for (size_t i = 0; i < cur.size(); ++i) local[cur[i]] = (int32_t)i;
        int w[3], ebase[3];
        for (int l = 0; l < 3; ++l) w[l] = level_w(l, cnt[l]);
        ebase[0] = 0; ebase[1] = w[0] * cnt[0]; ebase[2] = ebase[1] + w[1] * cnt[1];     // rows stored compactly, level by level
        const int ell_total = ebase[2] + w[2] * cnt[2];
        for (int l = 0; l < 3; ++l) { blk_row0.push_back(row0[l]); blk_rows.push_back((uint8_t)cnt[l]); blk_w.push_back((uint8_t)w[l]); }
        blk_rows.push_back((uint8_t)cur.size());
        blk_w.push_back(0);
        // slot numbers of the sources and the order of the entries inside every (row group, term) segment: scn_blk_layout.inc.
        // A lane group of the kernels holds four rows: the forward's 4-row group, or one of the two quads of the backward's 8 rows.
        const int n_quad = group_rows / 4;
        LP.nsrc = (int)cur.size();
        LP.src.clear();
        LP.up.clear();
        LP.level.resize(cur.size());
        for (size_t i = 0; i < cur.size(); ++i) LP.level[i] = (int8_t)((cur[i] >= lvl_row0[1]) + (cur[i] >= lvl_row0[2]));
        LP.selfs.clear();
        LP.segs.clear();
        ent_j.clear();
        int seg_of[16][2][3];
        for (int gi = 0; gi < n_groups; ++gi)
            for (int qd = 0; qd < n_quad; ++qd)
                for (int t = 0; t < 3; ++t) {
                    seg_of[gi][qd][t] = -1;
                    if (gw[gi][t] == 0) continue;
                    seg_of[gi][qd][t] = (int)LP.segs.size();
                    LP.segs.emplace_back();
                    LP.segs.back().w = gw[gi][t];
                    LP.segs.back().pad_level = t;
                }
        auto lane_row = [&](int o, int& qd, int& k) {           // row o of a group -> (quad, row of the quad)
            if (group_rows == 4) { qd = 0; k = o; return; }
            qd = (o == 1 || o == 2 || o == 4 || o == 7) ? 1 : 0;
            for (k = 0; QUAD_ROWS[qd][k] != o; ++k) {}
        };
        for (int l = 0; l < 3; ++l)
            for (int i = 0; i < cnt[l]; ++i) {
                const int r = lvl_row0[l] + row0[l] + i, pr = binstart[l] + i;
                int qd, k;
                lane_row(pr % group_rows, qd, k);
                for (int j = G.h_rowptr[r]; j < G.h_rowptr[r + 1]; ++j) {
                    LP.segs[seg_of[pr / group_rows][qd][term[j]]].ent[k].push_back((int)LP.src.size());
                    LP.src.push_back(local[G.h_col[j]]);
                    LP.up.push_back(0);
                    ent_j.push_back(j);
                }
            }
        solve_layout(LP, optimise_layout);
        sim_positions += LP.positions;
        sim_cycles += LP.cycles;
        {
            const size_t sb = src_rows.size();
            src_rows.resize(sb + cur.size());
            for (size_t i = 0; i < cur.size(); ++i) src_rows[sb + LP.slot_of[i]] = cur[i];
        }
        src_ptr.push_back((int32_t)src_rows.size());
        ell_ptr.push_back((int32_t)ell_slot.size());
        const size_t base = ell_slot.size();
        ell_slot.resize(base + (size_t)ell_total, 0);
        ell_v.resize(base + (size_t)ell_total, float2{0.f, 0.f});
        uint8_t gt[16][5];
        std::memset(gt, 0, sizeof(gt));
        float gather = 0.f;
        for (int l = 0; l < 3; ++l)
            for (int i = 0; i < cnt[l]; ++i) {
                const int pr = binstart[l] + i, gi = pr / group_rows;
                const int off[3] = {0, gw[gi][0], gw[gi][0] + gw[gi][1]};
                int qd, k;
                lane_row(pr % group_rows, qd, k);
                for (int t = 0; t < 3; ++t) {
                    if (gw[gi][t] == 0) continue;
                    const LayoutSeg& S = LP.segs[seg_of[gi][qd][t]];
                    for (int q = 0; q < gw[gi][t]; ++q) {
                        const size_t e = base + (size_t)ebase[l] + (size_t)i * w[l] + off[t] + q;
                        const int id = S.out[k][q];
                        if (id >= 0) {
                            ell_slot[e] = LP.slot_of[LP.src[id]];
                            ell_v[e] = float2{G.h_val0[ent_j[id]], 0.f};
                        } else {
                            // a padding entry (value 0) reads a staged source of its own term's level: a level whose tensor is absent
                            // (identically zero input) is never staged, so a pad of a present term must not point into its LDS pieces
                            ell_slot[e] = (uint8_t)(-(id + 1));
                        }
                    }
                    gt[gi][2 + t] = (uint8_t)gw[gi][t];
                }
                gt[gi][0] = (uint8_t)off[1];
                gt[gi][1] = (uint8_t)off[2];
            }
        for (int i = 0; i < n_groups; ++i) gather += gt[i][2] + gt[i][3] + gt[i][4];
        block_gather.push_back(gather);
        grp.insert(grp.end(), &gt[0][0], &gt[0][0] + 80);
        total_src += (int64_t)cur.size();
        ++bid;
    }
    BlockPlan& B = c->plan;
    TermsPlan& T = c->terms;
    B.dev.n_blocks = bid;
    int st;
    if ((st = upload(c, blk_row0, &T.blk_row0)) != SCN_OK) return st;
    if ((st = upload(c, blk_rows, &T.blk_rows)) != SCN_OK) return st;
    if ((st = upload(c, blk_w, &T.blk_w)) != SCN_OK) return st;
    if ((st = upload(c, grp, &T.grp)) != SCN_OK) return st;
    if ((st = upload(c, src_ptr, &B.dev.src_ptr)) != SCN_OK) return st;
    if ((st = upload(c, src_rows, &B.dev.src_rows)) != SCN_OK) return st;
    if ((st = upload(c, ell_ptr, &B.dev.ell_ptr)) != SCN_OK) return st;
    std::vector<uint16_t> ell_enc(ell_slot.size());
    for (size_t i = 0; i < ell_slot.size(); ++i) ell_enc[i] = (uint16_t)((ell_slot[i] << 9) | ((ell_slot[i] & 3) << 5));
    if ((st = upload(c, ell_enc, &B.dev.ell_enc)) != SCN_OK) return st;
    if ((st = upload(c, ell_v, &B.dev.ell_v)) != SCN_OK) return st;
    for (int i = 0; i < 4; ++i) T.lvl_row0[i] = lvl_row0[i];
    for (int i = 0; i < 3; ++i) T.bins[i] = bins[i];
    T.group_rows = group_rows;
    B.mean_src_per_row = (double)total_src / std::max(1, n_rows);
    B.gather_positions = sim_positions;
    B.gather_cycles = sim_cycles;
    B.h_cost.assign(block_gather.begin(), block_gather.end());
    T.built = true;
    return SCN_OK;
}

static TermsDev terms_dev(const scn_conv_s* c) {
    TermsDev T;
    T.n_blocks = c->plan.dev.n_blocks;
    for (int i = 0; i < 3; ++i) {
        T.bins[i] = c->terms.bins[i];
        T.lvl_rows[i] = c->terms.lvl_row0[i + 1] - c->terms.lvl_row0[i];
        T.lvl_row0[i] = c->terms.lvl_row0[i];
    }
    T.blk_row0 = c->terms.blk_row0;
    T.blk_rows = c->terms.blk_rows;
    T.blk_w = c->terms.blk_w;
    T.grp = c->terms.grp;
    T.src_ptr = c->plan.dev.src_ptr;
    T.src_rows = c->plan.dev.src_rows;
    T.ell_ptr = c->plan.dev.ell_ptr;
    T.ell_enc = c->plan.dev.ell_enc;
    T.ell_v = c->plan.dev.ell_v;
    return T;
}

__device__ __forceinline__ SmemC32 carve_terms(char* base) {
    SmemC32 s;
    s.buf0 = base;
    s.v = (float2*)(base + TK_OFF_V);
    s.enc = (uint16_t*)(base + TK_OFF_ENC);
    s.srcrows = (int32_t*)(base + TK_OFF_SRC);
    s.self = (uint8_t*)(base + TK_OFF_TAB);                   // the row-group table lives where the scone kernels keep `self`
    return s;
}

// one term of a row: entries [rb, rb + cnt) (cnt even), single value per entry.  The first entry pair's slots and values come in
// from the caller, which requests them for all three terms at once (three short loops: their start-up latencies would add up).
template <int NQ>
__device__ __forceinline__ void gather_term_c32(const SmemC32& sm, int rb, int cnt, const uint32_t (&cb)[NQ], f32x4 (&g)[NQ],
                                                uint32_t ss, f32x4 v) {
    const char* lds = sm.buf0;
    // `first`: the term's first pair ASSIGNS the accumulator (no zeroing moves, as in gather_c32)
    auto pair = [&](int t, auto first) {
        const uint32_t e0 = ss & 0xffffu, e1 = ss >> 16;
        const f32x4 vc = v;
        f32x4 d0[NQ], d1[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) d0[q] = *(const f32x4*)(lds + (cb[q] ^ e0));
#pragma unroll
        for (int q = 0; q < NQ; ++q) d1[q] = *(const f32x4*)(lds + (cb[q] ^ e1));
        if (t + 2 < cnt) {
            ss = *(const uint32_t*)(sm.enc + rb + t + 2);
            v = *(const f32x4*)(sm.v + rb + t + 2);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            if (decltype(first)::value) g[q] = vc[0] * d0[q];
            else g[q] += vc[0] * d0[q];
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) g[q] += vc[2] * d1[q];
        __builtin_amdgcn_sched_barrier(0);
    };
#ifdef SCN_AB_GATHER_NO_PEEL
#pragma unroll
    for (int q = 0; q < NQ; ++q) g[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < cnt; t += 2) pair(t, std::false_type{});
#else
    if (cnt > 0) {                                             // (cnt is wave-uniform)
        pair(0, std::true_type{});
        for (int t = 2; t < cnt; t += 2) pair(t, std::false_type{});
    } else {
#pragma unroll
        for (int q = 0; q < NQ; ++q) g[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#endif
}

// ------------------------------------------------------------------------------------------------
// forward, 32 -> 32 channels: fwd_c32_w16_kernel's structure (sixteen waves, wave = 4 rows x 4 trajectories, exact bf16 split,
// staggered halves) with three gathered terms, sources staged from three tensors, waves bound to levels.
// ------------------------------------------------------------------------------------------------
// wave priorities by remaining work of the visit, as in fwd_c32_w16_kernel (SCN_FWD_PRIO_SEQ): terms_fwd -2 to -3 % in the same-box
// A/B (profiles/r04_sync_ab.txt, section 8); -DSCN_TERMS_PRIO_SEQ=0 = none
#ifndef SCN_TERMS_PRIO_SEQ
#define SCN_TERMS_PRIO_SEQ 0x32103321
#endif
#if SCN_TERMS_PRIO_SEQ != 0
template <int I> __device__ __forceinline__ void terms_prio() { __builtin_amdgcn_s_setprio((SCN_TERMS_PRIO_SEQ >> (4 * (7 - I))) & 3); }
#define SCN_TERMS_PRIO_GATHER() do { if (late) terms_prio<7>(); else terms_prio<0>(); } while (0)
#define SCN_TERMS_PRIO_CONTRACT(g) do { if (late) { if ((g) == 0) terms_prio<4>(); if ((g) == 1) terms_prio<5>(); if ((g) == 2) terms_prio<6>(); } \
                                         else { if ((g) == 0) terms_prio<1>(); if ((g) == 1) terms_prio<2>(); if ((g) == 2) terms_prio<3>(); } } while (0)
#else
#define SCN_TERMS_PRIO_GATHER()
#define SCN_TERMS_PRIO_CONTRACT(g)
#endif

template <int ACT>
__global__ __launch_bounds__(W16_THREADS, 4) void terms_fwd_c32_kernel(TermsDev T, TermsPtrs A, int n_slabs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PIECE = 512, CPP = 32, NDMA = 4;             // 4 x 1024 lanes cover 128 slots; slots >= nsrc are masked
    const SmemC32 sm = carve_terms(smem);
    const uint32_t lds0 = lds_addr_of(smem);                   // LDS byte address of the dynamic shared memory
    char* wfrag = smem + TK_OFF_W;
    const uint8_t* grp = sm.self;                              // [16][5] of the current block
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pt = lane & 15, kq = lane >> 4, n = pt >> 2;    // trajectory-major points: every ds_read_b128 lane group holds the wave's
                                                               // four rows with all four trajectories (scn_blk_layout.inc)
    // this wave's level, and the local index (inside the block's rows of that level) of its first row.  Row groups are dealt
    // to waves so that consecutive groups alternate between the early and the late half (a level's first groups are the ones
    // that have rows: both halves of the stagger get their share): group slot = 2 * (wave & 7) + (wave >> 3).
    const int slot = __builtin_amdgcn_readfirstlane(((wave & 7) << 1) | (wave >> 3));
    const int w0n = T.bins[0] >> 2, w1n = T.bins[1] >> 2;
    const int lw = (slot >= w0n) + (slot >= w0n + w1n);
    const int wrow0 = (slot - (lw == 0 ? 0 : (lw == 1 ? w0n : w0n + w1n))) * 4;      // (wave-uniform)
    const int lrow = wrow0 + (pt & 3);
    // the seven weight matrices, split once under one scale: slot cls * 3 + g -> fragment (ct, part, lane) = W[8*kq' + j][16*ct + i] * sW
    float invW;
    bool w_bad;
    const float sW = pow2_scale(terms_weights_abs_max<W16_THREADS>(A.W, (uint32_t*)(wfrag + 7 * TK_WSLOT_BYTES + 2048), w_bad), invW);
    for (int f = tid; f < 9 * 2 * 64; f += W16_THREADS) {
        const int sl = f / 128, ct = (f >> 6) & 1, l = f & 63;
        const float* Wg = A.W[sl];
        if (!Wg || sl == 2 || sl == 6) continue;               // nodes have no face term, faces no node term: 7 slots stored
        const int store = sl - (sl > 2) - (sl > 6);
        float w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = Wg[(8 * (l >> 4) + j) * 32 + 16 * ct + (l & 15)];
        const Split2 sp = split2(w, sW);
        char* base = wfrag + store * TK_WSLOT_BYTES + (ct * 2) * 1024 + l * 16;
        *(f16x8*)(base) = sp.hi;
        *(f16x8*)(base + 1024) = sp.lo;
    }
    unsigned present = 0;                                      // bit g: term g of this wave's class has a weight and a source tensor
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const int sl = lw * 3 + g;
        if (sl != 2 && sl != 6 && A.W[sl] && (g == 0 ? A.x[0] : (g == 1 ? A.x[1] : A.x[2]))) present |= 1u << g;
    }
    const char* wbase[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const int sl = lw * 3 + g;
        wbase[g] = wfrag + (sl - (sl > 2) - (sl > 6)) * TK_WSLOT_BYTES + lane * 16;
    }
    float* const outb = lw == 0 ? A.out[0] : (lw == 1 ? A.out[1] : A.out[2]);
    const int out_rows = lw == 0 ? T.lvl_rows[0] : (lw == 1 ? T.lvl_rows[1] : T.lvl_rows[2]);
    int b, b_end, b_stride;
    block_range(T.n_blocks, b, b_end, b_stride);
    SCN_SLAB_RANGE();
    if (slab0 >= slab1) return;
    const int n_it = slab1 - slab0;
    f32x4 pend[2];
    float* pend_ptr = nullptr;
    bool pend_valid = false;
    uint32_t cqs[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) cqs[q] = (uint32_t)((n * 8 + kq * 2 + q) ^ (n >> 1)) << 4;
    const int r1 = T.lvl_row0[1], r2 = T.lvl_row0[2];
    const size_t sb0 = (size_t)T.lvl_rows[0] * PIECE, sb1 = (size_t)T.lvl_rows[1] * PIECE, sb2 = (size_t)T.lvl_rows[2] * PIECE;
    auto run = [&](auto late_c) {
    constexpr int late = decltype(late_c)::value;
    for (; b < b_end; b += b_stride) {
        wait_all_and_barrier();
        const int nsrc = T.blk_rows[b * 4 + 3];
        const int my_rows = outb ? T.blk_rows[b * 4 + lw] : 0;     // rows of this wave's level in the block (0: level not wanted)
        const int my_w = T.blk_w[b * 4 + lw];
        const int e1 = T.blk_w[b * 4] * T.blk_rows[b * 4], e2 = e1 + T.blk_w[b * 4 + 1] * T.blk_rows[b * 4 + 1];
        const int my_ebase = lw == 0 ? 0 : (lw == 1 ? e1 : e2);
        const int my_row0 = T.blk_row0[b * 3 + lw];
        {
            const int sp0 = T.src_ptr[b];
            const int ep = T.ell_ptr[b];
            const int ell_n = e2 + T.blk_w[b * 4 + 2] * T.blk_rows[b * 4 + 2];
            for (int i = tid; i < nsrc; i += W16_THREADS) sm.srcrows[i] = T.src_rows[sp0 + i];
            for (int i = tid; i < ell_n; i += W16_THREADS) {
                sm.enc[i] = T.ell_enc[ep + i];
                sm.v[i] = T.ell_v[ep + i];
            }
            if (tid < 80) sm.self[tid] = T.grp[(size_t)b * 80 + tid];
        }
        __syncthreads();
        const uint8_t* mg = grp + slot * 5;
        const int off1 = __builtin_amdgcn_readfirstlane(mg[0]), off2 = __builtin_amdgcn_readfirstlane(mg[1]);   // wave-uniform: SGPRs
        const int cnt0 = (present & 1u) ? __builtin_amdgcn_readfirstlane(mg[2]) : 0, cnt1 = (present & 2u) ? __builtin_amdgcn_readfirstlane(mg[3]) : 0,
                  cnt2 = (present & 4u) ? __builtin_amdgcn_readfirstlane(mg[4]) : 0;
#if defined(SCN_TERMS_FLOOR) && SCN_TERMS_FLOOR == 1           // diagnostic build (results wrong by design): staging + barriers only
        const bool wave_rows = false;
#else
        const bool wave_rows = wrow0 < my_rows;                // a wave without rows only stages data and keeps the barriers
#endif
        const int lrc = lrow < my_rows ? lrow : (my_rows > 0 ? my_rows - 1 : 0);
        // LDS-DMA: instruction k of this wave stages slot 2 * (k * 16 + wave) + (lane >> 5); its source row is a cat index, i.e.
        // (level, row inside the level's tensor).  Per block and k one 32-bit word: byte offset of the chunk inside a slab of its
        // level's tensor | level (the offset is a multiple of 16); 3 = nothing to stage.
        const int total = nsrc * CPP;
        const uint32_t dchunk = (uint32_t)swz32(((wave & 1) << 1) | (lane >> 5), lane & 31) * 16;
        uint32_t goff[NDMA];
#pragma unroll
        for (int k = 0; k < NDMA; ++k) {
            const int base = (k * W16_WAVES + wave) * 64;
            uint32_t gv = 3u;
            if (base + lane < total) {
                const int r = sm.srcrows[2 * (k * W16_WAVES + wave) + (lane >> 5)];
                const int lv = (r >= r1) + (r >= r2);
                const bool have = lv == 0 ? A.x[0] != nullptr : (lv == 1 ? A.x[1] != nullptr : A.x[2] != nullptr);
                if (have) gv = ((uint32_t)(r - (lv == 0 ? 0 : (lv == 1 ? r1 : r2))) * PIECE + dchunk) | (uint32_t)lv;
            }
            goff[k] = gv;
        }
        // the three levels' slab bases of one staging round: wave-uniform, and SAID so (readfirstlane) -- with the kernel short of
        // SGPRs the compiler otherwise re-fetched the tensor pointers from the argument block with a VECTOR load at every LDS-DMA,
        // waited s_waitcnt vmcnt(0) for it (i.e. for every LDS-DMA issued before) and did slab * slab_bytes in quarter-rate
        // v_mul_*_u32: the wave's four instructions of a round then went out one memory round trip apart
        struct Bases { const char* p[3]; };
        auto uniform_ptr = [](const char* q) {
            const uint64_t v = (uint64_t)q;
            const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
            return (const char*)(((uint64_t)hi << 32) | lo);
        };
        auto bases = [&](int slab) {
            Bases B;
            B.p[0] = uniform_ptr((const char*)A.x[0] + slab * sb0);
            B.p[1] = uniform_ptr((const char*)A.x[1] + slab * sb1);
            B.p[2] = uniform_ptr((const char*)A.x[2] + slab * sb2);
            return B;
        };
        auto dma = [&](int k, const Bases& B, char* buf) {
#if defined(SCN_TERMS_FLOOR) && SCN_TERMS_FLOOR == 2           // diagnostic build (results wrong by design): no staging, gather + contraction only
            return;
#endif
            const int base = (k * W16_WAVES + wave) * 64;
            const uint32_t gv = goff[k], off = gv & ~3u, lv = gv & 3u;
            const uint32_t dst = lds0 + (uint32_t)((buf - smem) + base * 16);
            if (lv == 0) lds_dma16(B.p[0], off, dst);
            if (lv == 1) lds_dma16(B.p[1], off, dst);
            if (lv == 2) lds_dma16(B.p[2], off, dst);
        };
        // L2 PREFETCH of the slab after the one being staged: one 4-byte LDS-DMA per wave into a dump area touches every 128-byte
        // line of this wave's share of the pieces (lane -> instruction k = lane>>3, piece (lane>>2)&1, line lane&3), so the staging
        // one visit later finds its lines in L2.  These blocks are small and bound by the staging round trip with one slab in
        // flight (profiles/HISTORY.md section 3.1); in the 64-row scone kernels, which saturate the memory system, the same prefetch costs 7 %.
        // It is the wave's newest load when the slab wait comes: that wait is vmcnt(1) (loads return in order).
        uint32_t pgv = 3u;
        if (lane < 8 * NDMA && ((lane >> 3) * W16_WAVES + wave) * 64 + ((lane >> 2) & 1) * 32 < total) {
            const int r = sm.srcrows[2 * ((lane >> 3) * W16_WAVES + wave) + ((lane >> 2) & 1)];
            const int lv = (r >= r1) + (r >= r2);
            const bool have = lv == 0 ? A.x[0] != nullptr : (lv == 1 ? A.x[1] != nullptr : A.x[2] != nullptr);
            if (have) pgv = ((uint32_t)(r - (lv == 0 ? 0 : (lv == 1 ? r1 : r2))) * PIECE + (uint32_t)(lane & 3) * 128) | (uint32_t)lv;
        }
        auto prefetch = [&](int slab) {
            const uint32_t off = pgv & ~3u, lv = pgv & 3u;
            const Bases B = bases(slab);
            const uint32_t dst = lds0 + TK_OFF_DUMP;
            if (lv == 0) lds_dma4(B.p[0], off, dst);
            if (lv == 1) lds_dma4(B.p[1], off, dst);
            if (lv == 2) lds_dma4(B.p[2], off, dst);
        };
        bool pf_out = false;
        {
            const Bases B = bases(slab0);
#pragma unroll
            for (int i = 0; i < NDMA; ++i) dma(i, B, sm.buf(0));
        }
        if (late && n_it > 1) {
            const Bases B = bases(slab0 + 1);
#pragma unroll
            for (int i = 0; i < NDMA; ++i) dma(i, B, sm.buf(1));
        }
        f32x4 z[3][2];
        // ---------------- GATHER of slab slab0 + it (staged in buffer it & 1) into z
        auto gather_phase = [&](int it) {
            // (blocks are small: the contraction is too short to cover a staging round trip, so an early wave asks for the
            // next slab right after the barrier -- the buffer was last read before it -- instead of inside its MFMA chain)
            if (!late && it + 1 < n_it) {
                const Bases B = bases(slab0 + it + 1);
#pragma unroll
                for (int i = 0; i < NDMA; ++i) dma(i, B, sm.buf((it + 1) & 1));
            }
            if (wave_rows) {
                __builtin_amdgcn_s_waitcnt(0xC07F);                 // (see fwd_c32_w16_kernel: lets the compiler count the gather's LDS reads)
                const uint32_t cb[2] = {cqs[0] | (uint32_t)((it & 1) << 16), cqs[1] | (uint32_t)((it & 1) << 16)};
                const int rb = my_ebase + lrc * my_w;
                const uint32_t s0 = *(const uint32_t*)(sm.enc + rb), s1 = *(const uint32_t*)(sm.enc + rb + off1),
                               s2 = *(const uint32_t*)(sm.enc + rb + off2);      // (a term without entries: read, not used)
                const f32x4 v0 = *(const f32x4*)(sm.v + rb), v1 = *(const f32x4*)(sm.v + rb + off1), v2 = *(const f32x4*)(sm.v + rb + off2);
                gather_term_c32<2>(sm, rb, cnt0, cb, z[0], s0, v0);
                gather_term_c32<2>(sm, rb + off1, cnt1, cb, z[1], s1, v1);
                gather_term_c32<2>(sm, rb + off2, cnt2, cb, z[2], s2, v2);
            }
        };
        // ---------------- CONTRACT of slab slab0 + it from z
        auto contract_phase = [&](int it) {
            const int slab = slab0 + it;
            const int vdma = it + 1 + late;
            const bool more = late && vdma < n_it;             // (early waves staged the next slab before their gather)
            char* nbuf = sm.buf(vdma & 1);
            const Bases Bn = bases(slab0 + (more ? vdma : it));
            if (!wave_rows) {                                  // no rows: its share of the staging, and a tile still pending from the last block
                if (more) {
#pragma unroll
                    for (int i = 0; i < NDMA; ++i) dma(i, Bn, nbuf);
                }
                if (pend_ptr && pend_valid) {
                    *(f32x4*)(pend_ptr) = pend[0];
                    *(f32x4*)(pend_ptr + 16) = pend[1];
                }
                pend_valid = false;
                pf_out = SCN_PF_DIST > 0 && vdma + SCN_PF_DIST < n_it;
                if (pf_out) prefetch(slab0 + vdma + SCN_PF_DIST);
                return;
            }
            {
                const f32x4 prev0 = pend[0], prev1 = pend[1];
                float* const prev_ptr = pend_ptr;
                const bool prev_valid = pend_valid && pend_ptr != nullptr;
                f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
                // the point's scale (see fwd_c32_w16_kernel): largest magnitude among the gathered values of its present terms
                float inv, sz;
                float m = 0.f;
#pragma unroll
                for (int g = 0; g < 3; ++g)
                    if (present & (1u << g)) m = amaxn_2x4(m, z[g][0], z[g][1]);        // (NaN counts: scn_blk_fwd.inc)
                const bool tile_zero = !w_bad && __builtin_amdgcn_ballot_w64(m != 0.f) == 0;   // zero-tile early-out (see fwd_c32_w16_kernel)
                {
                    sz = pow2_scale(max_over_rows(__float_as_uint(m)), inv);
                    inv *= invW;
                }
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    SCN_TERMS_PRIO_CONTRACT(g);
                    if ((present & (1u << g)) && !tile_zero) {
                        float x8[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j) x8[j] = z[g][j >> 2][j & 3];
                        const Split2 zs = split2(x8, sz);
#pragma unroll
                        for (int ct = 0; ct < 2; ++ct) {
                            const char* wb = wbase[g] + (ct * 2) * 1024;
                            const f16x8 wh = *(const f16x8*)(wb), wl = *(const f16x8*)(wb + 1024);
                            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, zs.hi, acc[ct], 0, 0, 0);
                            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, zs.lo, acc[ct], 0, 0, 0);
                            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, zs.hi, acc[ct], 0, 0, 0);
                        }
                    }
                    // side slots: 4 LDS-DMA instructions + 2 stores, two per segment whether or not the segment has work
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) {
                        const int k = g * 2 + ct;
                        if (k < NDMA) {
                            if (more) dma(k, Bn, nbuf);
                        } else if (prev_valid) {
                            *(f32x4*)(prev_ptr + 16 * (k - NDMA)) = (k - NDMA) == 0 ? prev0 : prev1;
                        }
                    }
                }
                pf_out = SCN_PF_DIST > 0 && vdma + SCN_PF_DIST < n_it;                      // (after the stores: the newest vector-memory operation of the visit)
                if (pf_out) prefetch(slab0 + vdma + SCN_PF_DIST);
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) pend[ct][r] = act_apply_fast(ACT, acc[ct][r] * inv);
            }
            pend_ptr = outb + (((size_t)slab * out_rows + my_row0 + lrow) * BK_NS + n) * 32 + 4 * kq;
            pend_valid = lrow < my_rows;
        };
        // one barrier interval per slab (+ one for the late waves' last contraction): see fwd_c32_w16_kernel
        for (int v = 0; v <= n_it; ++v) {
            if (pf_out)
                asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (!late) {
                if (v < n_it) {
                    SCN_TERMS_PRIO_GATHER();
                    gather_phase(v);
                    contract_phase(v);
                }
            } else {
                if (v > 0) contract_phase(v - 1);
                SCN_TERMS_PRIO_GATHER();
                if (v < n_it) gather_phase(v);
            }
        }
    }
    };
    if (wave >> 3) run(std::integral_constant<int, 1>{});      // the early and the late half of the stagger as two compile-time paths
    else run(std::integral_constant<int, 0>{});
    if (pend_ptr && pend_valid) {
        *(f32x4*)(pend_ptr) = pend[0];
        *(f32x4*)(pend_ptr + 16) = pend[1];
    }
}

static size_t terms_fwd_lds() { return (size_t)TK_LDS_BYTES; }

static dim3 terms_grid(const scn_conv_s* c) {
    const int nb = c->plan.dev.n_blocks;
    return dim3(std::max(8, std::min(256, ((nb + 7) / 8) * 8) / 8 * 8), 1);
}

int terms_forward(scn_conv_s* c, int n_slabs, const float* const* x, const float* const* W, int act, float* const* out,
                  hipStream_t st) {
    if (c->terms.group_rows != 4) return SCN_ERR_UNSUPPORTED;     // a plan cut for the backward's 8-row waves
    const TermsDev T = terms_dev(c);
    TermsPtrs A;
    for (int i = 0; i < 3; ++i) { A.x[i] = x[i]; A.aux[i] = nullptr; A.out[i] = out[i]; }
    for (int i = 0; i < 9; ++i) A.W[i] = W[i];
    return with_act(act, [&](auto ACT) -> int {
        return launch_checked(terms_fwd_c32_kernel<decltype(ACT)::value>, terms_grid(c), dim3(W16_THREADS), terms_fwd_lds(), st, T, A,
                              n_slabs);
    });
}

// ------------------------------------------------------------------------------------------------
// backward, 32 <- 32 channels: bwd_c32_bf16_kernel's structure (eight waves, wave = 8 rows x 4 trajectories = a 32-point tile,
// exact bf16 split, transposes into three exact accumulators) on the TRANSPOSED operator: three gathered terms of dz, waves
// bound to levels -- so a wave's three weight-gradient accumulators belong to one class for the whole launch.
//   partial: [workgroup][wave][3 terms][32 x 32], reduced per class afterwards (terms_dw_reduce_kernel)
// ------------------------------------------------------------------------------------------------
// y broadcast of the FIRST variant: lane 16 k + r of yl holds y[pt(r, h)] (h = half wave of the lane: both 16-lane rows of a
// half hold the same sixteen values); DPP row_newbcast:r hands lane r of its own row to every lane -- one VALU instruction
// per value, no vector registers (sixteen ds_swizzle results in flight spilled 33 of them; v_readlane pairs cost 5 instructions
// per value and SGPR hazards)
template <int ACT, int R>
__device__ __forceinline__ void terms_first_step(float yl, float acc, float a, float& dwf) {
    // (the broadcast as the DPP operand of the FMA itself, as in bwd_c32_bf16_kernel<.., FIRST>: see first_dw_step)
    const float t = acc * act_grad_from_output(ACT, a);
    if (R == 0) asm volatile("s_nop 1\n\tv_fmac_f32_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0xf" : "+v"(dwf) : "v"(yl), "v"(t));
    else asm volatile("v_fmac_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(dwf) : "v"(yl), "v"(t), "n"(R));
}
template <int ACT, int... Rs>
__device__ __forceinline__ void terms_first_tile(std::integer_sequence<int, Rs...>, float yl, const f32x16& acc, const float (&a)[16],
                                                 float& dwf) {
    (terms_first_step<ACT, Rs>(yl, acc[Rs], a[Rs], dwf), ...);
}

// FIRST: the layer whose backward this is follows the 1-channel FIRST layer, so its input gradient dx (= gradient of the first
// layer's pre-activation) is needed for one thing only -- dW_first[level][c] = sum_p y[p] dx[p][c] with y = S x, the first layer's
// shifted input of that level -- and is contracted with y right here, in registers, instead of being written (no dx tensors, no
// streaming kernel over them: the Bunch counterpart of bwd_c32_bf16_kernel<..., FIRST>).
template <int ACT, bool FIRST>
__global__ __launch_bounds__(BK_THREADS, 2) void terms_bwd_c32_kernel(TermsDev T, TermsPtrs A, float* __restrict__ partial,
                                                                      int n_slabs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PIECE = 512, CPP = 32, NDMA = 8;             // 8 x 512 lanes cover 128 slots; slots >= nsrc are masked
    const SmemC32 sm = carve_terms(smem);
    const uint32_t lds0 = lds_addr_of(smem);                   // LDS byte address of the dynamic shared memory
    char* wfrag = smem + TK_OFF_W;
    char* isel = wfrag + 7 * TK_WSLOT_BYTES;
    const uint8_t* grp = sm.self;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p = lane & 31, h = lane >> 5, n = p & 3;
    // row-group slot of this wave: the groups that usually have no rows (a level's last ones) share a SIMD (waves w, w + 4) with
    // groups that do: wave -> slot  0 4 1 2 3 5 6 7 -> 0 1 2 3 4 5 6 7
    const int slot = __builtin_amdgcn_readfirstlane(wave == 0 ? 0 : (wave == 4 ? 1 : (wave < 4 ? wave + 1 : wave)));
    const int w0n = T.bins[0] >> 3, w1n = T.bins[1] >> 3;
    const int lw = (slot >= w0n) + (slot >= w0n + w1n);
    const int wrow0 = (slot - (lw == 0 ? 0 : (lw == 1 ? w0n : w0n + w1n))) * 8;      // (wave-uniform)
    const int lrow = wrow0 + (p >> 2);
    // dgrad B fragments of the seven matrices under one scale: (t, part, lane) holds W[ca = lane&31][c = 16*(lane>>5) + 8t + j] * sW
    float invW;
    bool w_bad;
    const float sW = pow2_scale(terms_weights_abs_max<BK_THREADS>(A.W, (uint32_t*)(isel + 2048), w_bad), invW);
    for (int f = threadIdx.x; f < 9 * 2 * 64; f += BK_THREADS) {
        const int sl = f / 128, t = (f >> 6) & 1, l = f & 63;
        const float* Wg = A.W[sl];
        if (!Wg || sl == 2 || sl == 6) continue;
        const int store = sl - (sl > 2) - (sl > 6);
        float w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = Wg[(l & 31) * 32 + 16 * (l >> 5) + 8 * t + j];
        const Split2 sp = split2(w, sW);
        char* base = wfrag + store * TK_WSLOT_BYTES + (t * 2) * 1024 + l * 16;
        *(f16x8*)(base) = sp.hi;
        *(f16x8*)(base + 1024) = sp.lo;
    }
    if (threadIdx.x < 128) {                                   // selection fragments (see bwd_c32_bf16_kernel)
        const int t = threadIdx.x >> 6, l = threadIdx.x & 63, pp = l & 31, hh = l >> 5;
        u32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c0 = 16 * hh + 8 * t + 2 * i;
            v[i] = (pp == c0 ? 0x3C00u : 0u) | (pp == c0 + 1 ? 0x3C000000u : 0u);            // f16 1.0
        }
        *(u32x4*)(isel + t * 1024 + l * 16) = v;
    }
    unsigned present = 0;                                      // bit g: term g of this wave's class has a weight and a dz tensor
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const int sl = lw * 3 + g;
        if (sl != 2 && sl != 6 && A.W[sl] && (g == 0 ? A.x[0] : (g == 1 ? A.x[1] : A.x[2]))) present |= 1u << g;
    }
    const char* wbase[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const int sl = lw * 3 + g;
        wbase[g] = wfrag + (sl - (sl > 2) - (sl > 6)) * TK_WSLOT_BYTES + lane * 16;
    }
    const float* const auxb = lw == 0 ? A.aux[0] : (lw == 1 ? A.aux[1] : A.aux[2]);
    float* const dxb = FIRST ? nullptr : (lw == 0 ? A.out[0] : (lw == 1 ? A.out[1] : A.out[2]));
    const float* const yb = !FIRST ? nullptr : (lw == 0 ? A.y[0] : (lw == 1 ? A.y[1] : A.y[2]));
    float dwf = 0.f;                                           // FIRST: this lane's share of dW_first[level][c = p]
    int e_run = 1 << 20;                                       // running exponent of this wave's dW accumulators (see scn_blk_bwd.inc)
    const int lvl_rows = lw == 0 ? T.lvl_rows[0] : (lw == 1 ? T.lvl_rows[1] : T.lvl_rows[2]);
    f32x16 dWacc[3];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) dWacc[g][r] = 0.f;
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int b, b_end, b_stride;
    block_range(T.n_blocks, b, b_end, b_stride);
    SCN_SLAB_RANGE();
    const int n_it = slab1 - slab0;
    uint32_t cqs[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) cqs[q] = (uint32_t)((n * 8 + h * 4 + q) ^ (n >> 1)) << 4;
    const int r1 = T.lvl_row0[1], r2 = T.lvl_row0[2];
    const size_t sb0 = (size_t)T.lvl_rows[0] * PIECE, sb1 = (size_t)T.lvl_rows[1] * PIECE, sb2 = (size_t)T.lvl_rows[2] * PIECE;
    if (n_it > 0)
    for (; b < b_end; b += b_stride) {
        wait_all_and_barrier();
        const int nsrc = T.blk_rows[b * 4 + 3];
        const int my_rows = auxb ? T.blk_rows[b * 4 + lw] : 0;     // (no forward input: the level was identically zero, nothing to do)
        const int my_w = T.blk_w[b * 4 + lw];
        const int e1 = T.blk_w[b * 4] * T.blk_rows[b * 4], e2 = e1 + T.blk_w[b * 4 + 1] * T.blk_rows[b * 4 + 1];
        const int my_ebase = lw == 0 ? 0 : (lw == 1 ? e1 : e2);
        const int my_row0 = T.blk_row0[b * 3 + lw];
        {
            const int sp0 = T.src_ptr[b];
            const int ep = T.ell_ptr[b];
            const int ell_n = e2 + T.blk_w[b * 4 + 2] * T.blk_rows[b * 4 + 2];
            for (int i = threadIdx.x; i < nsrc; i += BK_THREADS) sm.srcrows[i] = T.src_rows[sp0 + i];
            for (int i = threadIdx.x; i < ell_n; i += BK_THREADS) {
                sm.enc[i] = T.ell_enc[ep + i];
                sm.v[i] = T.ell_v[ep + i];
            }
            if (threadIdx.x < 80) sm.self[threadIdx.x] = T.grp[(size_t)b * 80 + threadIdx.x];
        }
        __syncthreads();
        const uint8_t* mg = grp + slot * 5;
        const int off1 = __builtin_amdgcn_readfirstlane(mg[0]), off2 = __builtin_amdgcn_readfirstlane(mg[1]);   // wave-uniform: SGPRs
        const int cnt0 = (present & 1u) ? __builtin_amdgcn_readfirstlane(mg[2]) : 0, cnt1 = (present & 2u) ? __builtin_amdgcn_readfirstlane(mg[3]) : 0,
                  cnt2 = (present & 4u) ? __builtin_amdgcn_readfirstlane(mg[4]) : 0;
        const int rows_left = my_rows - wrow0;                 // rows of this wave's tile that exist (<= 0: none)
        const bool wave_rows = rows_left > 0;
        const int lrc = lrow < my_rows ? lrow : (my_rows > 0 ? my_rows - 1 : 0);
        const int total = nsrc * CPP;
        // LDS-DMA words as in terms_fwd_c32_kernel -- recomputed from the lane id at every use (registers are what this kernel
        // lacks: nothing of the staging lives across the contraction):
        // slot 2 * (k * 8 + wave) + (lane >> 5) -> cat row -> (level, byte offset inside a slab of that level's tensor)
        auto dma = [&](int k, int slab, char* buf) {
            const int base = (k * BK_WAVES + wave) * 64;
            int ln = threadIdx.x & 63;
            asm volatile("" : "+v"(ln));                       // opaque: keeps the offsets from being hoisted out of the slab loop (and spilled)
            if (base + ln < total) {
                const uint32_t dchunk = (uint32_t)swz32(((wave & 1) << 1) | (ln >> 5), ln & 31) * 16;
                const int r = sm.srcrows[2 * (k * BK_WAVES + wave) + (ln >> 5)];
                const int lv = (r >= r1) + (r >= r2);
                const uint32_t off = (uint32_t)(r - (lv == 0 ? 0 : (lv == 1 ? r1 : r2))) * PIECE + dchunk;
                const uint32_t dst = lds0 + (uint32_t)((buf - smem) + base * 16);
                if (lv == 0 && A.x[0]) lds_dma16((const char*)A.x[0] + slab * sb0, off, dst);
                if (lv == 1 && A.x[1]) lds_dma16((const char*)A.x[1] + slab * sb1, off, dst);
                if (lv == 2 && A.x[2]) lds_dma16((const char*)A.x[2] + slab * sb2, off, dst);
            }
        };
#pragma unroll
        for (int i = 0; i < NDMA; ++i) dma(i, slab0, sm.buf(0));
        f32x4 G[3][4];
        for (int it = 0; it < n_it; ++it) {
            const int slab = slab0 + it;
            const uint32_t bufbit = (uint32_t)((it & 1) << 16);
            const uint32_t cbs[4] = {cqs[0] | bufbit, cqs[1] | bufbit, cqs[2] | bufbit, cqs[3] | bufbit};
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            // (blocks are small: the contraction is too short to cover a staging round trip, so the next slab is requested right
            // after the barrier -- its buffer was last read before it -- instead of inside the MFMA chains.  The forward's L2
            // prefetch does not pay here: +7 % to +20 % at every placement tried -- loads return in order, so a wave's aux reads
            // queue behind it -- and still +7 % when only the waves without rows (and without aux reads) prefetch; moving the
            // aux reads ahead of the staging costs 10 %.)
            if (it + 1 < n_it) {
#pragma unroll
                for (int i = 0; i < NDMA; ++i) dma(i, slab + 1, sm.buf((it + 1) & 1));
            }
            const bool more = false;
            char* nbuf = nullptr;
            if (!wave_rows) continue;                          // no rows: only its share of the staging
            const size_t tuni = (((size_t)slab * lvl_rows + my_row0 + wrow0) * BK_NS) * 32;
            const float* ap = auxb + tuni;
            float* dp = dxb ? dxb + tuni : nullptr;
            const int L0 = p + 4 * 32 * h;
            float a[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool ok = 2 * (r >> 2) + h < rows_left;
                const float v = ap[ok ? L0 + ((r & 3) + 8 * (r >> 2)) * 32 : 0];
                a[r] = ok ? v : 0.f;
            }
            float yl = 0.f;                                    // FIRST: y of point pt(lane & 15, h) (0 where the row does not exist)
            if (FIRST && yb) {
                int ln = threadIdx.x & 63;
                asm volatile("" : "+v"(ln));                   // opaque: the lane part of the address is not hoisted out of the slab loop (and spilled)
                const int pp = ln & 15, hh = ln >> 5;
                const int rl = __builtin_amdgcn_readfirstlane(rows_left);      // (wave-uniform; as a VGPR it is spilled and its reload waits for the staging)
                if (2 * (pp >> 2) + hh < rl)
                    yl = yb[((size_t)slab * lvl_rows + my_row0 + wrow0) * BK_NS + (pp & 3) + 8 * (pp >> 2) + 4 * hh];
            }
            {
                const int rb = my_ebase + lrc * my_w;
                __builtin_amdgcn_s_setprio(3);
                const uint32_t s0 = *(const uint32_t*)(sm.enc + rb), s1 = *(const uint32_t*)(sm.enc + rb + off1),
                               s2 = *(const uint32_t*)(sm.enc + rb + off2);
                const f32x4 v0 = *(const f32x4*)(sm.v + rb), v1 = *(const f32x4*)(sm.v + rb + off1), v2 = *(const f32x4*)(sm.v + rb + off2);
                gather_term_c32<4>(sm, rb, cnt0, cbs, G[0], s0, v0);
                gather_term_c32<4>(sm, rb + off1, cnt1, cbs, G[1], s1, v1);
                gather_term_c32<4>(sm, rb + off2, cnt2, cbs, G[2], s2, v2);
                __builtin_amdgcn_s_setprio(1);
            }
            auto side = [&](int k) {
                if (k < NDMA && more) dma(k, slab + 1, nbuf);
            };
            // scales of the tile (wave-uniform; header of scn_blk_bwd.inc): G under sG = 2^eG from the largest of the tile's gathered
            // values, the aux tile under sigma = 2^(e_run - eG) so that the weight-gradient accumulators stay in the wave's running units
            float sG, inv_gw, sigma;
            {
                float mgv = 0.f;
#pragma unroll
                for (int g = 0; g < 3; ++g)
                    if (present & (1u << g)) mgv = amaxn_4x4(mgv, G[g][0], G[g][1], G[g][2], G[g][3]);     // (NaN counts: scn_blk_fwd.inc)
                uint32_t mgb = max_over_wave(__float_as_uint(mgv));
                if (!w_bad && mgb == 0) {                      // zero-tile early-out (see bwd_c32_bf16_kernel): dx = 0, nothing for the weight gradients
                    if (dp) {
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            if (2 * (r >> 2) + h < rows_left) dp[L0 + ((r & 3) + 8 * (r >> 2)) * 32] = 0.f;
                    }
                    continue;
                }
                if (mgb > 0x7f800000u) {                       // a NaN in the tile (rare): the scale from the NaN-ignoring maximum
                    float mf = 0.f;
#pragma unroll
                    for (int g = 0; g < 3; ++g)
                        if (present & (1u << g)) mf = amax_4x4(mf, G[g][0], G[g][1], G[g][2], G[g][3]);
                    mgb = max_over_wave(__float_as_uint(mf));
                }
                float inv_g;
                sG = pow2_scale(mgb, inv_g);
                inv_gw = inv_g * invW;
                const int eG = pow2_scale_exp(mgb);
                int eA = 14;                                   // tanh: |aux| <= 1
                if (ACT != SCN_ACT_TANH) {
                    float ma = 0.f;
#pragma unroll
                    for (int r = 0; r < 16; r += 2) ma = amax3(ma, a[r], a[r + 1]);
                    eA = pow2_scale_exp(max_over_wave(__float_as_uint(ma)));
                }
                const int u_t = eG + eA;
                if (u_t < e_run) {
                    asm volatile("; dW accumulators into the units of a larger tile (rare)");
                    const float f = exp2i(u_t - e_run);
#pragma unroll
                    for (int g = 0; g < 3; ++g)
#pragma unroll
                        for (int r = 0; r < 16; ++r) dWacc[g][r] *= f;
                    e_run = u_t;
                }
                sigma = exp2i(e_run - eG);
            }
            f32x16 acc = zero16;
            Split2 At[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float x8[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) x8[j] = a[8 * t + j];
                At[t] = split2(x8, sigma);
            }
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                if (!(present & (1u << g))) {                  // absent term: its LDS-DMA side slots still have to be issued
                    side(g * 4); side(g * 4 + 1); side(g * 4 + 2); side(g * 4 + 3);
                    continue;
                }
                f32x16 Th, Tl;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    float x8[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) x8[j] = G[g][2 * t + (j >> 2)][j & 3];
                    const Split2 zs = split2(x8, sG);
                    const char* wb = wbase[g] + (t * 2) * 1024;
                    const f16x8 wh = *(const f16x8*)(wb), wl = *(const f16x8*)(wb + 1024);
                    const f16x8 It = *(const f16x8*)(isel + t * 1024 + lane * 16);
                    const int k0 = (g * 2 + t) * 2;                          // two LDS-DMA side slots per group (8 used by g = 0, 1)
                    Tl = __builtin_amdgcn_mfma_f32_32x32x16_f16(zs.lo, It, t == 0 ? zero16 : Tl, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(zs.lo, wh, acc, 0, 0, 0);
                    side(k0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(zs.hi, wl, acc, 0, 0, 0);
                    side(k0 + 1);
                    Th = __builtin_amdgcn_mfma_f32_32x32x16_f16(zs.hi, It, t == 0 ? zero16 : Th, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(zs.hi, wh, acc, 0, 0, 0);
                }
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    f16x8 bh, bl;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {                        // (exact: the parts are f16 values)
                        const auto ph = __builtin_amdgcn_cvt_pkrtz(Th[8 * t + 2 * i], Th[8 * t + 2 * i + 1]);
                        const auto pl = __builtin_amdgcn_cvt_pkrtz(Tl[8 * t + 2 * i], Tl[8 * t + 2 * i + 1]);
                        bh[2 * i] = (_Float16)ph[0]; bh[2 * i + 1] = (_Float16)ph[1];
                        bl[2 * i] = (_Float16)pl[0]; bl[2 * i + 1] = (_Float16)pl[1];
                    }
                    const Split2& at = At[t];
                    dWacc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(at.lo, bh, dWacc[g], 0, 0, 0);
                    dWacc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(at.hi, bl, dWacc[g], 0, 0, 0);
                    dWacc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(at.hi, bh, dWacc[g], 0, 0, 0);
                }
            }
            __builtin_amdgcn_s_setprio(0);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] *= inv_gw;             // out of the tile's units: acc = sum_g G_g W_g^T
            if (FIRST) terms_first_tile<ACT>(std::make_integer_sequence<int, 16>{}, yl, acc, a, dwf);
            if (dp) {                                          // dX = acc * act'(aux)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (2 * (r >> 2) + h < rows_left)
                        dp[L0 + ((r & 3) + 8 * (r >> 2)) * 32] = acc[r] * act_grad_from_output(ACT, a[r]);   // (non-temporal: +11 % here)
            }
        }
    }
    // this wave's three 32 x 32 weight-gradient tiles: [ca][term * 32 + c] (the per-class sum over waves happens in the reduce)
    float* outp = partial + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * BK_WAVES + slot) * 3072;   // (indexed by row-group slot)
    const int k_un = e_run >= (1 << 20) ? 0 : -e_run;          // out of the wave's running units (see bwd_c32_bf16_kernel)
    const int k_1 = k_un < -126 ? -126 : (k_un > 127 ? 127 : k_un);
    const float un1 = exp2i(k_1), un2 = exp2i(k_un - k_1);
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ca = (r & 3) + 8 * (r >> 2) + 4 * h;
            outp[ca * 96 + g * 32 + p] = dWacc[g][r] * un1 * un2;
        }
    if (FIRST) A.partial_first[((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * BK_WAVES + slot) * 64 + lane] = dwf;
}

// dW_first[class][c] += sum over workgroups, the waves of that class and the two half waves (fixed order)
__global__ void terms_dwf_reduce_kernel(const float* __restrict__ pf, int n_wg, int w0n, int w1n, float* d0, float* d1, float* d2) {
    const int cls = blockIdx.x, c = threadIdx.x;               // 3 x 32
    const int wlo = cls == 0 ? 0 : (cls == 1 ? w0n : w0n + w1n), whi = cls == 0 ? w0n : (cls == 1 ? w0n + w1n : BK_WAVES);
    float s = 0.f;
    for (int g = 0; g < n_wg; ++g)
        for (int w = wlo; w < whi; ++w) {
            const float* q = pf + ((size_t)g * BK_WAVES + w) * 64;
            s += q[c] + q[32 + c];
        }
    float* d = cls == 0 ? d0 : (cls == 1 ? d1 : d2);
    if (d) d[c] += s;
}

// dW[class][term][ca][c] += sum over workgroups and the waves of that class (fixed order)
struct TermsDW { float* p[9]; };                    // [class][term] weight-gradient matrices, by value (nullptr = absent)
__global__ void terms_dw_reduce_kernel(const float* __restrict__ partial, int n_wg, int w0n, int w1n, TermsDW D) {
    const int cls = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;       // ca * 96 + term * 32 + c
    if (i >= 3072) return;
    const int wlo = cls == 0 ? 0 : (cls == 1 ? w0n : w0n + w1n), whi = cls == 0 ? w0n : (cls == 1 ? w0n + w1n : BK_WAVES);
    float s = 0.f;
    for (int g = 0; g < n_wg; ++g)
        for (int w = wlo; w < whi; ++w) s += partial[((size_t)g * BK_WAVES + w) * 3072 + i];
    const int ca = i / 96, rem = i - ca * 96, term = rem >> 5, cc = rem & 31;
    float* d = D.p[0];                                 // (selected without indexing the by-value array dynamically: no scratch copy)
#pragma unroll
    for (int q = 1; q < 9; ++q)
        if (cls * 3 + term == q) d = D.p[q];
    if (d) d[ca * 32 + cc] += s;
}

static size_t terms_bwd_lds() { return (size_t)TK_LDS_BYTES; }

// The forms of terms_bwd_c32_kernel by name:
template <int ACT> constexpr auto terms_bwd_c32_plain = terms_bwd_c32_kernel<ACT, false>;      // A.out = the input gradients, A.y null
template <int ACT> constexpr auto terms_bwd_c32_first = terms_bwd_c32_kernel<ACT, true>;       // A.out null: contracted with A.y into A.partial_first

size_t terms_backward_workspace(const scn_conv_s* c, int) {         // (any slab count: the grid covers the blocks)
    const dim3 grid = terms_grid(c);
    return (size_t)grid.x * grid.y * BK_WAVES * (3072 + 64) * sizeof(float);
}

// y / dW_first non-null: the FIRST variant (dx must then be all null: it is contracted with y instead of being written)
int terms_backward(scn_conv_s* c, int n_slabs, const float* const* dz, const float* const* W, const float* const* aux, int act,
                   float* const* dx, float* const* dW, const float* const* y, float* const* dW_first, void* ws, hipStream_t st) {
    if (c->terms.group_rows != 8) return SCN_ERR_UNSUPPORTED;     // a plan cut for the forward's 4-row waves
    const bool first = y != nullptr;
    const TermsDev T = terms_dev(c);
    TermsPtrs A;
    for (int i = 0; i < 3; ++i) { A.x[i] = dz[i]; A.aux[i] = aux[i]; A.out[i] = first ? nullptr : dx[i]; A.y[i] = first ? y[i] : nullptr; }
    for (int i = 0; i < 9; ++i) A.W[i] = W[i];
    const dim3 grid = terms_grid(c);
    const int n_wg = (int)(grid.x * grid.y);
    float* partial = (float*)ws;
    A.partial_first = partial + (size_t)n_wg * BK_WAVES * 3072;
    TermsDW D;
    for (int i = 0; i < 9; ++i) D.p[i] = dW[i];
    const int st_k = with_act(act, [&](auto ACT) -> int {
        constexpr int AV = decltype(ACT)::value;
        return launch_checked(first ? terms_bwd_c32_first<AV> : terms_bwd_c32_plain<AV>, grid, dim3(BK_THREADS), terms_bwd_lds(), st, T, A,
                              partial, n_slabs);
    });
    if (st_k != SCN_OK) return st_k;
    hipLaunchKernelGGL(terms_dw_reduce_kernel, dim3(12, 3), dim3(256), 0, st, partial, n_wg, T.bins[0] >> 3, T.bins[1] >> 3, D);
    SCN_LAUNCH_CHECK();
    if (first) {
        hipLaunchKernelGGL(terms_dwf_reduce_kernel, dim3(3), dim3(32), 0, st, (const float*)A.partial_first, n_wg, T.bins[0] >> 3,
                           T.bins[1] >> 3, dW_first[0], dW_first[1], dW_first[2]);
        SCN_LAUNCH_CHECK();
    }
    return SCN_OK;
}
