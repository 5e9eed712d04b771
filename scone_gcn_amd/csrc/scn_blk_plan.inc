// host side: the block plan of an operator -- part of scn_blocked.hip (one translation unit; included inside namespace scn)
// ------------------------------------------------------------------------------------------------
// plan
// ------------------------------------------------------------------------------------------------
void free_block_plan(scn_conv_s* c) {
    for (void* p : c->plan.allocs)
        if (p) (void)hipFree(p);
    c->plan.allocs.clear();
    c->small_pack = nullptr;
    c->small_ell = nullptr;
    c->plan.built = false;
}

template <typename T>
static int upload(scn_conv_s* c, const std::vector<T>& h, const T** out) {
    void* d = nullptr;
    size_t bytes = std::max<size_t>(h.size(), 1) * sizeof(T);
    SCN_HIP_TRY(hipMalloc(&d, bytes));
    c->plan.allocs.push_back(d);
    if (!h.empty()) SCN_HIP_TRY(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = (const T*)d;
    return SCN_OK;
}

int build_assignments(scn_conv_s* c);

// Greedy block cut shared by the plan builder and scn_plan_refine_order: starting at row r0, take consecutive rows (< r_end)
// while the block stays within BK_R rows, BK_SRC distinct source rows (the rows themselves included when the operator has
// an identity slot) and BK_ELL_CAP padded ELL entries.  `mark` is a per-column stamp array (block id), `cur` gets the sources.
static void grow_block(const int32_t* rowptr, const int32_t* col, int r_end, bool has_id, int r0, int bid,
                       std::vector<int32_t>& mark, std::vector<int32_t>& cur, int& rows, int& w) {
    cur.clear();
    rows = 0;
    w = 0;
    while (r0 + rows < r_end && rows < BK_R) {
        const int r = r0 + rows;
        const int j0 = rowptr[r], j1 = rowptr[r + 1];
        int add = 0;
        for (int j = j0; j < j1; ++j)
            if (mark[col[j]] != bid) ++add;
        bool self_new = has_id && mark[r] != bid;
        for (int j = j0; j < j1 && self_new; ++j)
            if (col[j] == r) self_new = false;
        if (self_new) ++add;
        const int nw = std::max(w, (j1 - j0 + 1) & ~1);          // padded width, even
        if ((int)cur.size() + add > BK_SRC || nw * (rows + 1) > BK_ELL_CAP || nw > 254) break;
        for (int j = j0; j < j1; ++j)
            if (mark[col[j]] != bid) { mark[col[j]] = bid; cur.push_back(col[j]); }
        if (has_id && mark[r] != bid) { mark[r] = bid; cur.push_back(r); }
        w = nw;
        ++rows;
    }
}

// the block's CSR slice in local source indices (local[col] = rank of the column among the block's sorted sources)
static void layout_input(BlockLayout& L, const int32_t* rowptr, const int32_t* col, const float* val1, bool has_id, int r0,
                         int rows, int w, int nsrc, const std::vector<int32_t>& local) {
    L.rows = rows;
    L.nsrc = nsrc;
    L.w = w;
    L.ptr.assign(1, 0);
    L.src.clear();
    L.up.clear();
    L.self.assign(rows, -1);
    for (int i = 0; i < rows; ++i) {
        const int r = r0 + i;
        for (int j = rowptr[r]; j < rowptr[r + 1]; ++j) {
            L.src.push_back(local[col[j]]);
            L.up.push_back(val1 && val1[j] != 0.f);
        }
        L.ptr.push_back((int)L.src.size());
        if (has_id) L.self[i] = local[r];
    }
}

int build_block_plan(scn_conv_s* c) {
    // only the scone/ebli shape gets a plan; everything else runs the generic kernels
    // single-group operators get a plan: identity + 2 value arrays is the scone/ebli layer (MFMA kernels); one value
    // array without identity is a bare shift (Bunch terms) served by the blocked SpMM
    if (c->n_groups != 1) return SCN_OK;
    const Group& G = c->g[0];
    if (G.n_vals < 1) return SCN_OK;
    // the kernels address a staged source row as a 32-bit byte offset inside one slab (row * piece, piece <= 512 B): an operator
    // with more source rows than that gets no plan and runs on the generic kernels (64-bit addressing)
    if ((int64_t)G.n_cols * 512 >= (int64_t)1 << 32 || (int64_t)c->n_rows * 512 >= (int64_t)1 << 32) return SCN_OK;
    const bool has_v1 = G.n_vals > 1, has_id = G.identity == 1;
    const int n_rows = c->n_rows;
    std::vector<int32_t> blk_row0, src_ptr(1, 0), src_rows, ell_ptr;
    std::vector<uint8_t> blk_rows, width, tile_w, tile_w4, tile_wu, tile_wu4, ell_slot, self_slot;
    std::vector<float2> ell_v;
    std::vector<float> block_gather;                              // per block: sum over the 8-row groups of their ELL width
    std::vector<int32_t> mark(G.n_cols, -1), local(G.n_cols, 0), cur;
    cur.reserve(BK_SRC + 64);
    int64_t total_src = 0;
    int wmax = 0;
    int bid = 0;
    const uint8_t* hint = c->block_start.empty() ? nullptr : c->block_start.data();
#ifdef SCN_AB_LEGACY_LAYOUT                                   // diagnostic builds: slots in row order, entries in CSR order
    const bool optimise_layout = false;
#else
    const bool optimise_layout = true;
#endif
    BlockLayout L;
    int64_t sim_positions = 0, sim_cycles = 0;
    for (int r0 = 0; r0 < n_rows;) {
        int rows = 0, w = 0, r_limit = n_rows;
        if (hint)                                               // a hinted boundary closes the block (limits still apply)
            for (int r = r0 + 1; r < std::min(n_rows, r0 + BK_R + 1); ++r)
                if (hint[r]) { r_limit = r; break; }
        grow_block(G.h_rowptr.data(), G.h_col.data(), r_limit, has_id, r0, bid, mark, cur, rows, w);
        if (rows == 0) return SCN_OK;   // a single row does not fit: no plan (generic kernels will be used)
        std::sort(cur.begin(), cur.end());
        for (size_t i = 0; i < cur.size(); ++i) local[cur[i]] = (int32_t)i;
        // slot numbers of the sources and the order of every row's entries: scn_blk_layout.inc (LDS bank classes)
        layout_input(L, G.h_rowptr.data(), G.h_col.data(), has_v1 ? G.h_val1.data() : nullptr, has_id, r0, rows, w,
                     (int)cur.size(), local);
        layout_block(L, optimise_layout);
        sim_positions += L.positions;
        sim_cycles += L.cycles;
        blk_row0.push_back(r0);
        blk_rows.push_back((uint8_t)rows);
        {
            const size_t sb = src_rows.size();
            src_rows.resize(sb + cur.size());
            for (size_t i = 0; i < cur.size(); ++i) src_rows[sb + L.slot_of[i]] = cur[i];
        }
        src_ptr.push_back((int32_t)src_rows.size());
        ell_ptr.push_back((int32_t)ell_slot.size());
        width.push_back((uint8_t)w);
        wmax = std::max(wmax, w);
        const size_t base = ell_slot.size();                 // entries are [row][w], w even, zero padded
        ell_slot.resize(base + (size_t)w * rows, 0);
        ell_v.resize(base + (size_t)w * rows, float2{0.f, 0.f});
        uint8_t tw[BK_WAVES], twu[BK_WAVES];
        for (int i = 0; i < BK_WAVES; ++i) {                  // a wave of the 8-row kernels walks both of its quads
            tw[i] = std::max(L.tw4[2 * i], L.tw4[2 * i + 1]);
            twu[i] = std::max(L.twu4[2 * i], L.twu4[2 * i + 1]);
        }
        for (int i = 0; i < BK_R; ++i) {
            uint8_t ss = 0;
            if (i < rows) {
                const int j0 = G.h_rowptr[r0 + i];
                for (int t = 0; t < w; ++t) {
                    const size_t e = base + (size_t)i * w + t;
                    const int k = L.order[(size_t)i * w + t];
                    if (k >= 0) {                            // k indexes the block's CSR slice: row i starts at L.ptr[i]
                        const int j = j0 + (k - L.ptr[i]);
                        ell_slot[e] = L.slot_of[L.src[k]];
                        ell_v[e] = float2{G.h_val0[j], has_v1 ? G.h_val1[j] : 0.f};
                    } else {
                        ell_slot[e] = L.pad_slot[(size_t)i * w + t];
                    }
                }
                ss = has_id ? L.slot_of[local[r0 + i]] : 0;
            }
            self_slot.push_back(ss);
        }
        tile_w.insert(tile_w.end(), tw, tw + BK_WAVES);
        tile_w4.insert(tile_w4.end(), L.tw4, L.tw4 + 2 * BK_WAVES);
        {
            float gather = 0.f;
            for (int i = 0; i < BK_WAVES; ++i) gather += tw[i];
            block_gather.push_back(gather);
        }
        tile_wu.insert(tile_wu.end(), twu, twu + BK_WAVES);
        tile_wu4.insert(tile_wu4.end(), L.twu4, L.twu4 + 2 * BK_WAVES);
        total_src += (int64_t)cur.size();
        r0 += rows;
        ++bid;
    }
    BlockPlan& P = c->plan;
    P.dev.n_blocks = bid;
    P.dev.ell_w_max = wmax;
    int st;
    if ((st = upload(c, blk_row0, &P.dev.blk_row0)) != SCN_OK) return st;
    if ((st = upload(c, blk_rows, &P.dev.blk_rows)) != SCN_OK) return st;
    if ((st = upload(c, src_ptr, &P.dev.src_ptr)) != SCN_OK) return st;
    if ((st = upload(c, src_rows, &P.dev.src_rows)) != SCN_OK) return st;
    if ((st = upload(c, ell_ptr, &P.dev.ell_ptr)) != SCN_OK) return st;
    if ((st = upload(c, width, &P.dev.width)) != SCN_OK) return st;
    if ((st = upload(c, tile_w, &P.dev.tile_w)) != SCN_OK) return st;
    if ((st = upload(c, tile_w4, &P.dev.tile_w4)) != SCN_OK) return st;
    if ((st = upload(c, tile_wu, &P.dev.tile_wu)) != SCN_OK) return st;
    if ((st = upload(c, tile_wu4, &P.dev.tile_wu4)) != SCN_OK) return st;
    if ((st = upload(c, ell_slot, &P.dev.ell_slot)) != SCN_OK) return st;
    std::vector<uint16_t> ell_enc(ell_slot.size());
    for (size_t i = 0; i < ell_slot.size(); ++i) ell_enc[i] = (uint16_t)((ell_slot[i] << 9) | ((ell_slot[i] & 3) << 5));   // slot*512 | slot part of swz32
    if ((st = upload(c, ell_enc, &P.dev.ell_enc)) != SCN_OK) return st;
    if ((st = upload(c, ell_v, &P.dev.ell_v)) != SCN_OK) return st;
    if ((st = upload(c, self_slot, &P.dev.self_slot)) != SCN_OK) return st;
    {   // the packed records of the visiting backwards' unit top, from the arrays above (which stay: every other kernel reads them)
        std::vector<BlockRec> rec(bid);
        if (!pack_block_records(bid, blk_row0.data(), blk_rows.data(), src_ptr.data(), ell_ptr.data(), width.data(), tile_w.data(), tile_wu.data(),
                                rec.data()))
            return SCN_ERR_INTERNAL;
        if ((st = upload(c, rec, &P.blk_rec)) != SCN_OK) return st;   // (hipMalloc: 256-byte aligned)
    }
    P.mean_src_per_row = (double)total_src / std::max(1, n_rows);
    P.gather_positions = sim_positions;
    P.gather_cycles = sim_cycles;
    {   // one slab of a block costs a constant part (MFMA, epilogue, barriers: ~60 % on average, tools/stamps.py) + its gather
        double mean = 0.0;
        for (float g : block_gather) mean += g;
        mean /= std::max<size_t>(1, block_gather.size());
        P.h_cost.resize(block_gather.size());
        for (size_t i = 0; i < block_gather.size(); ++i) P.h_cost[i] = (float)(1.5 * mean + block_gather[i]);
    }
    P.h_row0 = blk_row0;
    P.h_row0.push_back(n_rows);
    P.built = true;
    return build_assignments(c);
}
