// The step epilogue (scn_step_epilogue) -- part of scn_blocked.hip (one translation unit; included inside namespace scn).
// A micro-batch of the cone route ends with small launches nobody waits for before the micro-batch is over: the loss sum, the
// readout's weight gradient, the dW reduce of every backward, the clear of the readout gradient's rows and the masked clears of the
// pooled gradient buffers.  Each waited for a 0.1-0.2 ms backward to drain before it could start.  Here they are ONE launch: a
// workgroup finds its job by its index (scn_step_ranges.h) and runs the body of that job's own kernel -- the same threads per
// workgroup (the launch has 1024; a job of 64 or 256 lets the other waves go at once), the same summation order, so every result has
// the stand-alone launch's bits.  No workgroup reads what another one of the launch writes: each gradient element, loss[0] and each
// cleared item belongs to exactly one job.

struct EpiArgs {
    EpiRanges r;
    scn_step_epilogue_desc d;
    PlanDev P;                  // the masked clears' plan
    int32_t n_rows;
};

__global__ __launch_bounds__(1024) void step_epilogue_kernel(EpiArgs a) {
    int32_t rel = 0;
    const int job = epi_job_of(a.r, (int32_t)blockIdx.x, &rel);          // (workgroup-uniform)
    const int tid = threadIdx.x;
    const scn_step_epilogue_desc& d = a.d;
    if (job == EPI_JOB_LOSS) {
        masked_ce_body<false>(tid, d.loss_n, d.logp, d.y, d.scale, nullptr, d.loss, d.overwrite);
    } else if (job == EPI_JOB_READOUT_DW) {
        readout_dw_body(tid, d.rd_nd, d.rd_c, d.rd_dl, d.rd_bh, d.rd_d_w);
    } else if (job >= EPI_JOB_REDUCE && job < EPI_JOB_FIRST) {
        const scn_epi_reduce& q = d.reduce[job - EPI_JOB_REDUCE];
        blocked_dw_reduce_body(rel, q.partial, q.n_wg, q.c_aux, q.c_dz, q.dW[0], q.dW[1], q.dW[2]);
    } else if (job == EPI_JOB_FIRST) {
        if (tid >= 64) return;
        if (d.first_form == EPI_FIRST_C32)
            dw_first_reduce_body(rel, tid, d.first_partial, d.first_n_wg, 32, d.first_dW[0], d.first_dW[1], d.first_dW[2]);
        else
            dw_first_reduce_pair_body(rel, tid, d.first_partial, d.first_n_wg, d.first_dW[0], d.first_dW[1], d.first_dW[2]);
    } else if (job == EPI_JOB_READOUT_CLEAR) {
        if (tid >= 64) return;                                            // (a finished wave no longer takes part in the body's barriers)
        readout_bwd_body(rel, tid, d.rc_ns, d.rc_n_edges, d.rc_c, nullptr, nullptr, d.rc_nbr, d.rc_max_deg, d.rc_last_nodes, d.rc_inc_ptr,
                         d.rc_inc_edge, nullptr, d.rc_edge_nodes, nullptr, nullptr, 0, d.rc_dz, nullptr, 1);
    } else if (job >= EPI_JOB_CLEAR && job < EPI_JOBS) {
        if (tid >= 256) return;
        const int k = job - EPI_JOB_CLEAR;
        const scn_epi_clear& q = d.clear[k];
        const int32_t grid = a.r.end[job] - a.r.end[job - 1];
        clear_mask_body(rel, grid, a.P, KeepMask{q.mask, (q.n_slabs + 31) / 32}, q.tensor, a.n_rows, q.n_slabs, q.ns * q.channels);
    }
}

// the two reduces as launches of their own (scn_dw_reduce, scn_dw_first_reduce): what a backward runs behind its kernel
int blocked_dw_reduce_alone(const float* partial, int n_wg, int c_aux, int cd, float* const* dW, hipStream_t st) {
    return reduce_dw(partial, n_wg, c_aux, cd, dW, st);
}
int blocked_dw_first_reduce_alone(const float* partial, int n_wg, int form, float* const* dW, hipStream_t st) {
    if (form == EPI_FIRST_C32) return launch_checked(dw_first_reduce_kernel, dim3(96), dim3(64), 0, st, partial, n_wg, 32, dW[0], dW[1], dW[2]);
    return launch_checked(dw_first_reduce_pair_kernel, dim3(48), dim3(64), 0, st, partial, n_wg, dW[0], dW[1], dW[2]);
}

int blocked_step_epilogue(scn_conv_s* c, const scn_step_epilogue_desc& d, hipStream_t st) {
    int64_t counts[EPI_JOBS] = {0};
    if (d.n_reduce < 0 || d.n_reduce > EPI_MAX_REDUCES || d.n_clear < 0 || d.n_clear > EPI_MAX_CLEARS) return SCN_ERR_BAD_SHAPE;
    if (d.loss) {
        if (!d.logp || !d.y) return SCN_ERR_BAD_ARG;
        if (d.loss_n <= 0) return SCN_ERR_BAD_SHAPE;
        counts[EPI_JOB_LOSS] = 1;
    }
    if (d.rd_d_w) {
        if (!d.rd_dl || !d.rd_bh) return SCN_ERR_BAD_ARG;
        if (d.rd_nd <= 0 || d.rd_c <= 0) return SCN_ERR_BAD_SHAPE;
        counts[EPI_JOB_READOUT_DW] = 1;
    }
    for (int k = 0; k < d.n_reduce; ++k) {
        const scn_epi_reduce& q = d.reduce[k];
        if (!q.partial) return SCN_ERR_BAD_ARG;
        if (q.n_wg <= 0 || q.c_aux <= 0 || q.c_dz <= 0) return SCN_ERR_BAD_SHAPE;
        counts[EPI_JOB_REDUCE + k] = epi_reduce_blocks(q.c_aux, q.c_dz);
    }
    if (d.first_form != EPI_FIRST_NONE) {
        if (d.first_form != EPI_FIRST_C32 && d.first_form != EPI_FIRST_PAIR) return SCN_ERR_BAD_SHAPE;
        if (!d.first_partial || !d.first_dW[0] || !d.first_dW[1] || !d.first_dW[2]) return SCN_ERR_BAD_ARG;
        if (d.first_n_wg <= 0) return SCN_ERR_BAD_SHAPE;
        counts[EPI_JOB_FIRST] = epi_first_blocks(d.first_form);
    }
    if (d.rc_dz) {
        if (!d.rc_nbr || !d.rc_last_nodes || !d.rc_inc_ptr || !d.rc_inc_edge || !d.rc_edge_nodes) return SCN_ERR_BAD_ARG;
        if (d.rc_n_slabs <= 0 || d.rc_ns <= 0 || d.rc_n_edges <= 0 || d.rc_c <= 0 || d.rc_max_deg <= 0) return SCN_ERR_BAD_SHAPE;
        if (d.rc_max_deg > RO_MAXD) return SCN_ERR_UNSUPPORTED;
        counts[EPI_JOB_READOUT_CLEAR] = (int64_t)d.rc_n_slabs * d.rc_ns;
    }
    for (int k = 0; k < d.n_clear; ++k) {
        const scn_epi_clear& q = d.clear[k];
        if (!c || !q.tensor || !q.mask) return SCN_ERR_BAD_ARG;
        if (q.n_slabs <= 0 || q.ns <= 0 || q.channels <= 0) return SCN_ERR_BAD_SHAPE;
        if (!c->plan.built || q.ns != BK_NS || (q.ns * q.channels) % 4 || (reinterpret_cast<uintptr_t>(q.tensor) & 15)) return SCN_ERR_UNSUPPORTED;
        counts[EPI_JOB_CLEAR + k] = epi_clear_blocks(c->plan.dev.n_blocks);
    }
    EpiArgs a{};
    if (!epi_ranges(counts, &a.r)) return SCN_ERR_UNSUPPORTED;
    if (epi_total(a.r) == 0) return SCN_OK;
    a.d = d;
    if (d.n_clear) {
        a.P = c->plan.dev;
        a.n_rows = c->n_rows;
    }
    return launch_checked(step_epilogue_kernel, dim3((unsigned)epi_total(a.r)), dim3(1024), 0, st, a);
}
