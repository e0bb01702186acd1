// api_timing.cpp -- femshell_time_kernel, the measurement hook of bench.py, and the byte models of the kernels it times.
#include "api_internal.hpp"
#include "modal.hpp"

#include <algorithm>
#include <cstdlib>

using namespace femshell;

namespace femshell {

double bytes_assemble(const femshell_ctx *c)
{
    const Plan &p = c->plan;
    // (symmetric storage: only the stored blocks are computed and written -- the algorithmic bytes of that layout -- and of a
    //  diagonal block, symmetric itself, the 12 words of the upper triangle: 192 instead of 288 bytes per node)
    return 12.0 * p.n_ltri() + 16.0 * p.n_lquad() + 24.0 * (p.n_own + p.n_ghost) + 292.0 * (double)p.stored_blocks -
           (c->dm.diag_upper ? 96.0 * p.n_own : 0.0) + 4.0 * (p.n_own + 1) + 48.0 * p.n_own +
           // sections: an index per element and every row of the table that is in use, once
           (c->have_sections ? 4.0 * (p.n_ltri() + p.n_lquad()) + (double)sizeof(SecConst) * std::min<double>(c->n_sections, p.n_ltri() + p.n_lquad()) : 0.0);
}
double bytes_spmv(const femshell_ctx *c)
{
    const Plan &p = c->plan;
    // (symmetric storage: every stored block is streamed once; the 48-byte transposed products written and read
    // beside them are overhead of the method, not algorithmic traffic)
    // ... and of a diagonal block the 12 words (192 bytes) that hold its upper triangle
    return 292.0 * (double)p.stored_blocks - (p.symmetric ? 96.0 * p.n_own : 0.0) + 4.0 * (p.n_own + 1) + 96.0 * p.n_own;
}
// (the inverse diagonal blocks are symmetric: 21 of their 36 words are stored and read)
double bytes_update(const femshell_ctx *c) { return (7.0 * 48.0 + 168.0) * c->plan.n_own; }
double bytes_direction(const femshell_ctx *c) { return 3.0 * 48.0 * c->plan.n_own; }
// single-reduction recurrence: z, w, p, s, x, r read, p, s, x, r, z written, Minv read
double bytes_update_single_reduction(const femshell_ctx *c) { return (11.0 * 48.0 + 168.0) * c->plan.n_own; }

} // namespace femshell

extern "C" {

int femshell_time_kernel(femshell_ctx *c, femshell_kernel which, int32_t reps, double *mean_ms_out, double *bytes_out)
{
    if (!c || !mean_ms_out) return set_err(FEMSHELL_ERR_INVALID, "femshell_time_kernel: null argument");
    if (const int prc = finish_pending_assembly(c)) return prc;
    if (!c->have_mesh || reps <= 0) return set_err(FEMSHELL_ERR_INVALID, "femshell_time_kernel: no mesh or reps <= 0");
    int rc = select_device(c);
    if (rc) return rc;
    if (which >= FEMSHELL_KERNEL_LUMPED_MASS && which <= FEMSHELL_KERNEL_NEWMARK_UPDATE) {
        // the kernels of the dynamics, back to back between one event pair (they stream vectors only; k_lumped_mass and
        // k_mass_shift run once per mesh and per dt)
        if (!c->have_density) return set_err(FEMSHELL_ERR_INVALID, "femshell_time_kernel: no density set");
        if (which != FEMSHELL_KERNEL_LUMPED_MASS && !c->dyn.active) return set_err(FEMSHELL_ERR_INVALID, "femshell_time_kernel: dynamics is not active");
        rc = ensure(c, kMass);
        if (rc) return rc;
        hipStream_t st = c->stream;
        femshell_ctx::Dynamics &d = c->dyn;
        const Plan &p = c->plan;
        const double t = c->cfg.thickness;
        FS_HIP(hipStreamSynchronize(st));
        FS_HIP(hipEventRecord(c->ev0, st));
        for (int32_t i = 0; i < reps; i++) {
            if (which == FEMSHELL_KERNEL_LUMPED_MASS)
                launch_lumped_mass(c->dm, make_double2(c->rho * t, c->rho * t * t * t / 12.0), c->have_sections ? c->sec_mass.p : nullptr,
                                   c->ds.slice_elem_section, c->mass.p, st);
            else if (which == FEMSHELL_KERNEL_MASS_SHIFT) launch_mass_shift(c->dm, c->mass.p, d.k.shift, st);
            else if (which == FEMSHELL_KERNEL_NEWMARK_RHS) launch_newmark_rhs(c->dm, d.k, c->mass.p, c->F.p, d.u[d.cur].p, d.v[d.cur].p, d.a[d.cur].p, d.b.p, st);
            else launch_newmark_update(c->dm, d.k, c->x.p, d.u[d.cur].p, d.v[d.cur].p, d.a[d.cur].p, d.u[d.cur ^ 1].p, d.v[d.cur ^ 1].p, d.a[d.cur ^ 1].p, st);
        }
        FS_HIP(hipEventRecord(c->ev1, st));
        FS_HIP(hipStreamSynchronize(st));
        FS_HIP(hipGetLastError());
        float ms = 0.f;
        FS_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        *mean_ms_out = (double)ms / reps;
        if (which == FEMSHELL_KERNEL_MASS_SHIFT) invalidate(c, Change::matrix_spoiled); // (the shift was added `reps` times)
        if (which == FEMSHELL_KERNEL_NEWMARK_UPDATE) d.have_candidate = false;
        if (bytes_out) {
            const double n = p.n_own, ne = p.n_ltri() + p.n_lquad();
            // mass: node ids of the slices' element lists (16 B per entry, about six entries per element on a structured mesh:
            // counted as listed), coordinates once per node, 48 B written; shift: 48 B of M, the six diagonal words read and
            // written, the mask; right-hand side: M, F, u, v, a read, b written; update: x, u, v, a read, u', v', a' written
            *bytes_out = which == FEMSHELL_KERNEL_LUMPED_MASS ? 16.0 * (double)p.slice_elem_nodes.size() / 4.0 + 24.0 * n + 48.0 * n + (c->have_sections ? 4.0 * ne : 0.0)
                         : which == FEMSHELL_KERNEL_MASS_SHIFT ? (48.0 + 96.0 + 1.0) * n
                         : which == FEMSHELL_KERNEL_NEWMARK_RHS ? (6.0 * 48.0 + 1.0) * n
                                                                : (7.0 * 48.0 + 1.0) * n;
        }
        return FEMSHELL_OK;
    }
    if (which >= FEMSHELL_KERNEL_SPMM && which <= FEMSHELL_KERNEL_BLOCK_COMBINE) {
        // the block kernels of the modal analysis on scratch blocks of hashed vectors, back to back between one event pair
        if (c->cfg.world_size != 1) return set_err(FEMSHELL_ERR_UNSUPPORTED, "femshell_time_kernel: the block kernels run on single-rank contexts");
        if (which == FEMSHELL_KERNEL_GRAM && !c->have_density) return set_err(FEMSHELL_ERR_INVALID, "femshell_time_kernel: no density set");
        const int nc = (int)knob_long("FEMSHELL_TIME_KERNEL_COLS", 4);
        if (nc < 1 || nc > kModalMaxBlock) return set_err(FEMSHELL_ERR_INVALID, "femshell_time_kernel: FEMSHELL_TIME_KERNEL_COLS must be in 1 .. 32");
        if (which == FEMSHELL_KERNEL_GRAM && (rc = ensure(c, kMass))) return rc;
        if (which == FEMSHELL_KERNEL_SPMM && (rc = ensure(c, kK))) return rc;
        hipStream_t st = c->stream;
        const Plan &p = c->plan;
        const int64_t ld = (int64_t)p.n_local_nodes() * 6;
        const int q = 3 * nc, n_out = 2 * nc;
        DevBuf<double> S, Y, tb, partials, G, coef;
        FS_HIP(S.alloc((size_t)q * (size_t)ld));
        FS_HIP(S.zero(st));
        launch_modal_init(c->dm, nullptr, which == FEMSHELL_KERNEL_SPMM ? nc : q, S.p, ld, st);
        if (which == FEMSHELL_KERNEL_SPMM) {
            FS_HIP(Y.alloc((size_t)nc * (size_t)ld));
            if (c->dm.symmetric) FS_HIP(tb.alloc((size_t)kSpmmMaxCols * (size_t)p.total_slots() * 6));
        } else if (which == FEMSHELL_KERNEL_GRAM) {
            FS_HIP(partials.alloc((size_t)kGramGrid * q * q));
            FS_HIP(G.alloc((size_t)q * q));
        } else {
            FS_HIP(Y.alloc((size_t)n_out * (size_t)ld));
            const std::vector<double> ones((size_t)q * n_out, 1.0 / q);
            FS_HIP(coef.upload(ones, st));
            FS_HIP(hipStreamSynchronize(st)); // (the host array goes out of scope)
        }
        CombineSources src;
        src.S[0] = S.p;
        src.C[0] = coef.p;
        src.q[0] = q;
        int fused = 0;
        FS_HIP(hipStreamSynchronize(st));
        FS_HIP(hipEventRecord(c->ev0, st));
        for (int32_t i = 0; i < reps; i++) {
            if (which == FEMSHELL_KERNEL_SPMM) block_product(c->dm, S.p, Y.p, ld, nc, tb.p, p.total_slots() * 6, st, &fused);
            else if (which == FEMSHELL_KERNEL_GRAM) launch_gram(c->dm, q, S.p, q, S.p, ld, c->mass.p, partials.p, G.p, st);
            else launch_block_combine(c->dm, src, n_out, n_out, Y.p, ld, st);
        }
        FS_HIP(hipEventRecord(c->ev1, st));
        FS_HIP(hipStreamSynchronize(st));
        FS_HIP(hipGetLastError());
        float ms = 0.f;
        FS_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        *mean_ms_out = (double)ms / reps;
        if (bytes_out) {
            const double n = p.n_own;
            // product: every stored block once per pass of four columns (fused) or once per column, indices alike, x read and y
            // written per column (the transposed products beside the slots are overhead of the method, as in bytes_spmv); Gram:
            // the operand and the mass once (A = B); combine: 3c columns read, 2c written
            const double passes = fused ? (double)((nc + spmm_pass_cols(c->dm) - 1) / spmm_pass_cols(c->dm)) : (double)nc;
            *bytes_out = which == FEMSHELL_KERNEL_SPMM ? passes * (bytes_spmv(c) - 96.0 * n) + 96.0 * n * nc
                         : which == FEMSHELL_KERNEL_GRAM ? 48.0 * n * (q + 1)
                                                         : 48.0 * n * (q + n_out);
        }
        return FEMSHELL_OK;
    }
    if (which == FEMSHELL_KERNEL_ELEMENT_PRODUCT) {
        // the matrix-free product with the unconstrained element matrices on a hashed vector, back to back between one event pair
        if (c->cfg.world_size != 1) return set_err(FEMSHELL_ERR_UNSUPPORTED, "femshell_time_kernel: the element product runs on single-rank contexts");
        hipStream_t st = c->stream;
        const Plan &p = c->plan;
        const int64_t ld = (int64_t)p.n_local_nodes() * 6;
        DevBuf<double> S, Y;
        FS_HIP(S.alloc((size_t)ld));
        FS_HIP(S.zero(st));
        FS_HIP(Y.alloc((size_t)p.n_pad * 6));
        launch_modal_init(c->dm, nullptr, 1, S.p, ld, st);
        FS_HIP(hipStreamSynchronize(st));
        FS_HIP(hipEventRecord(c->ev0, st));
        for (int32_t i = 0; i < reps; i++) launch_element_product(c->dm, c->mc, c->sections_or_null(), S.p, nullptr, nullptr, Y.p, false, st);
        FS_HIP(hipEventRecord(c->ev1, st));
        FS_HIP(hipGetLastError());
        rc = check_status(c, "femshell_time_kernel");
        if (rc) return rc;
        float ms = 0.f;
        FS_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        *mean_ms_out = (double)ms / reps;
        // coordinates once per node, the node ids of the slices' element lists (16 B per entry, counted as listed, as for the
        // lumped mass; a section index beside each where the context has sections), x read and y written once per node.  (What
        // the lanes of phase B gather of x beyond that comes from the caches: overhead of the method, not algorithmic traffic.)
        if (bytes_out)
            *bytes_out = 24.0 * p.n_own + (16.0 + (c->have_sections ? 4.0 : 0.0)) * (double)p.slice_elem_nodes.size() / 4.0 + 96.0 * p.n_own;
        return FEMSHELL_OK;
    }
    if (which == FEMSHELL_KERNEL_ELEMENT_RESULTANTS) {
        // the element resultants of a hashed displacement vector, back to back between one event pair (rows in the local order: the
        // host's part of femshell_element_resultants is not timed)
        if (c->cfg.world_size != 1) return set_err(FEMSHELL_ERR_UNSUPPORTED, "femshell_time_kernel: the element resultants run on single-rank contexts");
        hipStream_t st = c->stream;
        const Plan &p = c->plan;
        const int64_t ld = (int64_t)p.n_local_nodes() * 6;
        DevBuf<double> S, R, thick;
        FS_HIP(S.alloc((size_t)ld));
        FS_HIP(S.zero(st));
        FS_HIP(R.alloc(((size_t)p.n_ltri() + (size_t)p.n_lquad()) * 14));
        const double *sec_t = nullptr;
        rc = upload_section_thickness(c, &thick, &sec_t);
        if (rc) return rc;
        launch_modal_init(c->dm, nullptr, 1, S.p, ld, st);
        FS_HIP(hipStreamSynchronize(st));
        FS_HIP(hipEventRecord(c->ev0, st));
        for (int32_t i = 0; i < reps; i++) launch_element_resultants(c->dm, c->mc, c->sections_or_null(), sec_t, S.p, nullptr, R.p, st);
        FS_HIP(hipEventRecord(c->ev1, st));
        FS_HIP(hipGetLastError());
        rc = check_status(c, "femshell_time_kernel");
        if (rc) return rc;
        float ms = 0.f;
        FS_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        *mean_ms_out = (double)ms / reps;
        if (bytes_out) *bytes_out = bytes_element_resultants(c);
        return FEMSHELL_OK;
    }
    if (which == FEMSHELL_KERNEL_ELEMENT_LOADS) {
        // hashed element values from the loads in force into a scratch vector (api_element_loads.cpp): every rank times its own rows
        rc = time_element_loads(c, reps, mean_ms_out);
        if (rc) return rc;
        if (bytes_out) *bytes_out = bytes_element_loads(c);
        return FEMSHELL_OK;
    }
    if (which == FEMSHELL_KERNEL_ELEMENT_THERMAL) {
        // hashed temperatures from the loads in force into a scratch vector (api_thermal.cpp): every rank times its own rows
        rc = time_element_thermal(c, reps, mean_ms_out);
        if (rc) return rc;
        if (bytes_out) *bytes_out = bytes_element_thermal(c);
        return FEMSHELL_OK;
    }
    if (which == FEMSHELL_KERNEL_ELASTIC_SUPPORT) {
        // hashed moduli into a scratch table (api_elastic_support.cpp): every rank times its own rows
        rc = time_elastic_support(c, reps, mean_ms_out);
        if (rc) return rc;
        if (bytes_out) *bytes_out = bytes_elastic_support(c);
        return FEMSHELL_OK;
    }
    if (which == FEMSHELL_KERNEL_NODAL_RECOVERY || which == FEMSHELL_KERNEL_RECOVERY_ERROR) {
        // the element rows of a hashed displacement vector, averaged to the nodes / compared with the average (api_resultants.cpp)
        if (c->cfg.world_size != 1) return set_err(FEMSHELL_ERR_UNSUPPORTED, "femshell_time_kernel: the nodal recovery runs on single-rank contexts");
        rc = time_recovery(c, which == FEMSHELL_KERNEL_RECOVERY_ERROR, reps, mean_ms_out);
        if (rc) return rc;
        if (bytes_out) *bytes_out = which == FEMSHELL_KERNEL_RECOVERY_ERROR ? bytes_recovery_error(c) : bytes_nodal_recovery(c);
        return FEMSHELL_OK;
    }
    if (which == FEMSHELL_KERNEL_GEOMETRIC_PRODUCT) {
        // one pass of four columns on hashed coefficients and vectors (api_buckling.cpp)
        if (c->cfg.world_size != 1) return set_err(FEMSHELL_ERR_UNSUPPORTED, "femshell_time_kernel: the geometric product runs on single-rank contexts");
        rc = time_geometric_product(c, reps, mean_ms_out);
        if (rc) return rc;
        if (bytes_out) *bytes_out = bytes_geometric_product(c, 4);
        return FEMSHELL_OK;
    }
    if (which != FEMSHELL_KERNEL_ASSEMBLE && (rc = ensure(c, kK | kF | kJacobi))) return rc;
    hipStream_t st = c->stream;
    const Plan &p = c->plan;
    const size_t nrow = (size_t)p.n_pad * 6, nrow_ext = (size_t)p.n_local_nodes() * 6;
    CgVectors v;
    if (which != FEMSHELL_KERNEL_ASSEMBLE) {
        FS_HIP(c->bx.alloc(nrow));
        FS_HIP(c->br.alloc(nrow));
        FS_HIP(c->bz.alloc(nrow));
        FS_HIP(c->bq.alloc(nrow));
        FS_HIP(c->bp.alloc(nrow_ext));
        FS_HIP(c->bpart.alloc(2 * (size_t)slice_grid(c->dm)));
        FS_HIP(c->bscal.alloc(1));
        FS_HIP(c->bscal.zero(st)); // the reduction's ticket counter must start at 0 (recycled memory is not)
        v.x = c->bx.p; v.r = c->br.p; v.z = c->bz.p; v.p = c->bp.p; v.q = c->bq.p;
        v.b = c->F.p; v.partials = c->bpart.p; v.s = c->bscal.p; v.hist = nullptr; v.hist_cap = 0;
        FS_HIP(c->bp.zero(st));
        launch_cg_init(c->dm, v, false, st);                // x=0, r=b, z=M^-1 b, p=z
        launch_cg_scalar(c->dm, v, true, 2, CG_PHASE_INIT, 0.0, st);
        launch_spmv(c->dm, v.p, v.q, SpmvEpilogue(), v.s, st, SpmvSpan(), v.partials);  // q = A p
        launch_cg_scalar(c->dm, v, true, 1, CG_PHASE_ALPHA, 0.0, st);
    }
    FS_HIP(hipStreamSynchronize(st));
    double bytes = 0.0;
    if (which == FEMSHELL_KERNEL_ASSEMBLE) {
        FS_HIP(hipEventRecord(c->ev0, st));
        for (int32_t i = 0; i < reps; i++)
            if (!launch_assemble(c->dm, c->mc, st, c->sections_or_null()))
                return set_err(FEMSHELL_ERR_INVALID, "femshell_time_kernel: the context's sections have no table in HBM");
        FS_HIP(hipEventRecord(c->ev1, st));
        FS_HIP(hipStreamSynchronize(st));
        FS_HIP(hipGetLastError());
        float ms = 0.f;
        FS_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        *mean_ms_out = (double)ms / reps;
        bytes = bytes_assemble(c);
    } else {
        // the CG kernels are timed where they run: `reps` iterations of the local recurrence (this rank's rows, no
        // communication, no stopping test), an event pair around the chosen kernel of every iteration.  A kernel
        // launched back to back with itself finds different cache contents and measured up to 13 % faster.
        if (which != FEMSHELL_KERNEL_SPMV && which != FEMSHELL_KERNEL_CG_UPDATE && which != FEMSHELL_KERNEL_CG_DIRECTION)
            return set_err(FEMSHELL_ERR_INVALID, "femshell_time_kernel: unknown kernel");
        double sum_ms = 0.0;
        for (int32_t i = 0; i < reps; i++) {
            // (as cg_classic runs them: with symmetric storage the SpMV is its first phase and the update kernel
            // collects the transposed products)
            if (which == FEMSHELL_KERNEL_SPMV) FS_HIP(hipEventRecord(c->ev0, st));
            if (c->dm.symmetric) launch_spmv_sym_phase1(c->dm, v.p, v.q, v.partials, v.s, st);
            else launch_spmv(c->dm, v.p, v.q, SpmvEpilogue(), v.s, st, SpmvSpan(), v.partials);
            if (which == FEMSHELL_KERNEL_SPMV) FS_HIP(hipEventRecord(c->ev1, st));
            launch_cg_scalar(c->dm, v, true, 1, CG_PHASE_ALPHA, 0.0, st);
            if (which == FEMSHELL_KERNEL_CG_UPDATE) FS_HIP(hipEventRecord(c->ev0, st));
            launch_cg_update(c->dm, v, st, c->dm.symmetric != 0);
            if (which == FEMSHELL_KERNEL_CG_UPDATE) FS_HIP(hipEventRecord(c->ev1, st));
            launch_cg_scalar(c->dm, v, true, 2, CG_PHASE_BETA, 0.0, st);
            if (which == FEMSHELL_KERNEL_CG_DIRECTION) FS_HIP(hipEventRecord(c->ev0, st));
            launch_cg_direction(c->dm, v, st);
            if (which == FEMSHELL_KERNEL_CG_DIRECTION) FS_HIP(hipEventRecord(c->ev1, st));
            FS_HIP(hipStreamSynchronize(st));
            float ms = 0.f;
            FS_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
            sum_ms += ms;
        }
        FS_HIP(hipGetLastError());
        *mean_ms_out = sum_ms / reps;
        bytes = which == FEMSHELL_KERNEL_SPMV ? bytes_spmv(c) : which == FEMSHELL_KERNEL_CG_UPDATE ? bytes_update(c) : bytes_direction(c);
    }
    if (bytes_out) *bytes_out = bytes;
    return which == FEMSHELL_KERNEL_ASSEMBLE ? timed_assembly_done(c) : FEMSHELL_OK;
}

} // extern "C"
