// api_modal.cpp -- the C ABI of the modal analysis (modal.cpp, modal.hip): femshell_modes and the block kernels it is made of.
#include "api_internal.hpp"
#include "modal.hpp"

#include <cmath>

using namespace femshell;

extern "C" {

int femshell_modal_defaults(femshell_modal_options *out)
{
    if (!out) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_defaults: null argument");
    out->n_modes = 6;
    out->guard = 4;
    out->max_it = 500;
    out->reserved = 0;
    out->tol = 1e-6;
    out->shift = 0.0;
    return FEMSHELL_OK;
}

int femshell_modal_gram(femshell_ctx *c, int32_t qa, const double *A, int32_t qb, const double *B, int32_t weighted, double *G)
{
    if (!c || !A || !B || !G) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_gram: null argument");
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_gram: no mesh set");
    if (qa < 1 || qa > kModalMaxCols || qb < 1 || qb > kModalMaxCols) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_gram: qa, qb must be in 1 .. 96");
    if (weighted && !c->have_density) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_gram: no density set (femshell_set_density)");
    if (c->cfg.world_size != 1) return set_err(FEMSHELL_ERR_UNSUPPORTED, "femshell_modal_gram: single-rank contexts only");
    int rc = select_device(c);
    if (rc) return rc;
    if (weighted && (rc = ensure(c, kMass))) return rc;
    const size_t ld = (size_t)c->plan.n_local_nodes() * 6;
    DevBuf<double> da, db, partials, dg;
    std::vector<double> stage_a, stage_b; // (synchronised below)
    FS_HIP(da.alloc((size_t)qa * ld));
    FS_HIP(db.alloc((size_t)qb * ld));
    if ((rc = upload_node_block(c, NodeOrder::caller, qa, A, da.p, ld, &stage_a))) return rc;
    if ((rc = upload_node_block(c, NodeOrder::caller, qb, B, db.p, ld, &stage_b))) return rc;
    FS_HIP(partials.alloc((size_t)kGramGrid * qa * qb));
    FS_HIP(dg.alloc((size_t)qa * qb));
    launch_gram(c->dm, qa, da.p, qb, db.p, (int64_t)ld, weighted ? c->mass.p : nullptr, partials.p, dg.p, c->stream);
    FS_HIP(hipGetLastError());
    FS_HIP(hipMemcpyAsync(G, dg.p, (size_t)qa * qb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    FS_HIP(hipStreamSynchronize(c->stream));
    return FEMSHELL_OK;
}

int femshell_modes(femshell_ctx *c, const femshell_modal_options *opt, double *lambda_out, double *modes_out, double *residual_out,
                   femshell_modal_info *info)
{
    if (!c || !opt || !lambda_out) return set_err(FEMSHELL_ERR_INVALID, "femshell_modes: null argument");
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, "femshell_modes: no mesh set");
    if (!c->have_density) return set_err(FEMSHELL_ERR_INVALID, "femshell_modes: no density set (femshell_set_density)");
    if (c->dyn.active) return set_err(FEMSHELL_ERR_INVALID, "femshell_modes: not while dynamics is active (femshell_dynamics_end first)");
    if (opt->n_modes < 1 || opt->guard < 0 || opt->n_modes + opt->guard > kModalMaxBlock)
        return set_err(FEMSHELL_ERR_INVALID, "femshell_modes: need n_modes >= 1, guard >= 0 and n_modes + guard <= 32");
    if (!(std::isfinite(opt->tol) && opt->tol > 0.0)) return set_err(FEMSHELL_ERR_INVALID, "femshell_modes: need a finite tol > 0");
    if (!(std::isfinite(opt->shift) && opt->shift >= 0.0)) return set_err(FEMSHELL_ERR_INVALID, "femshell_modes: need a finite shift >= 0");
    if (opt->max_it < 1) return set_err(FEMSHELL_ERR_INVALID, "femshell_modes: max_it < 1");
    if (c->cfg.world_size != 1)
        return set_err(FEMSHELL_ERR_UNSUPPORTED, "femshell_modes: single-rank contexts only (row-partitioned modal analysis is not implemented)");
    const Plan &p = c->plan;
    const int mb = opt->n_modes + opt->guard;
    {
        int64_t fixed = 0;
        for (uint8_t b : c->dmask_global) fixed += __builtin_popcount((unsigned)(b & 0x3Fu));
        if (6ll * p.n_nodes - fixed < 3ll * mb)
            return set_err(FEMSHELL_ERR_INVALID, "femshell_modes: fewer than 3 (n_modes + guard) free dofs");
    }
    if (const int prc = finish_pending_assembly(c)) return prc;
    TraceRange trace("femshell_modes");
    const double t_begin = wall_s();
    int rc = select_device(c);
    if (rc) return rc;
    rc = ensure(c, kMass | kK | kF, nullptr, /*solving=*/true); // K itself
    if (rc) return rc;
    hipStream_t st = c->stream;
    const bool shifted = opt->shift > 0.0;
    // from here on the matrix in HBM is K + shift M; whatever happens, it is gone when the call returns (femshell_dynamics_end)
    auto leave = [&](int code) {
        if (shifted) {
            (void)hipStreamSynchronize(st);
            invalidate(c, Change::matrix_spoiled);
        }
        return code;
    };
    if (shifted) {
        launch_mass_shift(c->dm, c->mass.p, opt->shift, st);
        invalidate(c, Change::matrix_shifted);
        if (hipGetLastError() != hipSuccess) return leave(set_err(FEMSHELL_ERR_HIP, "femshell_modes: the mass shift could not be launched"));
    }
    Timings t;
    if ((rc = ensure(c, kJacobi | (c->pc.type == FEMSHELL_PC_AMG ? kHierarchy : 0u), &t))) return leave(rc);

    ModalProblem mp;
    mp.dm = c->dm;
    mp.mass = c->mass.p;
    mp.ld = (int64_t)p.n_local_nodes() * 6;
    mp.total_slots = p.total_slots();
    mp.stream = st;
    mp.block_jacobi = c->pc.type != FEMSHELL_PC_AMG;
    if (!mp.block_jacobi) mp.precond = [c](const double *r, double *z) { return amg_apply(c, r, z, nullptr, false); };
    mp.n_modes = opt->n_modes;
    mp.guard = opt->guard;
    mp.max_it = opt->max_it;
    mp.tol = opt->tol;
    mp.shift = opt->shift;
    DevBuf<int32_t> node_ids;
    if (!c->perm.empty()) {
        if (hipSuccess != node_ids.upload(c->perm, st) || hipSuccess != hipStreamSynchronize(st))
            return leave(set_err(FEMSHELL_ERR_HIP, "femshell_modes: upload of the node numbering failed"));
        mp.node_ids = node_ids.p;
    }
    ModalResult res;
    std::unique_ptr<ModalWork, ModalWorkDeleter> work;
    rc = modal_lobpcg(mp, &res, &work);
    if (rc) return leave(rc);

    for (int j = 0; j < opt->n_modes; j++) lambda_out[j] = res.theta[(size_t)j] - opt->shift;
    if (residual_out)
        for (int j = 0; j < opt->n_modes; j++) residual_out[j] = res.residual[(size_t)j];
    if (modes_out) {
        rc = download_node_block(c, NodeOrder::caller, opt->n_modes, res.X, (size_t)mp.ld, modes_out);
        if (rc) return leave(rc);
        const size_t n6 = (size_t)p.n_nodes * 6;
        for (int j = 0; j < opt->n_modes; j++) { // the entry of largest magnitude (lowest index on ties) is positive
            double *x = modes_out + (size_t)j * n6;
            size_t big = 0;
            for (size_t i = 1; i < n6; i++)
                if (std::fabs(x[i]) > std::fabs(x[big])) big = i;
            if (x[big] < 0.0)
                for (size_t i = 0; i < n6; i++) x[i] = -x[i];
        }
    }
    if (info) {
        info->iterations = res.iterations;
        info->converged = res.converged;
        info->block = res.block;
        info->restarts = res.restarts;
        info->fused_product = res.fused_product;
        info->pc_type = c->pc.type;
        info->residual_max = res.residual_max;
        info->seconds_product = res.seconds_product;
        info->seconds_precond = res.seconds_precond;
        info->seconds_gram = res.seconds_gram;
        info->seconds_update = res.seconds_update;
        info->pc_setup_seconds = t.pc_setup_s;
        info->seconds_total = wall_s() - t_begin;
    }
    return leave(FEMSHELL_OK);
}

int femshell_spmm(femshell_ctx *c, int32_t n_cols, const double *X, double *Y)
{
    if (!c || !X || !Y) return set_err(FEMSHELL_ERR_INVALID, "femshell_spmm: null argument");
    if (n_cols < 1 || n_cols > kModalMaxCols) return set_err(FEMSHELL_ERR_INVALID, "femshell_spmm: n_cols must be in 1 .. 96");
    if (const int prc = finish_pending_assembly(c)) return prc;
    if (!have(c, kK)) return set_err(FEMSHELL_ERR_INVALID, "femshell_spmm: call femshell_assemble first");
    if (c->cfg.world_size != 1) return set_err(FEMSHELL_ERR_UNSUPPORTED, "femshell_spmm: single-rank contexts only");
    int rc = select_device(c);
    if (rc) return rc;
    const Plan &p = c->plan;
    const int64_t ld = (int64_t)p.n_local_nodes() * 6;
    DevBuf<double> dx, dy, tb;
    std::vector<double> stage;
    FS_HIP(dx.alloc((size_t)n_cols * (size_t)ld));
    rc = upload_node_block(c, NodeOrder::caller, n_cols, X, dx.p, (size_t)ld, &stage);
    if (rc) return rc;
    FS_HIP(dy.alloc((size_t)n_cols * (size_t)ld));
    FS_HIP(dy.zero(c->stream));
    if (c->dm.symmetric) FS_HIP(tb.alloc((size_t)kSpmmMaxCols * (size_t)p.total_slots() * 6));
    block_product(c->dm, dx.p, dy.p, ld, n_cols, tb.p, p.total_slots() * 6, c->stream, nullptr);
    FS_HIP(hipGetLastError());
    return download_node_block(c, NodeOrder::caller, n_cols, dy.p, (size_t)ld, Y);
}

} // extern "C"
