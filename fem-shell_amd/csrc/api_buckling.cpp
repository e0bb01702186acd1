// api_buckling.cpp -- the C ABI of linear buckling: femshell_geometric_product and its timing hook (kernels:
// geometric_stiffness.hip), femshell_buckling (solver: buckling.cpp).
#include "api_internal.hpp"
#include "buckling.hpp"
#include "geometric_stiffness.hpp"
#include "modal.hpp"

#include <algorithm>
#include <cmath>

using namespace femshell;

namespace femshell {

// one pass of k_geometric_product over `cols` columns (1 .. 4): per listed entry 16 B of node ids, 4 B of element index and
// 48 / 80 B of coefficients; per node and column 24 B of translations read and 48 B written
double bytes_geometric_product(const femshell_ctx *c, int cols)
{
    const Plan &p = c->plan;
    const double coeff = p.n_lquad() > 0 ? 80.0 : 48.0;
    return (16.0 + 4.0 + coeff) * (double)p.slice_elems.size() + (24.0 + 48.0) * (double)p.n_own * cols;
}

// The coefficients g_ab of every local element in HBM (geometric_coeff_words doubles each), from the prestress of u (n_nodes x 6,
// the caller's numbering) or, u == nullptr, of the last solution with its prescribed part: k_element_resultants, unchanged, then
// k_geometric_coeff.  The caller has checked that a mesh is set and that the NULL form has a solution.  Synchronises the stream.
int geometric_coefficients(femshell_ctx *c, const double *u, DevBuf<double> *coeff, const char *what)
{
    const Plan &p = c->plan;
    const size_t ld = (size_t)p.n_local_nodes() * 6, ne = (size_t)p.n_ltri() + (size_t)p.n_lquad();
    int rc = ensure_slice_elem_local(c);
    if (rc) return rc;
    DevBuf<double> x, res, thick;
    std::vector<double> stage;
    if (u) {
        FS_HIP(x.alloc(ld));
        rc = upload_node_block(c, NodeOrder::caller, 1, u, x.p, ld, &stage);
        if (rc) return rc;
    }
    const double *ux = u ? x.p : c->x.p, *up = nullptr;
    if (!u && c->have_prescribed) { // the solution in HBM is the homogeneous part: the kernel adds u_bar entry by entry
        rc = resolve_prescribed(c);
        if (rc) return rc;
        if (c->ubar_nonzero) up = c->ubar.p;
    }
    const double *sec_t = nullptr;
    rc = upload_section_thickness(c, &thick, &sec_t);
    if (rc) return rc;
    FS_HIP(res.alloc(std::max<size_t>(ne, 1) * 14));
    FS_HIP(coeff->alloc(std::max<size_t>(ne, 1) * (size_t)geometric_coeff_words(c->dm)));
    ThermalView tv; // (temperatures in force: the membrane forces of the heated shell, through the same switch as the resultants)
    launch_element_resultants(c->dm, c->mc, c->sections_or_null(), sec_t, ux, up, res.p, c->stream, thermal_view_or_null(c, &tv));
    launch_geometric_coeff(c->dm, res.p, coeff->p, c->stream);
    FS_HIP(hipGetLastError());
    return check_status(c, what); // (synchronises: x, res and the staging copy go out of scope)
}

// femshell_time_kernel: a four-column pass back to back between the context's event pair, on hashed coefficients and hashed
// vectors -- nothing of the context changes but the map of the lists, which a mesh gets once anyway
int time_geometric_product(femshell_ctx *c, int32_t reps, double *mean_ms_out)
{
    const Plan &p = c->plan;
    hipStream_t st = c->stream;
    const size_t ne = (size_t)p.n_ltri() + (size_t)p.n_lquad(), words = (size_t)geometric_coeff_words(c->dm);
    const int64_t ld = (int64_t)p.n_local_nodes() * 6;
    RawVec<double> rows(words * std::max<size_t>(ne, 1));
    parallel_chunks((int64_t)rows.size(), [&](int64_t b, int64_t e) {
        for (int64_t q = b; q < e; q++) {
            uint64_t h = (uint64_t)q * 0x9E3779B97F4A7C15ull; // (a fixed hash of the word's index: values in [-1, 1))
            h ^= h >> 29;
            h *= 0xBF58476D1CE4E5B9ull;
            h ^= h >> 32;
            rows[(size_t)q] = (double)(int64_t)(h >> 11) * (1.0 / 4503599627370496.0) - 1.0;
        }
    }, 1 << 18);
    DevBuf<double> cg, X, Y;
    int rc = ensure_slice_elem_local(c);
    if (rc) return rc;
    FS_HIP(cg.upload(rows, st));
    FS_HIP(X.alloc((size_t)kGeoMaxCols * (size_t)ld));
    FS_HIP(X.zero(st));
    FS_HIP(Y.alloc((size_t)kGeoMaxCols * (size_t)ld));
    launch_modal_init(c->dm, nullptr, kGeoMaxCols, X.p, ld, st);
    FS_HIP(hipStreamSynchronize(st));
    FS_HIP(hipEventRecord(c->ev0, st));
    for (int32_t i = 0; i < reps; i++) launch_geometric_product(c->dm, c->slice_elem_local.p, cg.p, X.p, Y.p, ld, kGeoMaxCols, false, st);
    FS_HIP(hipEventRecord(c->ev1, st));
    FS_HIP(hipStreamSynchronize(st));
    FS_HIP(hipGetLastError());
    float ms = 0.f;
    FS_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *mean_ms_out = (double)ms / reps;
    return FEMSHELL_OK;
}

} // namespace femshell

extern "C" {

int femshell_geometric_product(femshell_ctx *c, const double *u, int32_t n_cols, const double *X, double *Y)
{
    if (!c || !X || !Y) return set_err(FEMSHELL_ERR_INVALID, "femshell_geometric_product: null argument");
    if (c->cfg.world_size != 1)
        return set_err(FEMSHELL_ERR_UNSUPPORTED, "femshell_geometric_product: single-rank contexts only (the ghost values of u and X would need a halo exchange)");
    if (n_cols < 1 || n_cols > 96) return set_err(FEMSHELL_ERR_INVALID, "femshell_geometric_product: n_cols must be in 1 .. 96");
    if (const int prc = finish_pending_assembly(c)) return prc;
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, "femshell_geometric_product: no mesh set");
    if (c->dyn.active) return set_err(FEMSHELL_ERR_INVALID, "femshell_geometric_product: dynamics is active (the prestress of a Newmark state is an open end)");
    if (!u && !c->have_solution) return set_err(FEMSHELL_ERR_INVALID, "femshell_geometric_product: no solve has run (pass u)");
    const Plan &p = c->plan;
    if (u && !all_finite(u, 6ll * p.n_nodes)) return set_err(FEMSHELL_ERR_INVALID, "femshell_geometric_product: non-finite entry in u");
    int rc = select_device(c);
    if (rc) return rc;
    DevBuf<double> coeff, dx, dy;
    rc = geometric_coefficients(c, u, &coeff, "femshell_geometric_product");
    if (rc) return rc;
    const int64_t ld = (int64_t)p.n_local_nodes() * 6;
    std::vector<double> stage;
    FS_HIP(dx.alloc((size_t)n_cols * (size_t)ld));
    rc = upload_node_block(c, NodeOrder::caller, n_cols, X, dx.p, (size_t)ld, &stage);
    if (rc) return rc;
    FS_HIP(dy.alloc((size_t)n_cols * (size_t)ld));
    FS_HIP(dy.zero(c->stream));
    launch_geometric_product(c->dm, c->slice_elem_local.p, coeff.p, dx.p, dy.p, ld, n_cols, false, c->stream);
    FS_HIP(hipGetLastError());
    return download_node_block(c, NodeOrder::caller, n_cols, dy.p, (size_t)ld, Y);
}

int femshell_buckling_defaults(femshell_buckling_options *out)
{
    if (!out) return set_err(FEMSHELL_ERR_INVALID, "femshell_buckling_defaults: null argument");
    out->n_modes = 4;
    out->guard = 4;
    out->max_it = 100;
    out->reserved = 0;
    out->tol = 1e-8;
    out->inner_rtol = 0.0;
    return FEMSHELL_OK;
}

int femshell_buckling(femshell_ctx *c, const femshell_buckling_options *opt, const double *u, double *lambda_out, double *modes_out,
                      double *rho_out, femshell_buckling_info *info)
{
    if (!c || !opt || !lambda_out) return set_err(FEMSHELL_ERR_INVALID, "femshell_buckling: null argument");
    if (c->cfg.world_size != 1)
        return set_err(FEMSHELL_ERR_UNSUPPORTED, "femshell_buckling: single-rank contexts only (row-partitioned buckling analysis is not implemented)");
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, "femshell_buckling: no mesh set");
    if (opt->n_modes < 1 || opt->guard < 0 || opt->n_modes + opt->guard > kModalMaxBlock)
        return set_err(FEMSHELL_ERR_INVALID, "femshell_buckling: need n_modes >= 1, guard >= 0 and n_modes + guard <= 32");
    if (!(std::isfinite(opt->tol) && opt->tol > 0.0)) return set_err(FEMSHELL_ERR_INVALID, "femshell_buckling: need a finite tol > 0");
    if (!(std::isfinite(opt->inner_rtol) && opt->inner_rtol >= 0.0)) return set_err(FEMSHELL_ERR_INVALID, "femshell_buckling: need a finite inner_rtol >= 0 (0: tol / 100)");
    if (opt->max_it < 1) return set_err(FEMSHELL_ERR_INVALID, "femshell_buckling: max_it < 1");
    if (c->dyn.active) return set_err(FEMSHELL_ERR_INVALID, "femshell_buckling: not while dynamics is active (femshell_dynamics_end first)");
    if (!u && !c->have_solution) return set_err(FEMSHELL_ERR_INVALID, "femshell_buckling: no solve has run (pass u)");
    const Plan &p = c->plan;
    if (u && !all_finite(u, 6ll * p.n_nodes)) return set_err(FEMSHELL_ERR_INVALID, "femshell_buckling: non-finite entry in u");
    const int mb = opt->n_modes + opt->guard;
    {
        int64_t fixed = 0;
        for (uint8_t b : c->dmask_global) fixed += __builtin_popcount((unsigned)(b & 0x07u));
        if (3ll * p.n_nodes - fixed < 2ll * mb)
            return set_err(FEMSHELL_ERR_INVALID, "femshell_buckling: fewer than 2 (n_modes + guard) free translational dofs");
    }
    if (const int prc = finish_pending_assembly(c)) return prc;
    TraceRange trace("femshell_buckling");
    const double t_begin = wall_s();
    int rc = select_device(c);
    if (rc) return rc;
    // the prestress first: the NULL form reads the last solution where it lies
    DevBuf<double> coeff;
    rc = geometric_coefficients(c, u, &coeff, "femshell_buckling");
    if (rc) return rc;
    rc = ensure(c, kK | kJacobi | (c->pc.type == FEMSHELL_PC_AMG ? kHierarchy : 0u));
    if (rc) return rc;
    hipStream_t st = c->stream;

    BucklingProblem bp;
    bp.dm = c->dm;
    bp.slice_elem_local = c->slice_elem_local.p;
    bp.coeff = coeff.p;
    bp.ld = (int64_t)p.n_local_nodes() * 6;
    bp.total_slots = p.total_slots();
    bp.stream = st;
    bp.solve = [c](const double *b, double *x, double rtol, int32_t *iters) { return solve_vector(c, b, x, rtol, 100000, iters, nullptr); };
    bp.n_modes = opt->n_modes;
    bp.guard = opt->guard;
    bp.max_it = opt->max_it;
    bp.tol = opt->tol;
    // the inner solves run a hundred times tighter than the outer test: their error enters mu and rho in first order
    bp.inner_rtol = opt->inner_rtol > 0.0 ? opt->inner_rtol : opt->tol / 100.0;
    DevBuf<int32_t> node_ids;
    if (!c->perm.empty()) {
        if (hipSuccess != node_ids.upload(c->perm, st) || hipSuccess != hipStreamSynchronize(st))
            return set_err(FEMSHELL_ERR_HIP, "femshell_buckling: upload of the node numbering failed");
        bp.node_ids = node_ids.p;
    }
    BucklingResult res;
    std::unique_ptr<BucklingWork, BucklingWorkDeleter> work;
    rc = buckling_inverse_iteration(bp, &res, &work);
    if (rc) return rc;

    for (int j = 0; j < opt->n_modes; j++) lambda_out[j] = 1.0 / res.mu[(size_t)j];
    if (rho_out)
        for (int j = 0; j < opt->n_modes; j++) rho_out[j] = res.rho[(size_t)j];
    if (modes_out) {
        rc = download_node_block(c, NodeOrder::caller, opt->n_modes, res.X, (size_t)bp.ld, modes_out);
        if (rc) return rc;
        const size_t n6 = (size_t)p.n_nodes * 6;
        for (int j = 0; j < opt->n_modes; j++) { // the translational entry of largest magnitude (lowest index on ties) becomes +1
            double *x = modes_out + (size_t)j * n6;
            size_t big = 0;
            for (size_t i = 0; i < n6; i++)
                if (i % 6 < 3 && std::fabs(x[i]) > std::fabs(x[big])) big = i;
            const double s = x[big];
            if (s != 0.0)
                for (size_t i = 0; i < n6; i++) x[i] /= s;
        }
    }
    if (info) {
        info->iterations = res.iterations;
        info->converged = res.converged;
        info->block = res.block;
        info->pc_type = c->pc.type;
        info->inner_iterations = res.inner_iterations;
        info->rho_max = res.rho_max;
        info->seconds_solves = res.seconds_solves;
        info->seconds_products = res.seconds_products;
        info->seconds_gram = res.seconds_gram;
        info->seconds_update = res.seconds_update;
        info->seconds_total = wall_s() - t_begin;
    }
    return FEMSHELL_OK;
}

} // extern "C"
