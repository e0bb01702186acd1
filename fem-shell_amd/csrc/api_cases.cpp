// api_cases.cpp -- the C ABI of the load cases: femshell_solve_cases.  Block-Jacobi contexts run the lockstep CG
// of cases.cpp on buffers of the call's own; multigrid contexts run the cases one after another through solve_vector.
#include "api_internal.hpp"
#include "cases.hpp"

#include <algorithm>
#include <cmath>

using namespace femshell;

namespace femshell {

// One iteration of a pass of nb columns: the stored blocks of K and the inverse diagonal blocks once; per column the product's
// input and result, p and q of the dot, the update (p, q, x, r read; x, r, z written) and the direction (z, p read; p written)
double bytes_cases_iteration(const femshell_ctx *c, int nb)
{
    const double n = (double)c->plan.n_own;
    return (bytes_spmv(c) - 96.0 * n) + 168.0 * n + nb * (2.0 + 2.0 + 7.0 + 3.0) * 48.0 * n;
}

} // namespace femshell

extern "C" {

int femshell_solve_cases(femshell_ctx *c, int32_t n_cases, const double *loads, double rtol, int32_t max_it, double *u_out,
                         femshell_case_info *case_info, femshell_cases_info *info)
{
    if (!c || !loads || !u_out) return set_err(FEMSHELL_ERR_INVALID, "femshell_solve_cases: null argument");
    if (c->cfg.world_size != 1)
        return set_err(FEMSHELL_ERR_UNSUPPORTED, "femshell_solve_cases: single-rank contexts only (load cases on a row partition are not implemented)");
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, "femshell_solve_cases: no mesh set");
    if (n_cases < 1 || n_cases > kCasesMax) return set_err(FEMSHELL_ERR_INVALID, "femshell_solve_cases: n_cases must be in 1 .. 32");
    if (max_it < 0) return set_err(FEMSHELL_ERR_INVALID, "femshell_solve_cases: max_it < 0");
    if (c->dyn.active) return set_err(FEMSHELL_ERR_INVALID, "femshell_solve_cases: not while dynamics is active (femshell_dynamics_end first)");
    if (c->have_prescribed)
        return set_err(FEMSHELL_ERR_INVALID, "femshell_solve_cases: prescribed displacements are in force (femshell_set_prescribed with n = 0 clears them)");
    const Plan &p = c->plan;
    const size_t n6 = (size_t)p.n_nodes * 6;
    for (int32_t j = 0; j < n_cases; j++)
        if (!all_finite(loads + (size_t)j * n6, (int64_t)n6))
            return set_err(FEMSHELL_ERR_INVALID, "femshell_solve_cases: non-finite entry in the loads of case " + std::to_string(j + 1));
    if (const int prc = finish_pending_assembly(c)) return prc;
    TraceRange trace("femshell_solve_cases");
    int rc = select_device(c);
    if (rc) return rc;
    const bool use_amg = c->pc.type == FEMSHELL_PC_AMG;
    rc = ensure(c, kK | kJacobi | (use_amg ? kHierarchy : 0u));
    if (rc) return rc;
    hipStream_t st = c->stream;
    const int64_t ld = (int64_t)p.n_local_nodes() * 6;

    // the loads of every case, masked: zero on the fixed dofs, the padding rows and the ghost space
    DevBuf<double> R, X;
    std::vector<double> stage;
    FS_HIP(R.alloc((size_t)n_cases * (size_t)ld));
    FS_HIP(X.alloc((size_t)n_cases * (size_t)ld));
    FS_HIP(X.zero(st));
    rc = upload_node_block(c, NodeOrder::caller, n_cases, loads, R.p, (size_t)ld, &stage);
    if (rc) return rc;
    launch_block_mask(c->dm, R.p, ld, n_cases, st);
    FS_HIP(hipGetLastError());

    std::vector<femshell_case_info> ci((size_t)n_cases, femshell_case_info{0, 0, 0.0});
    int passes = 0, fused = 0;
    double bytes = 0.0;
    bool breakdown = false;
    FS_HIP(hipEventRecord(c->ev0, st));
    if (!use_amg) {
        CasesProblem cp;
        cp.dm = c->dm;
        cp.ld = ld;
        cp.total_slots = p.total_slots();
        cp.stream = st;
        cp.n_cases = n_cases;
        cp.rtol = rtol;
        cp.max_it = max_it;
        cp.R = R.p;
        cp.X = X.p;
        CasesResult res;
        rc = cases_lockstep_cg(cp, &res);
        if (rc) return rc;
        passes = res.passes;
        fused = res.fused_product;
        for (int32_t j = 0; j < n_cases; j++) {
            const CaseScalars &s = res.cases[(size_t)j];
            ci[(size_t)j].iterations = s.iters;
            ci[(size_t)j].converged = s.done;
            ci[(size_t)j].rel_residual = s.bb > 0.0 ? std::sqrt(s.rr / s.bb) : 0.0;
            breakdown = breakdown || s.done < 0;
        }
        const int kb = spmm_pass_cols(c->dm);
        for (int32_t j0 = 0; j0 < n_cases; j0 += kb) bytes += bytes_cases_iteration(c, std::min<int32_t>(kb, n_cases - j0));
    } else {
        for (int32_t j = 0; j < n_cases; j++) {
            int32_t it = 0, conv = 0;
            rc = solve_vector(c, R.p + (size_t)j * ld, X.p + (size_t)j * ld, rtol, max_it, &it, &conv);
            if (rc != FEMSHELL_OK && rc != FEMSHELL_ERR_BREAKDOWN) return rc;
            CgScalars hs{};
            FS_HIP(hipMemcpyAsync(&hs, c->scal.p, sizeof hs, hipMemcpyDeviceToHost, st));
            FS_HIP(hipStreamSynchronize(st));
            ci[(size_t)j].iterations = it;
            ci[(size_t)j].converged = rc == FEMSHELL_ERR_BREAKDOWN ? -1 : conv;
            ci[(size_t)j].rel_residual = hs.bb > 0.0 ? std::sqrt(hs.rr / hs.bb) : 0.0;
            breakdown = breakdown || rc == FEMSHELL_ERR_BREAKDOWN;
            passes++;
        }
        launch_block_mask(c->dm, X.p, ld, n_cases, st); // (the multigrid cycle leaves what the identity rows of K give on constrained dofs)
        FS_HIP(hipGetLastError());
        bytes = n_cases * (bytes_spmv(c) + (8.0 + 3.0 + 3.0) * 48.0 * p.n_own + amg_cycle_bytes(c));
    }
    FS_HIP(hipEventRecord(c->ev1, st));
    rc = download_node_block(c, NodeOrder::caller, n_cases, X.p, (size_t)ld, u_out); // (synchronises)
    if (rc) return rc;
    float ms = 0.f;
    FS_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (case_info) std::copy(ci.begin(), ci.end(), case_info);
    if (info) {
        info->passes = passes;
        info->fused_product = fused;
        info->pc_type = c->pc.type;
        info->reserved = 0;
        info->solve_seconds = 1e-3 * ms;
        info->bytes_per_iteration = bytes;
    }
    if (breakdown)
        return set_err(FEMSHELL_ERR_BREAKDOWN, "femshell_solve_cases: CG breakdown in at least one case, p.Ap <= 0 (femshell_case_info::converged = -1 names them)");
    return FEMSHELL_OK;
}

} // extern "C"
