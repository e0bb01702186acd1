// api_dynamics.cpp -- the C ABI of structural dynamics: density, lumped mass, Newmark time stepping (femshell_dynamics_*).
#include "api_internal.hpp"

#include <cmath>

using namespace femshell;

extern "C" {

int femshell_set_density(femshell_ctx *c, double rho, int32_t n_sections, const double *section_rho)
{
    if (!c) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_density: null context");
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_density: call femshell_set_mesh first");
    if (c->dyn.active) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_density: not while dynamics is active (femshell_dynamics_end first)");
    if (n_sections < 0) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_density: n_sections < 0");
    if (n_sections == 0) {
        if (!(std::isfinite(rho) && rho > 0.0)) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_density: need a finite rho > 0");
        c->rho = rho;
        c->sec_rho.clear();
    } else {
        if (!c->have_sections || n_sections != c->n_sections)
            return set_err(FEMSHELL_ERR_INVALID, "femshell_set_density: n_sections must be the context's section count (" +
                                                     std::to_string(c->have_sections ? c->n_sections : 0) + ")");
        if (!section_rho) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_density: section_rho is null");
        for (int32_t s = 0; s < n_sections; s++)
            if (!(std::isfinite(section_rho[s]) && section_rho[s] > 0.0))
                return set_err(FEMSHELL_ERR_INVALID, "femshell_set_density: section " + std::to_string(s) + ": need a finite density > 0");
        c->sec_rho.assign(section_rho, section_rho + n_sections);
        c->rho = 0.0;
    }
    c->have_density = true;
    invalidate(c, Change::density);
    return FEMSHELL_OK;
}

int femshell_lumped_mass(femshell_ctx *c, double *m6_out)
{
    if (!c || !m6_out) return set_err(FEMSHELL_ERR_INVALID, "femshell_lumped_mass: null argument");
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, "femshell_lumped_mass: no mesh set");
    if (!c->have_density) return set_err(FEMSHELL_ERR_INVALID, "femshell_lumped_mass: no density set (femshell_set_density)");
    int rc = select_device(c);
    if (rc) return rc;
    rc = ensure(c, kMass);
    if (rc) return rc;
    return gather_node_vector(c, c->mass.p, m6_out);
}

int femshell_dynamics_defaults(femshell_dynamics_options *out)
{
    if (!out) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_defaults: null argument");
    out->dt = 0.0;
    out->beta = 0.25;
    out->gamma = 0.5;
    out->alpha = 0.0;
    return FEMSHELL_OK;
}

int femshell_dynamics_begin(femshell_ctx *c, const femshell_dynamics_options *opt, const double *u0, const double *v0)
{
    if (!c || !opt) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_begin: null argument");
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_begin: no mesh set");
    if (c->dyn.active) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_begin: dynamics is active already (femshell_dynamics_end first)");
    if (!c->have_density) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_begin: no density set (femshell_set_density)");
    if (c->have_prescribed)
        return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_begin: prescribed displacements are in force (femshell_set_prescribed with n = 0 clears them)");
    const double dt = opt->dt, beta = opt->beta, gamma = opt->gamma, alpha = opt->alpha;
    if (!(std::isfinite(dt) && dt > 0.0)) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_begin: need a finite dt > 0");
    if (!(std::isfinite(gamma) && gamma >= 0.5)) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_begin: need gamma >= 1/2");
    // (the limit itself is allowed as written in decimals: beta 0.3025 with gamma 0.6, where 0.25 * 1.1 * 1.1 rounds upwards)
    if (!(std::isfinite(beta) && beta * (1.0 + 1e-12) >= 0.25 * (gamma + 0.5) * (gamma + 0.5)))
        return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_begin: need beta >= (gamma + 1/2)^2 / 4 (the unconditionally stable schemes)");
    if (!(std::isfinite(alpha) && alpha >= 0.0)) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_begin: need a finite alpha >= 0");
    const Plan &p = c->plan;
    if (u0 && !all_finite(u0, 6ll * p.n_nodes)) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_begin: non-finite entry in u0");
    if (v0 && !all_finite(v0, 6ll * p.n_nodes)) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_begin: non-finite entry in v0");
    if (const int prc = finish_pending_assembly(c)) return prc;
    CommWatch watch(c->cfg.rank, c->comm.active() ? c->cfg.world_size : 1, "femshell_dynamics_begin (assembly, halo exchange of K u0)");
    int rc = select_device(c);
    if (rc) return rc;
    rc = ensure(c, kMass | kK | kF); // K itself: dynamics is not active yet
    if (rc) return rc;
    hipStream_t st = c->stream;
    femshell_ctx::Dynamics &d = c->dyn;
    const size_t n6 = (size_t)p.n_pad * 6;
    for (int i = 0; i < 2; i++) {
        FS_HIP(d.u[i].alloc(n6));
        FS_HIP(d.v[i].alloc(n6));
        FS_HIP(d.a[i].alloc(n6));
    }
    FS_HIP(d.b.alloc(n6));
    FS_HIP(d.e_partials.alloc(3 * (size_t)kEnergyGrid));
    FS_HIP(d.e_sums.alloc(3));
    // the caller's vectors land in the candidate's buffers; K u0 with the K in HBM, before the shift
    std::vector<double> stage_u, stage_v; // (synchronised below)
    if (u0) {
        rc = upload_node_block(c, NodeOrder::caller, 1, u0, d.u[1].p, n6, &stage_u);
        if (rc) return rc;
        FS_HIP(hipMemcpyAsync(c->p.p, d.u[1].p, n6 * sizeof(double), hipMemcpyDeviceToDevice, st));
        rc = halo_exchange(c, c->p.p, st);
        if (rc) return rc;
        launch_spmv(c->dm, c->p.p, c->q.p, SpmvEpilogue(), nullptr, st);
    }
    if (v0) {
        rc = upload_node_block(c, NodeOrder::caller, 1, v0, d.v[1].p, n6, &stage_v);
        if (rc) return rc;
    }
    launch_newmark_init(c->dm, c->mass.p, c->F.p, u0 ? c->q.p : nullptr, u0 ? d.u[1].p : nullptr, v0 ? d.v[1].p : nullptr, alpha, d.u[0].p,
                        d.v[0].p, d.a[0].p, st);
    d.k.a0 = 1.0 / (beta * dt * dt);
    d.k.a1 = gamma / (beta * dt);
    d.k.a2 = 1.0 / (beta * dt);
    d.k.a3 = 1.0 / (2.0 * beta) - 1.0;
    d.k.a4 = gamma / beta - 1.0;
    d.k.a5 = 0.5 * dt * (gamma / beta - 2.0);
    d.k.alpha = alpha;
    d.k.dt = dt;
    d.k.gamma = gamma;
    d.k.shift = d.k.a0 + alpha * d.k.a1;
    launch_mass_shift(c->dm, c->mass.p, d.k.shift, st); // the matrix in HBM is K_eff from here on
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(st));
    d.cur = 0;
    d.have_candidate = false;
    d.active = true;
    invalidate(c, Change::dynamics_begin); // block-Jacobi and the multigrid hierarchy: from K_eff, at the first step
    return FEMSHELL_OK;
}

int femshell_dynamics_step(femshell_ctx *c, double rtol, int32_t max_it, femshell_solve_info *info)
{
    if (!c) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_step: null context");
    if (!c->dyn.active) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_step: call femshell_dynamics_begin first");
    int rc = select_device(c);
    if (rc) return rc;
    femshell_ctx::Dynamics &d = c->dyn;
    const size_t n6 = (size_t)c->plan.n_pad * 6;
    // the solve starts from the committed u (the hand-over of femshell_set_initial_guess)
    FS_HIP(c->x0.alloc(n6));
    FS_HIP(hipMemcpyAsync(c->x0.p, d.u[d.cur].p, n6 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    c->warm_next = true;
    rc = solve_system(c, rtol, max_it, nullptr, info, true);
    if (rc) return rc;
    launch_newmark_update(c->dm, d.k, c->x.p, d.u[d.cur].p, d.v[d.cur].p, d.a[d.cur].p, d.u[d.cur ^ 1].p, d.v[d.cur ^ 1].p, d.a[d.cur ^ 1].p,
                          c->stream);
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(c->stream));
    d.have_candidate = true;
    return FEMSHELL_OK;
}

int femshell_dynamics_accept(femshell_ctx *c)
{
    if (!c) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_accept: null context");
    if (!c->dyn.active) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_accept: call femshell_dynamics_begin first");
    if (!c->dyn.have_candidate) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_accept: no candidate (femshell_dynamics_step first)");
    c->dyn.cur ^= 1; // the candidate's buffers become the committed ones: no copy
    c->dyn.have_candidate = false;
    return FEMSHELL_OK;
}

int femshell_dynamics_state(femshell_ctx *c, int32_t which, double *u, double *v, double *a)
{
    if (!c) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_state: null context");
    if (!c->dyn.active) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_state: call femshell_dynamics_begin first");
    if (which != 0 && which != 1) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_state: which must be 0 (committed) or 1 (candidate)");
    if (which == 1 && !c->dyn.have_candidate) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_state: no candidate (femshell_dynamics_step first)");
    int rc = select_device(c);
    if (rc) return rc;
    const femshell_ctx::Dynamics &d = c->dyn;
    const int i = which == 0 ? d.cur : d.cur ^ 1;
    if (u) rc = gather_node_vector(c, d.u[i].p, u);
    if (!rc && v) rc = gather_node_vector(c, d.v[i].p, v);
    if (!rc && a) rc = gather_node_vector(c, d.a[i].p, a);
    return rc;
}

int femshell_dynamics_energy(femshell_ctx *c, int32_t which, double out[2])
{
    if (!c || !out) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_energy: null argument");
    if (!c->dyn.active) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_energy: call femshell_dynamics_begin first");
    if (which != 0 && which != 1) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_energy: which must be 0 (committed) or 1 (candidate)");
    if (which == 1 && !c->dyn.have_candidate) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_energy: no candidate (femshell_dynamics_step first)");
    CommWatch watch(c->cfg.rank, c->comm.active() ? c->cfg.world_size : 1, "femshell_dynamics_energy (halo exchange and all-reduce)");
    int rc = select_device(c);
    if (rc) return rc;
    rc = ensure(c, kK);
    if (rc) return rc;
    femshell_ctx::Dynamics &d = c->dyn;
    const int i = which == 0 ? d.cur : d.cur ^ 1;
    hipStream_t st = c->stream;
    // q = K_eff u through the SpMV kernel, whose input carries the ghost entries (the CG vectors are free between solves);
    // u.K u = u.q - shift u.M u: u is zero on the constrained dofs, where K_eff has no shift
    FS_HIP(hipMemcpyAsync(c->p.p, d.u[i].p, (size_t)c->plan.n_pad * 6 * sizeof(double), hipMemcpyDeviceToDevice, st));
    rc = halo_exchange(c, c->p.p, st);
    if (rc) return rc;
    launch_spmv(c->dm, c->p.p, c->q.p, SpmvEpilogue(), nullptr, st);
    launch_newmark_energy(c->dm, c->mass.p, d.u[i].p, d.v[i].p, c->q.p, d.e_partials.p, d.e_sums.p, st);
    FS_HIP(hipGetLastError());
    if (c->comm.active()) {
        std::string e;
        if (!comm_allreduce_sum(c->comm, d.e_sums.p, 3, st, &e)) return set_err(FEMSHELL_ERR_COMM, e);
    }
    double h[3] = {0.0, 0.0, 0.0};
    FS_HIP(hipMemcpyAsync(h, d.e_sums.p, sizeof h, hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st));
    out[0] = 0.5 * h[0];
    out[1] = 0.5 * h[1] - 0.5 * d.k.shift * h[2];
    return FEMSHELL_OK;
}

int femshell_dynamics_end(femshell_ctx *c)
{
    if (!c) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_end: null context");
    if (!c->dyn.active) return set_err(FEMSHELL_ERR_INVALID, "femshell_dynamics_end: dynamics is not active");
    int rc = select_device(c);
    if (rc) return rc;
    FS_HIP(hipStreamSynchronize(c->stream));
    c->dyn.reset();
    invalidate(c, Change::dynamics_end); // K and F again at the next use
    return FEMSHELL_OK;
}

} // extern "C"
