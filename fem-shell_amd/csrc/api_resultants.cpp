// api_resultants.cpp -- femshell_element_resultants: what the shell carries, element by element (kernel: element_resultants.hip).
#include "api_internal.hpp"

#include <cstring>
#include <vector>

using namespace femshell;

namespace femshell {

// ids and output of every element, coordinates and displacements once per node (what the lanes gather of a node beyond its first
// use comes from the caches); with sections an index per element
double bytes_element_resultants(const femshell_ctx *c)
{
    const Plan &p = c->plan;
    const double ne = (double)p.n_ltri() + p.n_lquad();
    return 12.0 * p.n_ltri() + 16.0 * p.n_lquad() + 112.0 * ne + (24.0 + 48.0) * p.n_own + (c->have_sections ? 4.0 * ne : 0.0);
}

// the thickness of every section in HBM (nullptr without sections): the section table keeps t only inside products
int upload_section_thickness(femshell_ctx *c, DevBuf<double> *buf, const double **sec_t)
{
    *sec_t = nullptr;
    if (!c->have_sections) return FEMSHELL_OK;
    FS_HIP(buf->upload(c->sec_thickness, c->stream)); // (the host vector is the context's: it outlives the stream's work)
    *sec_t = buf->p;
    return FEMSHELL_OK;
}

} // namespace femshell

extern "C" {

int femshell_element_resultants(femshell_ctx *c, const double *u, double *out)
{
    if (!c) return set_err(FEMSHELL_ERR_INVALID, "femshell_element_resultants: null context");
    if (c->cfg.world_size != 1)
        return set_err(FEMSHELL_ERR_UNSUPPORTED, "femshell_element_resultants: single-rank contexts only (the ghost values of u would need a halo exchange)");
    if (const int prc = finish_pending_assembly(c)) return prc;
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, "femshell_element_resultants: no mesh set");
    if (!out) return set_err(FEMSHELL_ERR_INVALID, "femshell_element_resultants: null argument");
    if (c->dyn.active) return set_err(FEMSHELL_ERR_INVALID, "femshell_element_resultants: dynamics is active (resultants of a Newmark state are an open end)");
    if (!u && !c->have_solution) return set_err(FEMSHELL_ERR_INVALID, "femshell_element_resultants: no solve has run (pass u)");
    const Plan &p = c->plan;
    if (u && !all_finite(u, 6ll * p.n_nodes)) return set_err(FEMSHELL_ERR_INVALID, "femshell_element_resultants: non-finite entry in u");
    int rc = select_device(c);
    if (rc) return rc;
    const size_t ld = (size_t)p.n_local_nodes() * 6, ne = (size_t)p.n_ltri() + (size_t)p.n_lquad();
    if (ne == 0) return FEMSHELL_OK;
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
    FS_HIP(res.alloc(ne * 14));
    ThermalView tv; // (temperatures in force: the thermal instantiations, N = t Dm (eps - eps0), M = -Dp (kappa - kappa0))
    launch_element_resultants(c->dm, c->mc, c->sections_or_null(), sec_t, ux, up, res.p, c->stream, thermal_view_or_null(c, &tv));
    FS_HIP(hipGetLastError());
    rc = check_status(c, "femshell_element_resultants");
    if (rc) return rc;
    // rows come back in the local element order; the caller's order on the host, after the copy (one contiguous copy, and the
    // kernel's stores stay whole lines)
    std::vector<double> local(ne * 14);
    FS_HIP(hipMemcpy(local.data(), res.p, ne * 14 * sizeof(double), hipMemcpyDeviceToHost));
    const size_t nt = (size_t)p.n_ltri();
    parallel_chunks((int64_t)ne, [&](int64_t b, int64_t e) {
        for (int64_t le = b; le < e; le++) {
            const size_t row = (size_t)le < nt ? (size_t)p.tri_global_id[(size_t)le] : (size_t)p.n_tri + (size_t)p.quad_global_id[(size_t)le - nt];
            std::memcpy(out + 14 * row, &local[14 * (size_t)le], 14 * sizeof(double));
        }
    }, 1 << 14);
    return FEMSHELL_OK;
}

} // extern "C"
