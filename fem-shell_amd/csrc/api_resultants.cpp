// api_resultants.cpp -- femshell_element_resultants: what the shell carries, element by element (kernel: element_resultants.hip),
// and femshell_nodal_resultants: the same averaged to the nodes and the error indicator of the difference (nodal_recovery.hip).
#include "api_internal.hpp"
#include "modal.hpp" // launch_modal_init: the hashed vector of the timing hook

#include <cstring>
#include <string>
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

// What femshell_element_resultants and femshell_nodal_resultants share: the refusals (in this order, under the caller's name), u in
// HBM -- the caller's vector, or the last solution with its prescribed part resolved --, the thermal view, the section thickness,
// and the rows of k_element_resultants in *res, LOCAL element order, checked for degenerate elements.  *ne_out = 0: an empty mesh,
// nothing launched.
static int resultants_to_device(femshell_ctx *c, const double *u, bool have_out, const char *what, DevBuf<double> *res, size_t *ne_out)
{
    const std::string w(what);
    *ne_out = 0;
    if (c->cfg.world_size != 1)
        return set_err(FEMSHELL_ERR_UNSUPPORTED, w + ": single-rank contexts only (the ghost values of u would need a halo exchange)");
    if (const int prc = finish_pending_assembly(c)) return prc;
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, w + ": no mesh set");
    if (!have_out) return set_err(FEMSHELL_ERR_INVALID, w + ": null argument");
    if (c->dyn.active) return set_err(FEMSHELL_ERR_INVALID, w + ": dynamics is active (resultants of a Newmark state are an open end)");
    if (!u && !c->have_solution) return set_err(FEMSHELL_ERR_INVALID, w + ": no solve has run (pass u)");
    const Plan &p = c->plan;
    if (u && !all_finite(u, 6ll * p.n_nodes)) return set_err(FEMSHELL_ERR_INVALID, w + ": non-finite entry in u");
    int rc = select_device(c);
    if (rc) return rc;
    const size_t ld = (size_t)p.n_local_nodes() * 6, ne = (size_t)p.n_ltri() + (size_t)p.n_lquad();
    if (ne == 0) return FEMSHELL_OK;
    DevBuf<double> x, thick;
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
    FS_HIP(res->alloc(ne * 14));
    ThermalView tv; // (temperatures in force: the thermal instantiations, N = t Dm (eps - eps0), M = -Dp (kappa - kappa0))
    launch_element_resultants(c->dm, c->mc, c->sections_or_null(), sec_t, ux, up, res->p, c->stream, thermal_view_or_null(c, &tv));
    FS_HIP(hipGetLastError());
    rc = check_status(c, what); // (synchronises: x, thick and stage may go)
    if (rc) return rc;
    *ne_out = ne;
    return FEMSHELL_OK;
}

// `width` doubles per local element at `src` in HBM -> the caller's element order on the host, after one contiguous copy (the
// kernels' stores stay whole lines)
static int download_element_rows(femshell_ctx *c, const double *src, size_t ne, size_t width, double *out)
{
    const Plan &p = c->plan;
    std::vector<double> local(ne * width);
    FS_HIP(hipMemcpyAsync(local.data(), src, ne * width * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    FS_HIP(hipStreamSynchronize(c->stream));
    const size_t nt = (size_t)p.n_ltri();
    parallel_chunks((int64_t)ne, [&](int64_t b, int64_t e) {
        for (int64_t le = b; le < e; le++) {
            const size_t row = (size_t)le < nt ? (size_t)p.tri_global_id[(size_t)le] : (size_t)p.n_tri + (size_t)p.quad_global_id[(size_t)le - nt];
            std::memcpy(out + width * row, &local[width * (size_t)le], width * sizeof(double));
        }
    }, 1 << 14);
    return FEMSHELL_OK;
}

// (1 / (E t), 12 / (E t^3), nu) of the uniform material, and of every section in HBM where the context has sections (uploaded per
// call, as the section thickness is: nothing is cached)
static RecoveryMat recovery_mat(double nu, double E, double t)
{
    RecoveryMat r;
    r.cn = 1.0 / (E * t);
    r.cm = 12.0 / (E * t * t * t);
    r.nu = nu;
    r.pad = 0.0;
    return r;
}
static int upload_recovery_sections(femshell_ctx *c, std::vector<RecoveryMat> *host, DevBuf<RecoveryMat> *buf, const RecoveryMat **sec_mat)
{
    *sec_mat = nullptr;
    if (!c->have_sections) return FEMSHELL_OK;
    host->resize((size_t)c->n_sections);
    for (size_t s = 0; s < host->size(); s++) (*host)[s] = recovery_mat(c->sec_nu[s], c->sec_E[s], c->sec_thickness[s]);
    FS_HIP(buf->upload(*host, c->stream)); // (the caller keeps *host until the stream is through)
    *sec_mat = buf->p;
    return FEMSHELL_OK;
}

namespace femshell {

// k_nodal_recovery: per listed element 16 B of node ids, 4 B of element index and the 96 B of its twelve tensor words; coordinates
// once per node; 112 B written per row of the slices
double bytes_nodal_recovery(const femshell_ctx *c)
{
    const Plan &p = c->plan;
    return (16.0 + 4.0 + 96.0) * (double)p.slice_elems.size() + 24.0 * ((double)p.n_own + p.n_ghost) + 112.0 * 32.0 * p.n_slices;
}
// k_recovery_error: per element its node ids, its twelve tensor words and 16 B written (4 B of a section index with sections);
// coordinates and the twelve recovered words once per node (what the lanes gather of a node beyond its first use comes from the
// caches)
double bytes_recovery_error(const femshell_ctx *c)
{
    const Plan &p = c->plan;
    const double ne = (double)p.n_ltri() + p.n_lquad();
    return 12.0 * p.n_ltri() + 16.0 * p.n_lquad() + (96.0 + 16.0) * ne + (24.0 + 96.0) * p.n_own + (c->have_sections ? 4.0 * ne : 0.0);
}

// femshell_time_kernel: element rows of a hashed displacement vector once, then the chosen kernel back to back between the context's
// event pair, into scratch buffers -- nothing of the context changes but the map of the lists, which a mesh gets once anyway
int time_recovery(femshell_ctx *c, bool error_kernel, int32_t reps, double *mean_ms_out)
{
    hipStream_t st = c->stream;
    const Plan &p = c->plan;
    const int64_t ld = (int64_t)p.n_local_nodes() * 6;
    const size_t ne = (size_t)p.n_ltri() + (size_t)p.n_lquad();
    DevBuf<double> S, R, thick, nodes, err;
    DevBuf<RecoveryMat> secbuf;
    std::vector<RecoveryMat> sec_host;
    FS_HIP(S.alloc((size_t)ld));
    FS_HIP(S.zero(st));
    FS_HIP(R.alloc(ne * 14));
    FS_HIP(nodes.alloc((size_t)p.n_slices * kSliceNodes * 14));
    FS_HIP(err.alloc(ne * 2));
    const double *sec_t = nullptr;
    const RecoveryMat *sec_mat = nullptr;
    int rc = upload_section_thickness(c, &thick, &sec_t);
    if (rc) return rc;
    rc = upload_recovery_sections(c, &sec_host, &secbuf, &sec_mat);
    if (rc) return rc;
    rc = ensure_slice_elem_local(c);
    if (rc) return rc;
    launch_modal_init(c->dm, nullptr, 1, S.p, ld, st);
    launch_element_resultants(c->dm, c->mc, c->sections_or_null(), sec_t, S.p, nullptr, R.p, st);
    launch_nodal_recovery(c->dm, c->slice_elem_local.p, R.p, nodes.p, st);
    FS_HIP(hipGetLastError());
    rc = check_status(c, "femshell_time_kernel");
    if (rc) return rc;
    const RecoveryMat mat = recovery_mat(c->cfg.nu, c->cfg.E, c->cfg.thickness);
    FS_HIP(hipEventRecord(c->ev0, st));
    for (int32_t i = 0; i < reps; i++) {
        if (error_kernel) launch_recovery_error(c->dm, mat, sec_mat, c->ds.elem_section, R.p, nodes.p, err.p, st);
        else launch_nodal_recovery(c->dm, c->slice_elem_local.p, R.p, nodes.p, st);
    }
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

int femshell_element_resultants(femshell_ctx *c, const double *u, double *out)
{
    if (!c) return set_err(FEMSHELL_ERR_INVALID, "femshell_element_resultants: null context");
    DevBuf<double> res;
    size_t ne = 0;
    const int rc = resultants_to_device(c, u, out != nullptr, "femshell_element_resultants", &res, &ne);
    if (rc || ne == 0) return rc;
    return download_element_rows(c, res.p, ne, 14, out);
}

int femshell_nodal_resultants(femshell_ctx *c, const double *u, double *nodes_out, double *elems_out)
{
    if (!c) return set_err(FEMSHELL_ERR_INVALID, "femshell_nodal_resultants: null context");
    DevBuf<double> res, nodes, err;
    DevBuf<RecoveryMat> secbuf;
    std::vector<RecoveryMat> sec_host;
    size_t ne = 0;
    int rc = resultants_to_device(c, u, nodes_out || elems_out, "femshell_nodal_resultants", &res, &ne);
    if (rc || ne == 0) return rc;
    const Plan &p = c->plan;
    rc = ensure_slice_elem_local(c);
    if (rc) return rc;
    FS_HIP(nodes.alloc((size_t)p.n_slices * kSliceNodes * 14));
    launch_nodal_recovery(c->dm, c->slice_elem_local.p, res.p, nodes.p, c->stream);
    if (elems_out) {
        const RecoveryMat *sec_mat = nullptr;
        rc = upload_recovery_sections(c, &sec_host, &secbuf, &sec_mat);
        if (rc) return rc;
        FS_HIP(err.alloc(ne * 2));
        launch_recovery_error(c->dm, recovery_mat(c->cfg.nu, c->cfg.E, c->cfg.thickness), sec_mat, c->ds.elem_section, res.p, nodes.p, err.p,
                              c->stream);
    }
    FS_HIP(hipGetLastError());
    if (nodes_out) { // node rows: one contiguous copy, then every row to the place of the caller's id of its node
        const size_t n = (size_t)p.n_own;
        const bool reorder = !c->perm.empty();
        std::vector<double> local(reorder ? n * 14 : 0);
        FS_HIP(hipMemcpyAsync(reorder ? local.data() : nodes_out, nodes.p, n * 14 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        FS_HIP(hipStreamSynchronize(c->stream));
        if (reorder)
            parallel_chunks((int64_t)n, [&](int64_t b, int64_t e) {
                for (int64_t i = b; i < e; i++)
                    std::memcpy(nodes_out + 14 * (size_t)caller_node(c, (int32_t)i), &local[14 * (size_t)i], 14 * sizeof(double));
            }, 1 << 14);
    }
    if (elems_out) {
        rc = download_element_rows(c, err.p, ne, 2, elems_out);
        if (rc) return rc;
    }
    FS_HIP(hipStreamSynchronize(c->stream)); // (sec_host and the buffers may go)
    return FEMSHELL_OK;
}

} // extern "C"
