// api_elastic_support.cpp -- femshell_set_foundation / femshell_set_springs / femshell_support_stiffness / femshell_support_forces:
// element foundations and nodal springs (kernels: elastic_support.hip; the state behind them: api_state.cpp).
#include "api_internal.hpp"

#include <cmath>
#include <cstring>

using namespace femshell;

namespace femshell {

// per listed element 16 B of node ids, 4 B of element index and 16 B of moduli; coordinates once per node; 72 B written per row
// of the slices (padding rows included)
double bytes_elastic_support(const femshell_ctx *c)
{
    const Plan &p = c->plan;
    return (16.0 + 4.0 + 16.0) * (double)p.slice_elems.size() + 24.0 * ((double)p.n_own + p.n_ghost) + 72.0 * (double)c->dm.n_slices * kSliceNodes;
}

// femshell_time_kernel: k_support_rows back to back between the context's event pair, on hashed moduli, into a scratch table --
// nothing of the context changes but the map of the lists, which a mesh gets once anyway
int time_elastic_support(femshell_ctx *c, int32_t reps, double *mean_ms_out)
{
    const Plan &p = c->plan;
    hipStream_t st = c->stream;
    const size_t ne = (size_t)p.n_ltri() + (size_t)p.n_lquad();
    RawVec<double> rows(2 * ne);
    parallel_chunks((int64_t)rows.size(), [&](int64_t b, int64_t e) {
        for (int64_t q = b; q < e; q++) {
            uint64_t h = (uint64_t)q * 0x9E3779B97F4A7C15ull; // (a fixed hash of the word's index: values in [0, 2))
            h ^= h >> 29;
            h *= 0xBF58476D1CE4E5B9ull;
            h ^= h >> 32;
            rows[(size_t)q] = (double)(int64_t)(h >> 11) * (1.0 / 4503599627370496.0);
        }
    }, 1 << 18);
    DevBuf<double> ef, table;
    int rc = ensure_slice_elem_local(c);
    if (rc) return rc;
    FS_HIP(ef.upload(rows, st));
    FS_HIP(table.alloc((size_t)std::max(c->dm.n_slices * kSliceNodes, p.n_pad) * 9));
    FS_HIP(hipStreamSynchronize(st));
    FS_HIP(hipEventRecord(c->ev0, st));
    for (int32_t i = 0; i < reps; i++) launch_support_rows(c->dm, c->slice_elem_local.p, ef.p, nullptr, table.p, st);
    FS_HIP(hipEventRecord(c->ev1, st));
    FS_HIP(hipStreamSynchronize(st));
    FS_HIP(hipGetLastError());
    float ms = 0.f;
    FS_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *mean_ms_out = (double)ms / reps;
    return FEMSHELL_OK;
}

} // namespace femshell

namespace {

// every value finite and >= 0
bool all_stiffness(const double *x, int64_t n)
{
    std::atomic<int> bad{0};
    parallel_chunks(n, [&](int64_t b, int64_t e) {
        for (int64_t i = b; i < e; i++)
            if (!(std::isfinite(x[i]) && x[i] >= 0.0)) bad.store(1);
    }, 1 << 18);
    return bad.load() == 0;
}

} // namespace

extern "C" {

int femshell_set_foundation(femshell_ctx *c, const double *tri_k, const double *quad_k)
{
    if (!c) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_foundation: null context");
    if (const int prc = finish_pending_assembly(c)) return prc;
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_foundation: call femshell_set_mesh first");
    if (c->dyn.active) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_foundation: not while dynamics is active (femshell_dynamics_end first)");
    const Plan &p = c->plan;
    if (tri_k && p.n_tri > 0 && !all_stiffness(tri_k, 2ll * p.n_tri))
        return set_err(FEMSHELL_ERR_INVALID, "femshell_set_foundation: negative or non-finite modulus of a triangle");
    if (quad_k && p.n_quad > 0 && !all_stiffness(quad_k, 2ll * p.n_quad))
        return set_err(FEMSHELL_ERR_INVALID, "femshell_set_foundation: negative or non-finite modulus of a quadrilateral");
    int rc = select_device(c);
    if (rc) return rc;
    if (!tri_k && !quad_k) return foundation_clear(c);
    // the caller's rows in the local element order (triangles, then quadrilaterals; the ghost elements of a row-partitioned
    // context included: every rank has the full arrays): 16 bytes per local element go to HBM
    const size_t nt = (size_t)p.n_ltri(), ne = nt + (size_t)p.n_lquad();
    RawVec<double> rows(2 * ne);
    parallel_chunks((int64_t)ne, [&](int64_t b, int64_t e) {
        for (int64_t le = b; le < e; le++) {
            const bool tri = (size_t)le < nt;
            const double *src = tri ? tri_k : quad_k;
            if (src) std::memcpy(&rows[2 * (size_t)le], src + 2 * (size_t)(tri ? p.tri_global_id[(size_t)le] : p.quad_global_id[(size_t)le - nt]), 2 * sizeof(double));
            else std::memset(&rows[2 * (size_t)le], 0, 2 * sizeof(double));
        }
    }, 1 << 16);
    return foundation_apply(c, rows);
}

int femshell_set_springs(femshell_ctx *c, int32_t n, const int32_t *node_ids, const double *k6)
{
    if (!c || (n > 0 && !k6)) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_springs: null argument");
    if (const int prc = finish_pending_assembly(c)) return prc;
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_springs: call femshell_set_mesh first");
    if (c->dyn.active) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_springs: not while dynamics is active (femshell_dynamics_end first)");
    const Plan &p = c->plan;
    if (n < 0) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_springs: n < 0");
    if (n > 0 && !node_ids && n != p.n_nodes) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_springs: dense form needs n == n_nodes");
    if (n > 0 && !all_stiffness(k6, 6ll * n)) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_springs: negative or non-finite stiffness");
    // the owned rows of the rank in the internal numbering, zero on the padding rows
    RawVec<double> rows((size_t)p.n_pad * 6);
    std::fill(rows.begin(), rows.end(), 0.0);
    std::vector<uint8_t> seen(node_ids ? (size_t)p.n_nodes : 0, 0);
    for (int32_t i = 0; i < n; i++) {
        const int32_t a = internal_node(c, node_ids ? node_ids[i] : i);
        if (a < 0) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_springs: node id out of range");
        if (node_ids) {
            if (seen[(size_t)a]) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_springs: a node is listed twice");
            seen[(size_t)a] = 1;
        }
        if (a >= p.row_begin && a < p.row_begin + p.n_own) std::memcpy(&rows[6ull * (size_t)(a - p.row_begin)], k6 + 6ll * i, 6 * sizeof(double));
    }
    const int rc = select_device(c);
    if (rc) return rc;
    if (n == 0) return springs_clear(c);
    return springs_apply(c, rows);
}

int femshell_support_stiffness(femshell_ctx *c, double *out)
{
    if (!c || !out) return set_err(FEMSHELL_ERR_INVALID, "femshell_support_stiffness: null argument");
    if (const int prc = finish_pending_assembly(c)) return prc;
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, "femshell_support_stiffness: no mesh set");
    const Plan &p = c->plan;
    if (!c->have_supports()) { // (every rank of a row partition is in the same state: nothing to gather)
        std::memset(out, 0, (size_t)p.n_nodes * 9 * sizeof(double));
        return FEMSHELL_OK;
    }
    int rc = select_device(c);
    if (rc) return rc;
    // the nine words of a row as two node vectors, through the transfers every node vector takes (node_io.hpp)
    DevBuf<double> lo, hi;
    FS_HIP(lo.alloc((size_t)p.n_pad * 6));
    FS_HIP(hi.alloc((size_t)p.n_pad * 6));
    launch_support_words(c->dm, c->support.p, lo.p, hi.p, c->stream);
    FS_HIP(hipGetLastError());
    RawVec<double> hlo((size_t)p.n_nodes * 6), hhi((size_t)p.n_nodes * 6);
    rc = gather_node_vector(c, lo.p, hlo.data());
    if (rc) return rc;
    rc = gather_node_vector(c, hi.p, hhi.data());
    if (rc) return rc;
    parallel_chunks((int64_t)p.n_nodes, [&](int64_t b, int64_t e) {
        for (int64_t a = b; a < e; a++) {
            std::memcpy(out + 9 * a, &hlo[6 * (size_t)a], 6 * sizeof(double));
            std::memcpy(out + 9 * a + 6, &hhi[6 * (size_t)a], 3 * sizeof(double));
        }
    }, 1 << 16);
    return FEMSHELL_OK;
}

int femshell_support_forces(femshell_ctx *c, const double *u, double *f6_out)
{
    if (!c) return set_err(FEMSHELL_ERR_INVALID, "femshell_support_forces: null context");
    if (c->cfg.world_size != 1) return set_err(FEMSHELL_ERR_UNSUPPORTED, "femshell_support_forces: single-rank contexts only (like femshell_reactions)");
    if (!f6_out) return set_err(FEMSHELL_ERR_INVALID, "femshell_support_forces: null argument");
    if (const int prc = finish_pending_assembly(c)) return prc;
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, "femshell_support_forces: no mesh set");
    if (!u && !c->have_solution) return set_err(FEMSHELL_ERR_INVALID, "femshell_support_forces: no solve has run (pass u)");
    const Plan &p = c->plan;
    if (u && !all_finite(u, 6ll * p.n_nodes)) return set_err(FEMSHELL_ERR_INVALID, "femshell_support_forces: non-finite entry in u");
    if (!c->have_supports()) {
        std::memset(f6_out, 0, (size_t)p.n_nodes * 6 * sizeof(double));
        return FEMSHELL_OK;
    }
    int rc = select_device(c);
    if (rc) return rc;
    DevBuf<double> x, y;
    std::vector<double> stage; // (upload_node_block: lives until the download below has synchronised)
    FS_HIP(y.alloc((size_t)p.n_pad * 6));
    if (u) {
        const size_t ld = (size_t)p.n_local_nodes() * 6;
        FS_HIP(x.alloc(ld));
        rc = upload_node_block(c, NodeOrder::caller, 1, u, x.p, ld, &stage);
        if (rc) return rc;
    }
    const double *xp = nullptr;
    if (!u && c->have_prescribed) { // the solution in HBM is the homogeneous part: u_bar is added entry by entry
        rc = resolve_prescribed(c);
        if (rc) return rc;
        if (c->ubar_nonzero) xp = c->ubar.p;
    }
    launch_support_apply(c->dm, c->support.p, u ? x.p : c->x.p, xp, nullptr, -1.0, y.p, c->stream); // -K_sup u
    FS_HIP(hipGetLastError());
    return gather_node_vector(c, y.p, f6_out);
}

} // extern "C"
