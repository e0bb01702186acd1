// api_element_loads.cpp -- femshell_set_element_loads / femshell_element_load_vector: pressure and traction per element (kernel:
// element_loads.hip; the state behind them: api_state.cpp).
#include "api_internal.hpp"

#include <cstring>

using namespace femshell;

namespace femshell {

// per listed element 16 B of node ids, 4 B of element index and 32 B of load words; coordinates once per node; per owned row
// 48 B of base read and 48 B written
double bytes_element_loads(const femshell_ctx *c)
{
    const Plan &p = c->plan;
    return (16.0 + 4.0 + 32.0) * (double)p.slice_elems.size() + 24.0 * ((double)p.n_own + p.n_ghost) + 96.0 * p.n_own;
}

// femshell_time_kernel: the kernel back to back between the context's event pair, on hashed element values, from the loads in
// force into a scratch vector -- nothing of the context changes but the map of the lists, which a mesh gets once anyway
int time_element_loads(femshell_ctx *c, int32_t reps, double *mean_ms_out)
{
    const Plan &p = c->plan;
    hipStream_t st = c->stream;
    const size_t ne = (size_t)p.n_ltri() + (size_t)p.n_lquad();
    RawVec<double> rows(4 * ne);
    parallel_chunks((int64_t)rows.size(), [&](int64_t b, int64_t e) {
        for (int64_t q = b; q < e; q++) {
            uint64_t h = (uint64_t)q * 0x9E3779B97F4A7C15ull; // (a fixed hash of the word's index: values in [-1, 1))
            h ^= h >> 29;
            h *= 0xBF58476D1CE4E5B9ull;
            h ^= h >> 32;
            rows[(size_t)q] = (double)(int64_t)(h >> 11) * (1.0 / 4503599627370496.0) - 1.0;
        }
    }, 1 << 18);
    DevBuf<double> el, out;
    int rc = ensure_slice_elem_local(c);
    if (rc) return rc;
    FS_HIP(el.upload(rows, st));
    FS_HIP(out.alloc((size_t)p.n_pad * 6));
    FS_HIP(hipStreamSynchronize(st));
    FS_HIP(hipEventRecord(c->ev0, st));
    for (int32_t i = 0; i < reps; i++) launch_element_loads(c->dm, c->slice_elem_local.p, el.p, c->loads.p, out.p, st);
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

int femshell_set_element_loads(femshell_ctx *c, const double *tri_load, const double *quad_load)
{
    if (!c) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_element_loads: null context");
    if (const int prc = finish_pending_assembly(c)) return prc;
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_element_loads: call femshell_set_mesh first");
    const Plan &p = c->plan;
    if (tri_load && p.n_tri > 0 && !all_finite(tri_load, 4ll * p.n_tri)) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_element_loads: non-finite load of a triangle");
    if (quad_load && p.n_quad > 0 && !all_finite(quad_load, 4ll * p.n_quad)) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_element_loads: non-finite load of a quadrilateral");
    int rc = select_device(c);
    if (rc) return rc;
    if (!tri_load && !quad_load) return element_loads_clear(c);
    // the caller's rows in the local element order (triangles, then quadrilaterals; the ghost elements of a row-partitioned
    // context included: every rank has the full arrays): 32 bytes per local element go to HBM
    const size_t nt = (size_t)p.n_ltri(), ne = nt + (size_t)p.n_lquad();
    RawVec<double> rows(4 * ne);
    parallel_chunks((int64_t)ne, [&](int64_t b, int64_t e) {
        for (int64_t le = b; le < e; le++) {
            const bool tri = (size_t)le < nt;
            const double *src = tri ? tri_load : quad_load;
            if (src) std::memcpy(&rows[4 * (size_t)le], src + 4 * (size_t)(tri ? p.tri_global_id[(size_t)le] : p.quad_global_id[(size_t)le - nt]), 4 * sizeof(double));
            else std::memset(&rows[4 * (size_t)le], 0, 4 * sizeof(double));
        }
    }, 1 << 16);
    return element_loads_apply(c, rows);
}

int femshell_element_load_vector(femshell_ctx *c, double *f6_out)
{
    if (!c || !f6_out) return set_err(FEMSHELL_ERR_INVALID, "femshell_element_load_vector: null argument");
    if (const int prc = finish_pending_assembly(c)) return prc;
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, "femshell_element_load_vector: no mesh set");
    const Plan &p = c->plan;
    if (!c->have_element_loads) { // (every rank of a row partition is in the same state: nothing to gather)
        std::memset(f6_out, 0, (size_t)p.n_nodes * 6 * sizeof(double));
        return FEMSHELL_OK;
    }
    const int rc = select_device(c);
    if (rc) return rc;
    DevBuf<double> S;
    FS_HIP(S.alloc((size_t)p.n_pad * 6));
    launch_element_loads(c->dm, c->slice_elem_local.p, c->elem_load.p, nullptr, S.p, c->stream);
    FS_HIP(hipGetLastError());
    return gather_node_vector(c, S.p, f6_out);
}

} // extern "C"
