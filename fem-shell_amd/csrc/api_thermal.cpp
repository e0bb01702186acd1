// api_thermal.cpp -- femshell_set_expansion / femshell_set_thermal / femshell_thermal_load_vector: element temperatures and
// gradients through the thickness (kernel: element_thermal.hip; the state behind them: api_state.cpp).
#include "api_internal.hpp"

#include <cmath>
#include <cstring>

using namespace femshell;

namespace femshell {

// per listed element 16 B of node ids, 4 B of element index and 16 B of temperatures, with sections 4 B of section index (the
// rows of the section table come from the caches); coordinates once per node; per owned row 48 B of base read and 48 B written
// -- all six components carry a sum here, the rotational rows included
double bytes_element_thermal(const femshell_ctx *c)
{
    const Plan &p = c->plan;
    return (16.0 + 4.0 + 16.0 + (c->have_sections ? 4.0 : 0.0)) * (double)p.slice_elems.size() + 24.0 * ((double)p.n_own + p.n_ghost) + 96.0 * p.n_own;
}

// femshell_time_kernel: the kernel back to back between the context's event pair, on hashed temperatures and a unit alpha, from
// the loads in force into a scratch vector -- nothing of the context changes but the map of the lists, which a mesh gets once
int time_element_thermal(femshell_ctx *c, int32_t reps, double *mean_ms_out)
{
    const Plan &p = c->plan;
    hipStream_t st = c->stream;
    const size_t ne = (size_t)p.n_ltri() + (size_t)p.n_lquad();
    RawVec<double> rows(2 * ne);
    parallel_chunks((int64_t)rows.size(), [&](int64_t b, int64_t e) {
        for (int64_t q = b; q < e; q++) {
            uint64_t h = (uint64_t)q * 0x9E3779B97F4A7C15ull; // (a fixed hash of the word's index: values in [-1, 1))
            h ^= h >> 29;
            h *= 0xBF58476D1CE4E5B9ull;
            h ^= h >> 32;
            rows[(size_t)q] = (double)(int64_t)(h >> 11) * (1.0 / 4503599627370496.0) - 1.0;
        }
    }, 1 << 18);
    DevBuf<double> temp, out;
    DevBuf<ThermalSec> sec;
    int rc = ensure_slice_elem_local(c);
    if (rc) return rc;
    FS_HIP(temp.upload(rows, st));
    FS_HIP(out.alloc((size_t)p.n_pad * 6));
    ThermalView tv;
    tv.elem_temp = reinterpret_cast<const double2 *>(temp.p);
    tv.uni.nt = c->mc.t * c->mc.cm * (1.0 + c->mc.nu);
    tv.uni.mt = c->mc.cp * (1.0 + c->mc.nu) / c->mc.t;
    tv.uni.alpha = 1.0;
    tv.uni.alpha_t = 1.0 / c->mc.t;
    std::vector<ThermalSec> table;
    if (c->have_sections) {
        table.assign((size_t)c->n_sections, tv.uni);
        FS_HIP(sec.upload(table, st));
        tv.sec = sec.p;
    }
    FS_HIP(hipStreamSynchronize(st));
    FS_HIP(hipEventRecord(c->ev0, st));
    for (int32_t i = 0; i < reps; i++) launch_element_thermal(c->dm, c->slice_elem_local.p, c->ds.slice_elem_section, tv, c->loads.p, out.p, st);
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

int femshell_set_expansion(femshell_ctx *c, double alpha, int32_t n_sections, const double *section_alpha)
{
    if (!c) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_expansion: null context");
    if (const int prc = finish_pending_assembly(c)) return prc;
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_expansion: call femshell_set_mesh first");
    if (n_sections < 0) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_expansion: n_sections < 0");
    if (n_sections == 0) {
        if (!std::isfinite(alpha)) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_expansion: need a finite alpha");
    } else {
        if (!c->have_sections || n_sections != c->n_sections)
            return set_err(FEMSHELL_ERR_INVALID, "femshell_set_expansion: n_sections must be the context's section count (" +
                                                     std::to_string(c->have_sections ? c->n_sections : 0) + ")");
        if (!section_alpha) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_expansion: section_alpha is null");
        for (int32_t s = 0; s < n_sections; s++)
            if (!std::isfinite(section_alpha[s]))
                return set_err(FEMSHELL_ERR_INVALID, "femshell_set_expansion: section " + std::to_string(s) + ": need a finite alpha");
    }
    const int rc = select_device(c);
    if (rc) return rc;
    return expansion_apply(c, alpha, n_sections, section_alpha);
}

int femshell_set_thermal(femshell_ctx *c, const double *tri_temp, const double *quad_temp)
{
    if (!c) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_thermal: null context");
    if (const int prc = finish_pending_assembly(c)) return prc;
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_thermal: call femshell_set_mesh first");
    const Plan &p = c->plan;
    if (tri_temp && p.n_tri > 0 && !all_finite(tri_temp, 2ll * p.n_tri)) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_thermal: non-finite temperature of a triangle");
    if (quad_temp && p.n_quad > 0 && !all_finite(quad_temp, 2ll * p.n_quad)) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_thermal: non-finite temperature of a quadrilateral");
    int rc = select_device(c);
    if (rc) return rc;
    if (!tri_temp && !quad_temp) return thermal_clear(c);
    if (!c->have_alpha) return set_err(FEMSHELL_ERR_INVALID, "femshell_set_thermal: no expansion coefficient set (femshell_set_expansion)");
    // the caller's rows in the local element order (triangles, then quadrilaterals; the ghost elements of a row-partitioned
    // context included: every rank has the full arrays): 16 bytes per local element go to HBM
    const size_t nt = (size_t)p.n_ltri(), ne = nt + (size_t)p.n_lquad();
    RawVec<double> rows(2 * ne);
    parallel_chunks((int64_t)ne, [&](int64_t b, int64_t e) {
        for (int64_t le = b; le < e; le++) {
            const bool tri = (size_t)le < nt;
            const double *src = tri ? tri_temp : quad_temp;
            if (src) std::memcpy(&rows[2 * (size_t)le], src + 2 * (size_t)(tri ? p.tri_global_id[(size_t)le] : p.quad_global_id[(size_t)le - nt]), 2 * sizeof(double));
            else std::memset(&rows[2 * (size_t)le], 0, 2 * sizeof(double));
        }
    }, 1 << 16);
    return thermal_apply(c, rows);
}

int femshell_thermal_load_vector(femshell_ctx *c, double *f6_out)
{
    if (!c || !f6_out) return set_err(FEMSHELL_ERR_INVALID, "femshell_thermal_load_vector: null argument");
    if (const int prc = finish_pending_assembly(c)) return prc;
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, "femshell_thermal_load_vector: no mesh set");
    const Plan &p = c->plan;
    if (!c->have_thermal) { // (every rank of a row partition is in the same state: nothing to gather)
        std::memset(f6_out, 0, (size_t)p.n_nodes * 6 * sizeof(double));
        return FEMSHELL_OK;
    }
    const int rc = select_device(c);
    if (rc) return rc;
    DevBuf<double> T;
    FS_HIP(T.alloc((size_t)p.n_pad * 6));
    launch_element_thermal(c->dm, c->slice_elem_local.p, c->ds.slice_elem_section, thermal_view(c), nullptr, T.p, c->stream);
    FS_HIP(hipGetLastError());
    return gather_node_vector(c, T.p, f6_out);
}

} // extern "C"
