// api_envelope.cpp -- femshell_combination_envelope: the stress envelope of every element over factored sums of load cases
// (kernels: envelope.hip).  Nothing is kept and nothing of the context changes: every buffer is the call's own.
#include "api_internal.hpp"

#include <cstring>
#include <string>
#include <vector>

using namespace femshell;

// k_case_resultants: ids of every element, coordinates once per node, with sections an index per element, with temperatures in
// the call 16 B per element; per case the displacements once per node (what the lanes gather of a node beyond its first use comes
// from the caches), the 8 B of its tau with temperatures, and 48 B written per element
static double bytes_case_resultants(const femshell_ctx *c, int n_cases, bool thermal)
{
    const Plan &p = c->plan;
    const double ne = (double)p.n_ltri() + p.n_lquad();
    return 12.0 * p.n_ltri() + 16.0 * p.n_lquad() + 24.0 * p.n_own + (c->have_sections ? 4.0 * ne : 0.0) + (thermal ? 16.0 * ne : 0.0) +
           n_cases * (48.0 * p.n_own + 48.0 * ne + (thermal ? 8.0 : 0.0));
}
// k_envelope: the table once per pass of kEnvCombosPerPass combinations, the factors once, 48 + 24 B written per element, with
// sections an index per element
static double bytes_envelope(const femshell_ctx *c, int n_cases, int n_combos)
{
    const Plan &p = c->plan;
    const double ne = (double)p.n_ltri() + p.n_lquad();
    const double passes = (double)((n_combos + kEnvCombosPerPass - 1) / kEnvCombosPerPass);
    return passes * n_cases * 48.0 * ne + 8.0 * n_combos * n_cases + (48.0 + 24.0) * ne + (c->have_sections ? 4.0 * ne : 0.0);
}

// `width` words of T per local element in `local` -> the caller's element order (triangles, then quadrilaterals)
template <class T> static void rows_to_caller(const Plan &p, const std::vector<T> &local, size_t ne, size_t width, T *out)
{
    const size_t nt = (size_t)p.n_ltri();
    parallel_chunks((int64_t)ne, [&](int64_t b, int64_t e) {
        for (int64_t le = b; le < e; le++) {
            const size_t row = (size_t)le < nt ? (size_t)p.tri_global_id[(size_t)le] : (size_t)p.n_tri + (size_t)p.quad_global_id[(size_t)le - nt];
            std::memcpy(out + width * row, &local[width * (size_t)le], width * sizeof(T));
        }
    }, 1 << 14);
}

extern "C" {

int femshell_combination_envelope(femshell_ctx *c, int32_t n_cases, const double *u, const double *case_thermal, int32_t n_combos,
                                  const double *factors, double *env_out, int32_t *gov_out, femshell_envelope_info *info)
{
    const std::string w("femshell_combination_envelope");
    if (!c) return set_err(FEMSHELL_ERR_INVALID, w + ": null context");
    if (c->cfg.world_size != 1)
        return set_err(FEMSHELL_ERR_UNSUPPORTED, w + ": single-rank contexts only (the ghost values of u would need a halo exchange)");
    if (const int prc = finish_pending_assembly(c)) return prc;
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, w + ": no mesh set");
    if (!u || !factors || !env_out) return set_err(FEMSHELL_ERR_INVALID, w + ": null argument");
    if (n_cases < 1 || n_cases > 32) return set_err(FEMSHELL_ERR_INVALID, w + ": n_cases must be in 1 .. 32");
    if (n_combos < 1 || n_combos > 256) return set_err(FEMSHELL_ERR_INVALID, w + ": n_combos must be in 1 .. 256");
    const Plan &p = c->plan;
    const size_t n6 = (size_t)p.n_nodes * 6;
    for (int32_t j = 0; j < n_cases; j++)
        if (!all_finite(u + (size_t)j * n6, (int64_t)n6)) return set_err(FEMSHELL_ERR_INVALID, w + ": non-finite entry in u of case " + std::to_string(j + 1));
    if (!all_finite(factors, (int64_t)n_combos * n_cases)) return set_err(FEMSHELL_ERR_INVALID, w + ": non-finite entry in factors");
    bool any_tau = false;
    if (case_thermal) {
        if (!all_finite(case_thermal, n_cases)) return set_err(FEMSHELL_ERR_INVALID, w + ": non-finite entry in case_thermal");
        for (int32_t j = 0; j < n_cases; j++) any_tau = any_tau || case_thermal[j] != 0.0;
    }
    if (any_tau && !c->have_thermal)
        return set_err(FEMSHELL_ERR_INVALID, w + ": a non-zero case_thermal, but no temperatures are in force (femshell_set_thermal)");
    if (c->dyn.active) return set_err(FEMSHELL_ERR_INVALID, w + ": dynamics is active (resultants of a Newmark state are an open end)");
    TraceRange trace("femshell_combination_envelope");
    int rc = select_device(c);
    if (rc) return rc;
    const size_t ld = (size_t)p.n_local_nodes() * 6, ne = (size_t)p.n_ltri() + (size_t)p.n_lquad();
    if (info) *info = femshell_envelope_info{0.0, 0.0, 0.0, 0.0};
    if (ne == 0) return FEMSHELL_OK;
    hipStream_t st = c->stream;

    DevBuf<double> U, table, thick, fac, tau, env;
    DevBuf<int32_t> gov;
    std::vector<double> stage;
    FS_HIP(U.alloc((size_t)n_cases * ld));
    rc = upload_node_block(c, NodeOrder::caller, n_cases, u, U.p, ld, &stage);
    if (rc) return rc;
    const double *sec_t = nullptr;
    rc = upload_section_thickness(c, &thick, &sec_t);
    if (rc) return rc;
    const std::vector<double> fac_host(factors, factors + (size_t)n_combos * n_cases);
    FS_HIP(fac.upload(fac_host, st));
    // the thermal instantiations run only where a case carries the temperatures: without, the call computes what a context
    // without temperatures computes
    ThermalView tv;
    const ThermalView *thermal = any_tau ? thermal_view_or_null(c, &tv) : nullptr;
    std::vector<double> tau_host;
    if (thermal) {
        tau_host.assign(case_thermal, case_thermal + n_cases);
        FS_HIP(tau.upload(tau_host, st));
    }
    FS_HIP(table.alloc((size_t)n_cases * 6 * ne));
    FS_HIP(env.alloc(ne * 6));
    FS_HIP(gov.alloc(ne * 6 + 2));

    hipEvent_t mid = nullptr;
    FS_HIP(hipEventCreate(&mid));
    struct EventGuard {
        hipEvent_t e;
        ~EventGuard() { (void)hipEventDestroy(e); }
    } guard{mid};
    FS_HIP(hipEventRecord(c->ev0, st));
    launch_case_resultants(c->dm, c->mc, c->sections_or_null(), thermal, U.p, (int64_t)ld, n_cases, tau.p, table.p, st);
    FS_HIP(hipEventRecord(mid, st));
    launch_envelope(c->dm, c->mc, c->ds.elem_section, sec_t, table.p, n_cases, fac.p, n_combos, env.p, gov.p, st);
    FS_HIP(hipEventRecord(c->ev1, st));
    FS_HIP(hipGetLastError());
    rc = check_status(c, "femshell_combination_envelope"); // (synchronises: the host copies may go)
    if (rc) return rc;

    std::vector<double> env_local(ne * 6);
    std::vector<int32_t> gov_local(gov_out ? ne * 6 : 0);
    FS_HIP(hipMemcpyAsync(env_local.data(), env.p, ne * 6 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (gov_out) FS_HIP(hipMemcpyAsync(gov_local.data(), gov.p, ne * 6 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st));
    rows_to_caller(p, env_local, ne, 6, env_out);
    if (gov_out) rows_to_caller(p, gov_local, ne, 6, gov_out);
    if (info) {
        float ms1 = 0.f, ms2 = 0.f;
        FS_HIP(hipEventElapsedTime(&ms1, c->ev0, mid));
        FS_HIP(hipEventElapsedTime(&ms2, mid, c->ev1));
        info->seconds_cases = 1e-3 * ms1;
        info->seconds_envelope = 1e-3 * ms2;
        info->bytes_cases = bytes_case_resultants(c, n_cases, thermal != nullptr);
        info->bytes_envelope = bytes_envelope(c, n_cases, n_combos);
    }
    return FEMSHELL_OK;
}

} // extern "C"
