// api_internal.hpp -- what the files of the C ABI share: api.cpp (context, mesh and its data, solve, export, products), api_state.cpp
// (what of the context's derived state is valid, and the functions that make it so), api_dynamics.cpp, api_modal.cpp,
// api_resultants.cpp, api_element_loads.cpp, api_thermal.cpp, api_elastic_support.cpp, api_cases.cpp, api_envelope.cpp, api_timing.cpp.  Not for the rest of the library.  Each function is described where it is defined: api.cpp, but
// for the block from invalidate to timed_assembly_done (api_state.cpp), the byte models of the hot-path kernels (api_timing.cpp)
// and what api_resultants.cpp shares with the timing hook.
#pragma once

#include "amg_device.hpp"
#include "context.hpp"
#include "derived.hpp"
#include "node_io.hpp"
#include "trace.hpp"

#pragma GCC visibility push(hidden)
namespace femshell {

int select_device(femshell_ctx *c);
double wall_s();
bool all_finite(const double *x, int64_t n);
int check_status(femshell_ctx *c, const char *what);
int check_and_agree(femshell_ctx *c, const char *what);
int agree_status(femshell_ctx *c, int local_rc, const char *what, bool neutral = false);
int solve_system(femshell_ctx *c, double rtol, int32_t max_it, double *u_out, femshell_solve_info *info, bool dynamic);
int solve_vector(femshell_ctx *c, const double *b, double *x, double rtol, int32_t max_it, int32_t *iters, int32_t *converged);

// seconds of what ensure() had to do (0: the product was there)
struct Timings {
    double assemble_s = 0.0, setup_s = 0.0, pc_setup_s = 0.0;
};
void invalidate(femshell_ctx *c, Change what);
// a mesh is set and every product (Derived bits) named is valid: for the entry points that refuse rather than rebuild
bool have(const femshell_ctx *c, uint32_t products);
// brings the products named in `need` up to date: the lumped mass, K (solving: again with FEMSHELL_REASSEMBLE_EACH_SOLVE), F,
// block-Jacobi, the multigrid hierarchy, in that order; adds the seconds of what it did to *t
int ensure(femshell_ctx *c, uint32_t need, Timings *t = nullptr, bool solving = false);
int finish_pending_assembly(femshell_ctx *c);
int do_assemble(femshell_ctx *c, bool wait = true);
int resolve_prescribed(femshell_ctx *c);
void forget_density(femshell_ctx *c);
int timed_assembly_done(femshell_ctx *c);
// element loads (api_state.cpp): c->loads holds nodal + S; uploads of the nodal part go to nodal_loads_buffer and end in combine_loads
void forget_element_loads(femshell_ctx *c);
int nodal_loads_buffer(femshell_ctx *c, double **buf);
int ensure_slice_elem_local(femshell_ctx *c);
int combine_loads(femshell_ctx *c);
int element_loads_apply(femshell_ctx *c, const RawVec<double> &rows);
int element_loads_clear(femshell_ctx *c);
// thermal loads (api_state.cpp): c->loads holds (nodal + S) + T; the same buffers and the same chain
void forget_thermal(femshell_ctx *c);
int thermal_forget_and_restore(femshell_ctx *c);
int expansion_apply(femshell_ctx *c, double alpha, int32_t n_sections, const double *section_alpha);
int thermal_apply(femshell_ctx *c, const RawVec<double> &rows);
int thermal_clear(femshell_ctx *c);
ThermalView thermal_view(const femshell_ctx *c);
const ThermalView *thermal_view_or_null(const femshell_ctx *c, ThermalView *store);
// elastic supports (api_state.cpp): c->support holds the table of the foundation and the springs in force; every assembly adds it
void forget_supports(femshell_ctx *c);
int foundation_apply(femshell_ctx *c, const RawVec<double> &rows);
int foundation_clear(femshell_ctx *c);
int springs_apply(femshell_ctx *c, const RawVec<double> &rows);
int springs_clear(femshell_ctx *c);

double bytes_assemble(const femshell_ctx *c);
double bytes_spmv(const femshell_ctx *c);
double bytes_update(const femshell_ctx *c);
double bytes_direction(const femshell_ctx *c);
double bytes_update_single_reduction(const femshell_ctx *c);
double bytes_element_resultants(const femshell_ctx *c);
double bytes_element_loads(const femshell_ctx *c);
int time_element_loads(femshell_ctx *c, int32_t reps, double *mean_ms_out);
double bytes_elastic_support(const femshell_ctx *c);
int time_elastic_support(femshell_ctx *c, int32_t reps, double *mean_ms_out);
double bytes_element_thermal(const femshell_ctx *c);
int time_element_thermal(femshell_ctx *c, int32_t reps, double *mean_ms_out);
double bytes_geometric_product(const femshell_ctx *c, int cols);
int time_geometric_product(femshell_ctx *c, int32_t reps, double *mean_ms_out);
int geometric_coefficients(femshell_ctx *c, const double *u, DevBuf<double> *coeff, const char *what);
int upload_section_thickness(femshell_ctx *c, DevBuf<double> *buf, const double **sec_t);
double bytes_nodal_recovery(const femshell_ctx *c);
double bytes_recovery_error(const femshell_ctx *c);
int time_recovery(femshell_ctx *c, bool error_kernel, int32_t reps, double *mean_ms_out);

} // namespace femshell
#pragma GCC visibility pop
