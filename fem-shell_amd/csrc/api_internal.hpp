// api_internal.hpp -- what the files of the C ABI share: api.cpp (context, mesh and its data, assembly, solve, export, products),
// api_dynamics.cpp, api_modal.cpp, api_resultants.cpp, api_timing.cpp.  Not for the rest of the library.  Each function is described where it is
// defined: api.cpp, but for ensure_mass (api_dynamics.cpp), the byte models of the hot-path kernels (api_timing.cpp) and what
// api_resultants.cpp shares with the timing hook.
#pragma once

#include "amg_device.hpp"
#include "context.hpp"
#include "node_io.hpp"
#include "trace.hpp"

#pragma GCC visibility push(hidden)
namespace femshell {

int select_device(femshell_ctx *c);
double wall_s();
bool all_finite(const double *x, int64_t n);
int check_status(femshell_ctx *c, const char *what);
int finish_pending_assembly(femshell_ctx *c);
int do_assemble(femshell_ctx *c, bool wait = true);
int do_rhs(femshell_ctx *c);
int resolve_prescribed(femshell_ctx *c);
int do_jacobi(femshell_ctx *c);
int ensure_amg_hierarchy(femshell_ctx *c, double *pc_setup_s);
int solve_system(femshell_ctx *c, double rtol, int32_t max_it, double *u_out, femshell_solve_info *info, bool dynamic);
int ensure_mass(femshell_ctx *c);

double bytes_assemble(const femshell_ctx *c);
double bytes_spmv(const femshell_ctx *c);
double bytes_update(const femshell_ctx *c);
double bytes_direction(const femshell_ctx *c);
double bytes_update_single_reduction(const femshell_ctx *c);
double bytes_element_resultants(const femshell_ctx *c);
int upload_section_thickness(femshell_ctx *c, DevBuf<double> *buf, const double **sec_t);

} // namespace femshell
#pragma GCC visibility pop
