// derived.hpp -- what a femshell_ctx derives from its inputs, and which of it every kind of change makes stale (DESIGN
// section 8e).  Host only, plain C++17 without HIP, like knobs.hpp.  api_state.cpp applies the table (invalidate) and is the only
// file that writes the flags behind it; femshell_stale_after (plan_api.cpp) shows it to the tests.
#pragma once

#include <cstdint>

namespace femshell {

// One bit per derived product.  (kWarmStart: the one-shot start of the next solve; kFp64Only: the choice of an all-FP64
// hierarchy, made by a solve that broke down -- "stale" means forgotten for both.)
enum Derived : uint32_t {
    kK = 1u << 0,         // K in HBM (matrix_valid)
    kF = 1u << 1,         // F (rhs_valid)
    kJacobi = 1u << 2,    // the block-Jacobi inverse (jacobi_valid)
    kHierarchy = 1u << 3, // the multigrid hierarchy (c->amg)
    kMass = 1u << 4,      // the lumped mass (mass_valid)
    kUbar = 1u << 5,      // u_bar of the prescribed displacements (ubar_valid)
    kSolution = 1u << 6,  // the last solution (have_solution)
    kWarmStart = 1u << 7, // warm_next
    kFp64Only = 1u << 8,  // amg_fp64_only
    kEverything = (1u << 9) - 1,
};

// (the numbers are those of femshell_stale_after: new changes go at the end)
enum class Change : int32_t {
    mesh,                      // femshell_set_mesh, from the moment it touches the context: also when it is refused later
    dirichlet,                 // femshell_set_dirichlet
    sections,                  // femshell_set_sections: set, or cleared when some were set
    sections_cleared_none_set, // ... cleared when none were set: the densities are forgotten all the same
    loads,                     // femshell_set_loads, femshell_set_element_loads; femshell_set_thermal / femshell_set_expansion
                               // changed the temperatures in force, or they were forgotten: temperatures are loads
    prescribed,                // femshell_set_prescribed: set or cleared
    density,                   // femshell_set_density
    pc_options,                // femshell_set_preconditioner, unless only the refinement passes changed
    assembled,                 // K and F were just written (femshell_assemble, the timed assembly)
    matrix_shifted,            // K in HBM became K + s M and the caller knows it (a shifted femshell_modes)
    dynamics_begin,            // ... femshell_dynamics_begin: the same, and a pending warm start is dropped
    matrix_spoiled,            // HBM no longer holds what the flags say (leaving a shifted femshell_modes, the timed mass
                               // shift, a failed asynchronous assembly)
    dynamics_end,              // ... femshell_dynamics_end: the same, and a pending warm start is dropped
    fp64_fallback,             // a solve broke down under single-precision copies: the hierarchy again, all FP64
    krylov_probe,              // femshell_krylov_set / _launch wrote the vectors of the solve: x is no solution any more
    count
};

// The closure rule: whatever is computed from K is stale when K is.
constexpr uint32_t kWithK = kK | kF | kJacobi | kHierarchy;

constexpr uint32_t stale_after(Change what)
{
    switch (what) {
    case Change::mesh: return kEverything;
    case Change::dirichlet: return kWithK | kUbar;
    case Change::sections: return kWithK | kMass;
    case Change::sections_cleared_none_set: return kMass;
    case Change::loads: return kF;
    case Change::prescribed: return kF | kUbar;
    case Change::density: return kMass;
    case Change::pc_options: return kHierarchy | kFp64Only;
    case Change::assembled: return kJacobi | kHierarchy;
    case Change::matrix_shifted: return kJacobi | kHierarchy;
    case Change::dynamics_begin: return kJacobi | kHierarchy | kWarmStart;
    case Change::matrix_spoiled: return kWithK;
    case Change::dynamics_end: return kWithK | kWarmStart;
    case Change::fp64_fallback: return kHierarchy;
    case Change::krylov_probe: return kSolution;
    case Change::count: break;
    }
    return 0;
}

} // namespace femshell
