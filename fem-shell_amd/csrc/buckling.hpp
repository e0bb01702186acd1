// buckling.hpp -- linear buckling (femshell_buckling): the driver of the block inverse iteration (buckling.cpp).
// Blocks of vectors are stored as in modal.hpp: column j at X + j * ld, every column laid out like the vectors of the solve.
#pragma once

#include <functional>
#include <memory>
#include <vector>

#include "kernels.hpp"

namespace femshell {

// The pencil (K + lambda K_G) x = 0 on the free dofs as A x = mu K x, A = -K_G, mu = 1 / lambda.  The solver works on the K in
// HBM and the coefficients of K_G and knows nothing of the context: the solve with K is a callback on one column.
struct BucklingProblem {
    DeviceMatrix dm;
    const int32_t *slice_elem_local = nullptr; // the slices' element lists as local element indices (HBM)
    const double *coeff = nullptr;             // g_ab of every local element (HBM, launch_geometric_coeff)
    const int32_t *node_ids = nullptr;         // caller's id of every owned row (HBM), or nullptr
    int64_t ld = 0;
    int64_t total_slots = 0;
    hipStream_t stream = nullptr;
    // x = K^-1 b from zero to the relative residual rtol; *iters: the iterations it took
    std::function<int(const double *b, double *x, double rtol, int32_t *iters)> solve;
    int n_modes = 0, guard = 0, max_it = 0;
    double tol = 0.0, inner_rtol = 0.0;
};
struct BucklingResult {
    int iterations = 0, converged = 0, block = 0;
    int64_t inner_iterations = 0;
    double rho_max = 0.0;
    double seconds_solves = 0.0, seconds_products = 0.0, seconds_gram = 0.0, seconds_update = 0.0;
    std::vector<double> mu;    // n_modes values, descending in magnitude
    std::vector<double> rho;   // the convergence measure of every returned pair
    const double *X = nullptr; // HBM: the n_modes columns (leading dimension ld), K-orthonormal; valid until `work` is released
};
struct BucklingWork; // device buffers of a run
struct BucklingWorkDeleter {
    void operator()(BucklingWork *w) const;
};
// returns FEMSHELL_OK / _ERR_BREAKDOWN / _ERR_HIP; *work keeps the buffers result->X points into
int buckling_inverse_iteration(const BucklingProblem &p, BucklingResult *result, std::unique_ptr<BucklingWork, BucklingWorkDeleter> *work);

} // namespace femshell
