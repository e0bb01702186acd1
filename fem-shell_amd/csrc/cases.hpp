// cases.hpp -- load cases (femshell_solve_cases): launchers of the lockstep kernels (cases.hip) and the driver
// (cases.cpp).  Several right-hand sides on one K run the classic block-Jacobi CG side by side: one block product per iteration
// for all columns of a pass (modal.hpp block_product), every column on a recurrence of its own -- its own alpha, beta and done
// flag.  This is not block CG: the iterates of a column are those it has when it runs alone.
//
// The vectors are blocks in the layout of modal.hpp: column j at X + j * ld, ld = Plan::n_local_nodes() * 6.
#pragma once

#include <vector>

#include "kernels.hpp"
#include "modal.hpp"

namespace femshell {

// Scalars of one column, resident in HBM (the CgScalars of a column; 64 bytes).  Written by the one workgroup of k_cases_scalar that
// owns the column, read by every other kernel as wave-uniform values.
struct CaseScalars {
    double rz;     // r.z of the current iterate
    double alpha;
    double beta;
    double rr;     // r.r
    double bb;     // b.b
    double tol2;   // rtol^2 * b.b (0: run max_it iterations)
    double pq;     // the last p.Kp
    int32_t done;  // 0 running, 1 converged, -1 breakdown (p.Kp <= 0): the column is frozen from then on
    int32_t iters; // iterations performed
};
static_assert(sizeof(CaseScalars) == 64, "one column's scalars are 64 bytes");

enum CasesPhase : int {
    CASES_PHASE_INIT = 1,  // sums (r.z, b.b) of the start: threshold, done at once where b = 0
    CASES_PHASE_ALPHA = 2, // sum p.Kp: alpha = r.z / p.Kp, or the breakdown
    CASES_PHASE_BETA = 3   // sums (r.z, r.r) behind the update: iteration count, stopping test, beta
};

constexpr int kCasesMax = 32; // cases of one femshell_solve_cases call

// workgroups of the lockstep kernels that write partial sums: node_grid of device_common.hpp (64 lanes = two slices, walked with
// SliceWalk; never more than slice_grid).  The partial sums of a pass lie column by column: sum q of column j, one double per
// workgroup, at partials + (2 j + q) * G -- 2 * kSpmmMaxCols * G doubles.
int cases_grid(const DeviceMatrix &m);

// All launchers: nb = 1 .. kSpmmMaxCols columns; s = the scalars of the pass's first column; a column with s[j].done != 0 is
// neither read nor written (its partial sums are not written either, and k_cases_scalar does not read them).
// start: x = 0, z = D^-1 r, p = z for r = the masked right-hand side already in R; sums (r.z, r.r)
void launch_cases_init(const DeviceMatrix &m, int nb, double *X, const double *R, double *Z, double *P, int64_t ld, double *partials,
                       hipStream_t st);
// sum p.q
void launch_cases_dot(const DeviceMatrix &m, int nb, const CaseScalars *s, const double *P, const double *Q, int64_t ld, double *partials,
                      hipStream_t st);
// x += alpha_j p, r -= alpha_j q, z = D^-1 r (every node's inverse block read once for all columns); sums (r.z, r.r)
void launch_cases_update(const DeviceMatrix &m, int nb, const CaseScalars *s, const double *P, const double *Q, double *X, double *R, double *Z,
                         int64_t ld, double *partials, hipStream_t st);
// p = z + beta_j p over the owned (padded) rows
void launch_cases_direction(const DeviceMatrix &m, int nb, const CaseScalars *s, const double *Z, double *P, int64_t ld, hipStream_t st);
// The scalar step: workgroup j adds the partial sums of column j -- every lane its contiguous stretch of ceil(G / 64) in index
// order, then one lane the 64 stretches in index order: plain index order while G <= 64 -- and takes the step of `phase` for that
// column.  No atomics, no hand-off between workgroups: a column needs its own sums only.
void launch_cases_scalar(int nb, CaseScalars *s, const double *partials, int G, CasesPhase phase, double rtol, hipStream_t st);

// ---- the driver (cases.cpp).  Knows nothing of the context: K and D^-1 through dm, the loads already masked in HBM.
struct CasesProblem {
    DeviceMatrix dm;
    int64_t ld = 0;
    int64_t total_slots = 0;
    hipStream_t stream = nullptr;
    int n_cases = 0;
    double rtol = 0.0;
    int32_t max_it = 0;
    double *R = nullptr; // n_cases columns: the masked loads on entry, the residuals on return
    double *X = nullptr; // n_cases columns: the solutions on return (ghost space untouched)
};
struct CasesResult {
    int passes = 0, fused_product = 0;
    std::vector<CaseScalars> cases; // the scalars every column ended with
};
// returns FEMSHELL_OK / _ERR_HIP; a breakdown is reported per column (done = -1), not as a status
int cases_lockstep_cg(const CasesProblem &p, CasesResult *result);

} // namespace femshell
