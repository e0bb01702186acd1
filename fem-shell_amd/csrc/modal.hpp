// modal.hpp -- modal analysis (femshell_modes): launchers of the block kernels (modal.hip) and the LOBPCG driver (modal.cpp).
//
// A BLOCK of vectors is stored column by column: column j starts at X + j * ld, ld = Plan::n_local_nodes() * 6 doubles, every
// column laid out like the vectors of the solve (owned rows | padding | ghost space; padding and ghost space zero, constrained
// dofs zero).  Every single-vector kernel of the library, the multigrid cycle included, therefore works on a column as it is.
#pragma once

#include <functional>
#include <memory>
#include <vector>

#include "kernels.hpp"

namespace femshell {

constexpr int kModalMaxCols = 96; // columns of a Gram operand: 3 (n_modes + guard) of the Rayleigh-Ritz basis [X P W]
constexpr int kModalMaxBlock = 32; // n_modes + guard
constexpr int kGramGrid = 128;    // workgroups (= partial Gram matrices) of launch_gram
constexpr int kSpmmMaxCols = 4;   // columns one pass of the fused block product multiplies

// ---- Y = K X, symmetric storage: every stored 6x6 block is read ONCE per pass and used for all columns of the pass -- as K_ac
// for the lane's own row and as K_ac^T for row c (k_spmv_sym's mapping: a wave per slice pair, a lane per node row).  A block of
// n_cols columns runs ceil(n_cols / 4) passes of 4 columns and a narrower one for the tail.  tbuf: kSpmmMaxCols planes of
// `plane` = total_slots * 6 doubles for the transposed products that leave their slice (those that stay go through LDS).
// Per column the additions are those of k_spmv_sym + k_sym_gather_node in their order: column j of Y is bitwise launch_spmv's.
// Returns false, having launched nothing, when m is not in symmetric storage.
bool launch_spmm_sym(const DeviceMatrix &m, const double *X, double *Y, int64_t ld, int n_cols, double *tbuf, int64_t plane, hipStream_t st);
// columns one pass takes with this operator: 4 unless the in-slice products of four columns exceed the LDS of a workgroup
int spmm_pass_cols(const DeviceMatrix &m);

// ---- G = A^T diag(w) B (qa x qb, row-major; w == nullptr: A^T B) over the owned rows.  kGramGrid workgroups, each over one
// contiguous stretch of the rows, staged through LDS; partials[kGramGrid][qa * qb] are then added in index order: the same bits
// from run to run.  qa, qb <= kModalMaxCols.
void launch_gram(const DeviceMatrix &m, int qa, const double *A, int qb, const double *B, int64_t ld, const double *w, double *partials,
                 double *G, hipStream_t st);

// ---- Y = sum_k S_k C_k: up to three source blocks S_k (q_k columns, leading dimension ld) and coefficient matrices C_k in HBM
// (q_k x n_out, row-major with leading dimension ldc); Y (n_out columns) must not alias a source.  One pass: a lane holds two
// consecutive rows (16-byte accesses) and reads every source column once.  Rows [0, n_pad * 6).
struct CombineSources {
    const double *S[3] = {nullptr, nullptr, nullptr};
    const double *C[3] = {nullptr, nullptr, nullptr};
    int q[3] = {0, 0, 0};
};
void launch_block_combine(const DeviceMatrix &m, const CombineSources &src, int ldc, int n_out, double *Y, int64_t ld, hipStream_t st);

// ---- R_j = (KX)_j - theta_j m o X_j on the free dofs, 0 on the constrained ones, for the columns cols[0 .. n) (device array of
// column indices into KX / X / theta; R column i belongs to cols[i]); norms[i] = sum r^2 / m over the free dofs with m > 0, by
// kGramGrid partial sums added in index order.
void launch_block_residual(const DeviceMatrix &m, const double *KX, const double *X, const double *mass, const double *theta,
                           const int32_t *cols, int n, double *R, int64_t ld, double *partials, double *norms, hipStream_t st);

// ---- Z_j = D^-1 R_j (the 6x6 block-Jacobi inverse of m.minv), masked on the constrained dofs, n columns
void launch_block_bj(const DeviceMatrix &m, const double *R, double *Z, int64_t ld, int n, hipStream_t st);
// X_j = mask(X_j), n columns, in place (the multigrid cycle leaves what the identity rows of K give on constrained dofs)
void launch_block_mask(const DeviceMatrix &m, double *X, int64_t ld, int n, hipStream_t st);

// ---- start vectors: a splitmix64 hash of (caller's node id, dof, column) mapped to (-1, 1), 0 on constrained dofs and on the
// padding.  node_ids == nullptr: the internal numbering is the caller's.
void launch_modal_init(const DeviceMatrix &m, const int32_t *node_ids, int n_cols, double *X, int64_t ld, hipStream_t st);

// ---- the solver (modal.cpp).  Works on the operator in HBM (K + shift M; the caller put the shift there and prepared the
// preconditioner) and knows nothing of the context: the preconditioner is a callback z = T r on one column.
struct ModalProblem {
    DeviceMatrix dm;
    const double *mass = nullptr;     // n_pad x 6, the lumped mass (positive on every free dof)
    const int32_t *node_ids = nullptr; // caller's id of every owned row (HBM), or nullptr
    int64_t ld = 0;
    int64_t total_slots = 0;
    hipStream_t stream = nullptr;
    bool block_jacobi = true;         // W = D^-1 R by k_block_bj; else `precond` per column
    std::function<int(const double *r, double *z)> precond;
    int n_modes = 0, guard = 0, max_it = 0;
    double tol = 0.0, shift = 0.0;
};
struct ModalResult {
    int iterations = 0, converged = 0, block = 0, restarts = 0, fused_product = 0;
    double residual_max = 0.0;
    double seconds_product = 0.0, seconds_precond = 0.0, seconds_gram = 0.0, seconds_update = 0.0;
    std::vector<double> theta;    // n_modes values of lambda + shift, ascending
    std::vector<double> residual; // ||K x - lambda M x||_{M^-1} / (lambda + shift) per returned pair
    const double *X = nullptr;    // HBM: the n_modes columns (leading dimension ld), M-orthonormal; valid until `work` is released
};
struct ModalWork; // device buffers of a run
struct ModalWorkDeleter {
    void operator()(ModalWork *w) const;
};
// returns FEMSHELL_OK / _ERR_BREAKDOWN / _ERR_HIP; *work keeps the buffers result->X points into
int modal_lobpcg(const ModalProblem &p, ModalResult *result, std::unique_ptr<ModalWork, ModalWorkDeleter> *work);

// Y (n_cols columns) = K X with the context-free pieces: the fused kernel with symmetric storage, else column by column through
// launch_spmv.  *fused = 1 when k_spmm_sym ran.  tbuf: as for launch_spmm_sym (unused with full storage).
void block_product(const DeviceMatrix &m, const double *X, double *Y, int64_t ld, int n_cols, double *tbuf, int64_t plane, hipStream_t st,
                   int *fused);

} // namespace femshell
