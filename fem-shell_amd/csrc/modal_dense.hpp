// modal_dense.hpp -- the small dense work of the modal solver (modal.cpp): Cholesky, a cyclic Jacobi eigensolver and the symmetric
// definite pencil A z = theta B z built from the two, for matrices of order <= 96.  Plain C++ on the host, no LAPACK, nothing of
// HIP: the header compiles on its own (tests/test_modal_cpu.py builds a stand-alone program around it, with the host sanitizers).
// All matrices are row-major, n x n with leading dimension n unless said otherwise.
#pragma once

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace femshell {
namespace dense {

// A = L L^T, L (lower triangle, row-major) written over a copy in `L`; the strict upper triangle of L is zeroed.
// false: a pivot was not positive (or not finite) -- A is not numerically positive definite.
inline bool cholesky(int n, const double *A, double *L)
{
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) L[i * n + j] = j <= i ? A[i * n + j] : 0.0;
    for (int j = 0; j < n; j++) {
        double d = L[j * n + j];
        for (int k = 0; k < j; k++) d -= L[j * n + k] * L[j * n + k];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        const double ljj = std::sqrt(d);
        L[j * n + j] = ljj;
        for (int i = j + 1; i < n; i++) {
            double s = L[i * n + j];
            for (int k = 0; k < j; k++) s -= L[i * n + k] * L[j * n + k];
            L[i * n + j] = s / ljj;
        }
    }
    return true;
}

// (max diag L / min diag L)^2: the cheap estimate of cond(A) the solver's restart rule uses (a lower bound of it)
inline double cholesky_condition(int n, const double *L)
{
    double lo = L[0], hi = L[0];
    for (int i = 1; i < n; i++) {
        lo = std::min(lo, L[i * n + i]);
        hi = std::max(hi, L[i * n + i]);
    }
    return (hi / lo) * (hi / lo);
}

// X <- L^-1 X for the n x m matrix X (row-major, leading dimension m)
inline void solve_lower(int n, const double *L, int m, double *X)
{
    for (int i = 0; i < n; i++) {
        for (int k = 0; k < i; k++) {
            const double l = L[i * n + k];
            for (int c = 0; c < m; c++) X[i * m + c] -= l * X[k * m + c];
        }
        const double inv = 1.0 / L[i * n + i];
        for (int c = 0; c < m; c++) X[i * m + c] *= inv;
    }
}

// X <- L^-T X
inline void solve_lower_transposed(int n, const double *L, int m, double *X)
{
    for (int i = n - 1; i >= 0; i--) {
        for (int k = i + 1; k < n; k++) {
            const double l = L[k * n + i];
            for (int c = 0; c < m; c++) X[i * m + c] -= l * X[k * m + c];
        }
        const double inv = 1.0 / L[i * n + i];
        for (int c = 0; c < m; c++) X[i * m + c] *= inv;
    }
}

// Eigenvalues (ascending, in w) and orthonormal eigenvectors (the COLUMNS of V) of the symmetric matrix A by cyclic Jacobi
// rotations; A is destroyed.  Sweeps are bounded (kMaxSweeps); returns the number of sweeps used, or -1 when the off-diagonal
// part did not fall below eps ||A||_F by then (non-finite input ends up here).
constexpr int kMaxSweeps = 60;
inline int jacobi_eigh(int n, double *A, double *w, double *V)
{
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) V[i * n + j] = i == j ? 1.0 : 0.0;
    int sweeps = -1;
    for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
        double off = 0.0, all = 0.0;
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) {
                all += A[i * n + j] * A[i * n + j];
                if (i != j) off += A[i * n + j] * A[i * n + j];
            }
        if (!std::isfinite(all)) return -1;
        if (off <= 1e-32 * all) { // ||off||_F <= 1e-16 ||A||_F
            sweeps = sweep;
            break;
        }
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                const double apq = A[p * n + q];
                if (apq == 0.0) continue;
                const double app = A[p * n + p], aqq = A[q * n + q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; k++) { // columns p, q
                    const double akp = A[k * n + p], akq = A[k * n + q];
                    A[k * n + p] = c * akp - s * akq;
                    A[k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; k++) { // rows p, q
                    const double apk = A[p * n + k], aqk = A[q * n + k];
                    A[p * n + k] = c * apk - s * aqk;
                    A[q * n + k] = s * apk + c * aqk;
                }
                A[p * n + q] = A[q * n + p] = 0.0;
                for (int k = 0; k < n; k++) {
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - s * vkq;
                    V[k * n + q] = s * vkp + c * vkq;
                }
            }
    }
    if (sweeps < 0) return -1;
    std::vector<int> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return A[a * n + a] < A[b * n + b]; });
    std::vector<double> Vs((size_t)n * n);
    for (int j = 0; j < n; j++) {
        w[j] = A[order[(size_t)j] * n + order[(size_t)j]];
        for (int i = 0; i < n; i++) Vs[(size_t)i * n + j] = V[i * n + order[(size_t)j]];
    }
    std::copy(Vs.begin(), Vs.end(), V);
    return sweeps;
}

// The pencil A z = theta B z with A symmetric, B symmetric positive definite: theta ascending, the columns of Z B-orthonormal
// (Z^T B Z = I, Z^T A Z = diag theta).  B is scaled to a unit diagonal first (D B D), factored by Cholesky, and the standard
// problem L^-1 D A D L^-T goes to jacobi_eigh.  *cond_out: cholesky_condition of the scaled B.
// Returns 0, 1 when B is not positive definite (Cholesky failed), 2 when the Jacobi sweeps did not converge.
inline int pencil_eigh(int n, const double *A, const double *B, double *theta, double *Z, double *cond_out)
{
    std::vector<double> d((size_t)n), Bs((size_t)n * n), L((size_t)n * n), As((size_t)n * n), V((size_t)n * n);
    for (int i = 0; i < n; i++) {
        if (!(B[i * n + i] > 0.0) || !std::isfinite(B[i * n + i])) return 1;
        d[(size_t)i] = 1.0 / std::sqrt(B[i * n + i]);
    }
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            // (both triangles from the mean: the Gram matrices come from sums in different orders)
            Bs[(size_t)i * n + j] = 0.5 * (B[i * n + j] + B[j * n + i]) * d[(size_t)i] * d[(size_t)j];
            As[(size_t)i * n + j] = 0.5 * (A[i * n + j] + A[j * n + i]) * d[(size_t)i] * d[(size_t)j];
        }
    if (!cholesky(n, Bs.data(), L.data())) return 1;
    if (cond_out) *cond_out = cholesky_condition(n, L.data());
    // As <- L^-1 As L^-T
    solve_lower(n, L.data(), n, As.data());
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++) std::swap(As[(size_t)i * n + j], As[(size_t)j * n + i]);
    solve_lower(n, L.data(), n, As.data());
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++) {
            const double m = 0.5 * (As[(size_t)i * n + j] + As[(size_t)j * n + i]);
            As[(size_t)i * n + j] = As[(size_t)j * n + i] = m;
        }
    if (jacobi_eigh(n, As.data(), theta, V.data()) < 0) return 2;
    // Z = D L^-T V
    solve_lower_transposed(n, L.data(), n, V.data());
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) Z[i * n + j] = d[(size_t)i] * V[(size_t)i * n + j];
    return 0;
}

} // namespace dense
} // namespace femshell
