// Stand-alone driver of csrc/modal_dense.hpp for tests/test_modal_cpu.py (built there with the host sanitizers).
// stdin: n, then A (n x n) and B (n x n) row-major as text.  stdout: status of pencil_eigh, theta[n], Z (n x n), then the status
// of cholesky(B) (1 = factored) and L (n x n), then the sweeps of jacobi_eigh(A), w[n], V (n x n); all in %.17g.
#include <cstdio>
#include <vector>

#include "modal_dense.hpp"

int main()
{
    int n = 0;
    if (std::scanf("%d", &n) != 1 || n < 1 || n > 96) return 2;
    std::vector<double> A((size_t)n * n), B((size_t)n * n);
    for (double &v : A)
        if (std::scanf("%lf", &v) != 1) return 2;
    for (double &v : B)
        if (std::scanf("%lf", &v) != 1) return 2;
    std::vector<double> theta((size_t)n), Z((size_t)n * n), L((size_t)n * n), w((size_t)n), V((size_t)n * n);
    double cond = 0.0;
    const int e = femshell::dense::pencil_eigh(n, A.data(), B.data(), theta.data(), Z.data(), &cond);
    std::printf("%d\n", e);
    for (double v : theta) std::printf("%.17g\n", v);
    for (double v : Z) std::printf("%.17g\n", v);
    std::printf("%d\n", femshell::dense::cholesky(n, B.data(), L.data()) ? 1 : 0);
    for (double v : L) std::printf("%.17g\n", v);
    std::vector<double> A2(A);
    std::printf("%d\n", femshell::dense::jacobi_eigh(n, A2.data(), w.data(), V.data()));
    for (double v : w) std::printf("%.17g\n", v);
    for (double v : V) std::printf("%.17g\n", v);
    return 0;
}
