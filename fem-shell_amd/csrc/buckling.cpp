// buckling.cpp -- linear buckling: block inverse iteration with Rayleigh-Ritz on A x = mu K x, A = -K_G(N) on the free dofs,
// mu = 1 / lambda (femshell_buckling).  K_G is indefinite in general, K is positive definite: the pencil is
// symmetric-definite in the K inner product, its eigenvalues of largest magnitude are the load factors of smallest magnitude,
// and the subspace iteration X <- K^-1 A X converges to them whatever their signs.
//
// One iteration, with a block of mb = n_modes + guard columns:
//   Y = K^-1 (A X)          mb solves by the context's CG and preconditioner, from zero
//   KY = K Y, AY = A Y      the block product of the modal analysis and k_geometric_product
//   Y^T K Y, Y^T A Y        the Gram kernel; Cholesky and Jacobi on the host (modal_dense.hpp): one synchronisation per pair
//   X, AX, KX <- (Y, AY, KY) C, the Ritz pairs ordered by descending |mu|
// The convergence measure of pair j comes with the next iteration's solve z_j = K^-1 A x_j:
//   rho_j = ||A x_j - mu_j K x_j||_{K^-1} / (|mu_j| ||x_j||_K) = sqrt((z_j - mu_j x_j)^T (A x_j - mu_j K x_j)) / (|mu_j| sqrt(x_j^T K x_j)),
// the two difference vectors formed by k_block_combine (the expanded form would cancel to nothing at rho ~ 1e-8).  Some eigenvalue
// lies within rho_j |mu_j| of mu_j.  When the wanted pairs have passed by the rotated images, A X and K X are computed again from
// X and the test is repeated with a solve of its own: the pairs returned passed with products of their own.
#include "buckling.hpp"
#include "geometric_stiffness.hpp"
#include "modal.hpp"
#include "modal_dense.hpp"

#include "context.hpp"
#include "trace.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>

namespace femshell {

struct BucklingWork {
    DevBuf<double> X, AX, KX, Y, AY, KY, D, R; // mb columns each
    DevBuf<double> tbuf;                       // transposed products of the block product
    DevBuf<double> gram_partials, G, coef;
};
void BucklingWorkDeleter::operator()(BucklingWork *w) const { delete w; }

namespace {

struct Solver {
    const BucklingProblem &p;
    BucklingWork &w;
    BucklingResult &res;
    hipStream_t st;
    int mb;
    int64_t ld;

    struct Lap {
        Solver &s;
        double &acc;
        double t0;
        TraceRange range;
        Lap(Solver &s_, double &acc_, const char *name) : s(s_), acc(acc_), t0(now_s()), range(name) {}
        ~Lap()
        {
            (void)hipStreamSynchronize(s.st);
            acc += now_s() - t0;
        }
    };

    static int breakdown(const char *what) { return set_err(FEMSHELL_ERR_BREAKDOWN, std::string("femshell_buckling: ") + what); }

    int gram(const double *A, const double *B, std::vector<double> *out)
    {
        out->assign((size_t)mb * mb, 0.0);
        launch_gram(p.dm, mb, A, mb, B, ld, nullptr, w.gram_partials.p, w.G.p, st);
        FS_HIP(hipGetLastError());
        FS_HIP(hipMemcpyAsync(out->data(), w.G.p, (size_t)mb * mb * sizeof(double), hipMemcpyDeviceToHost, st));
        FS_HIP(hipStreamSynchronize(st));
        return FEMSHELL_OK;
    }
    int upload_coef(const std::vector<double> &c)
    {
        FS_HIP(hipMemcpyAsync(w.coef.p, c.data(), c.size() * sizeof(double), hipMemcpyHostToDevice, st));
        FS_HIP(hipStreamSynchronize(st)); // (the host matrix goes out of scope; a few KB)
        return FEMSHELL_OK;
    }
    // KV = K V and AV = -K_G V on the free dofs
    int products(const double *V, double *KV, double *AV)
    {
        Lap lap(*this, res.seconds_products, "femshell_buckling products");
        block_product(p.dm, V, KV, ld, mb, w.tbuf.p, p.total_slots * 6, st, nullptr);
        launch_geometric_product(p.dm, p.slice_elem_local, p.coeff, V, AV, ld, mb, true, st);
        FS_HIP(hipGetLastError());
        return FEMSHELL_OK;
    }
    int solves(const double *B, double *Xo)
    {
        Lap lap(*this, res.seconds_solves, "femshell_buckling solves");
        for (int j = 0; j < mb; j++) {
            int32_t it = 0;
            const int rc = p.solve(B + (size_t)j * ld, Xo + (size_t)j * ld, p.inner_rtol, &it);
            if (rc) return rc;
            res.inner_iterations += it;
        }
        launch_block_mask(p.dm, Xo, ld, mb, st); // (the multigrid cycle leaves what the identity rows of K give on constrained dofs)
        FS_HIP(hipGetLastError());
        return FEMSHELL_OK;
    }
    // Out = S0 + S1 diag(-mu): the difference vectors of the convergence measure
    int minus_mu(const double *S0, const double *S1, const std::vector<double> &mu, double *Out)
    {
        std::vector<double> c((size_t)2 * mb * mb, 0.0); // [I ; -diag mu]
        for (int j = 0; j < mb; j++) {
            c[(size_t)j * mb + j] = 1.0;
            c[(size_t)(mb + j) * mb + j] = -mu[(size_t)j];
        }
        int rc = upload_coef(c);
        if (rc) return rc;
        CombineSources src;
        src.S[0] = S0;
        src.C[0] = w.coef.p;
        src.q[0] = mb;
        src.S[1] = S1;
        src.C[1] = w.coef.p + (size_t)mb * mb;
        src.q[1] = mb;
        launch_block_combine(p.dm, src, mb, mb, Out, ld, st);
        FS_HIP(hipGetLastError());
        return FEMSHELL_OK;
    }

    int run()
    {
        const int n_modes = p.n_modes;
        const size_t col = (size_t)ld;
        for (DevBuf<double> *b : {&w.X, &w.AX, &w.KX, &w.Y, &w.AY, &w.KY, &w.D, &w.R}) {
            FS_HIP(b->alloc((size_t)mb * col));
            FS_HIP(b->zero(st)); // (ghost space)
        }
        if (p.dm.symmetric) FS_HIP(w.tbuf.alloc((size_t)kSpmmMaxCols * p.total_slots * 6));
        FS_HIP(w.gram_partials.alloc((size_t)kGramGrid * mb * mb));
        FS_HIP(w.G.alloc((size_t)mb * mb));
        FS_HIP(w.coef.alloc((size_t)2 * mb * mb));

        int rc;
        std::vector<double> mu((size_t)mb, 0.0), rho((size_t)mb, 0.0), G1, G2;
        launch_modal_init(p.dm, p.node_ids, mb, w.X.p, ld, st); // (zero on the constrained dofs and the padding)
        FS_HIP(hipGetLastError());
        if ((rc = products(w.X.p, w.KX.p, w.AX.p))) return rc;
        {
            Lap lap(*this, res.seconds_gram, "femshell_buckling gram");
            if ((rc = gram(w.AX.p, w.AX.p, &G1))) return rc;
        }
        bool any = false;
        for (int j = 0; j < mb; j++) {
            if (!std::isfinite(G1[(size_t)j * mb + j])) return breakdown("K_G X is not finite");
            any = any || G1[(size_t)j * mb + j] > 0.0;
        }
        if (!any) return breakdown("there is no prestress: the membrane forces of u are zero in every element, K_G = 0");

        bool have_mu = false, fresh = true; // fresh: A X and K X are products of their own (not rotated ones)
        int it = 0, done = 0;
        for (;;) {
            if ((rc = solves(w.AX.p, w.Y.p))) return rc; // Y = K^-1 A X: the next basis, and z of the convergence measure
            if (have_mu) {
                {
                    Lap lap(*this, res.seconds_update, "femshell_buckling update");
                    if ((rc = minus_mu(w.Y.p, w.X.p, mu, w.D.p))) return rc;   // z - mu x
                    if ((rc = minus_mu(w.AX.p, w.KX.p, mu, w.R.p))) return rc; // A x - mu K x
                }
                {
                    Lap lap(*this, res.seconds_gram, "femshell_buckling gram");
                    if ((rc = gram(w.D.p, w.R.p, &G1))) return rc;
                    if ((rc = gram(w.X.p, w.KX.p, &G2))) return rc;
                }
                done = 0;
                bool lowest = true;
                for (int j = 0; j < mb; j++) {
                    const double dr = G1[(size_t)j * mb + j], xkx = G2[(size_t)j * mb + j];
                    if (!std::isfinite(dr) || !std::isfinite(xkx) || !(xkx > 0.0)) return breakdown("the Gram matrices of the convergence test are not finite");
                    rho[(size_t)j] = std::sqrt(std::fabs(dr)) / (std::fabs(mu[(size_t)j]) * std::sqrt(xkx));
                    lowest = lowest && rho[(size_t)j] <= p.tol;
                    if (lowest && j < n_modes) done = j + 1;
                }
                if (done == n_modes && !fresh) {
                    // the verdict of the rotated images is checked with A X and K X computed from X, and a solve of its own
                    if ((rc = products(w.X.p, w.KX.p, w.AX.p))) return rc;
                    fresh = true;
                    continue;
                }
                if (done == n_modes || it >= p.max_it) break;
            }
            it++;
            if ((rc = products(w.Y.p, w.KY.p, w.AY.p))) return rc;
            {
                Lap lap(*this, res.seconds_gram, "femshell_buckling gram");
                if ((rc = gram(w.Y.p, w.KY.p, &G1))) return rc; // Y^T K Y
                if ((rc = gram(w.Y.p, w.AY.p, &G2))) return rc; // Y^T A Y
            }
            for (size_t i = 0; i < G1.size(); i++)
                if (!std::isfinite(G1[i]) || !std::isfinite(G2[i])) return breakdown("the Gram matrices Y^T K Y, Y^T A Y are not finite");
            std::vector<double> th((size_t)mb), Z((size_t)mb * mb);
            double cond = 0.0;
            const int e = dense::pencil_eigh(mb, G2.data(), G1.data(), th.data(), Z.data(), &cond);
            if (e == 1 || (e == 0 && !(cond <= 1e24)))
                return breakdown("Y^T K Y is not positive definite: K_G has too low a rank for a block of n_modes + guard columns (reduce them), or K is not positive definite on the free dofs");
            if (e) return breakdown("the Ritz problem did not converge");
            // descending |mu|, a positive one before a negative one of equal magnitude
            std::vector<int> order((size_t)mb);
            std::iota(order.begin(), order.end(), 0);
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
                const double fa = std::fabs(th[(size_t)a]), fb = std::fabs(th[(size_t)b]);
                return fa != fb ? fa > fb : th[(size_t)a] > th[(size_t)b];
            });
            // (magnitudes that agree to tol count as equal: the two members of a shear pair differ by rounding only)
            for (int j = 0; j + 1 < mb; j++) {
                const double a = th[(size_t)order[(size_t)j]], b = th[(size_t)order[(size_t)j + 1]];
                if (a < 0.0 && b > 0.0 && std::fabs(std::fabs(a) - std::fabs(b)) <= p.tol * std::fabs(a)) std::swap(order[(size_t)j], order[(size_t)j + 1]);
            }
            std::vector<double> C((size_t)mb * mb);
            for (int j = 0; j < mb; j++) {
                mu[(size_t)j] = th[(size_t)order[(size_t)j]];
                for (int i = 0; i < mb; i++) C[(size_t)i * mb + j] = Z[(size_t)i * mb + order[(size_t)j]];
            }
            for (int j = 0; j < n_modes; j++)
                if (mu[(size_t)j] == 0.0) return breakdown("a wanted Ritz value is zero: K_G has too low a rank for n_modes pairs");
            {
                Lap lap(*this, res.seconds_update, "femshell_buckling update");
                if ((rc = upload_coef(C))) return rc;
                CombineSources src;
                src.C[0] = w.coef.p;
                src.q[0] = mb;
                src.S[0] = w.Y.p;
                launch_block_combine(p.dm, src, mb, mb, w.X.p, ld, st);
                src.S[0] = w.AY.p;
                launch_block_combine(p.dm, src, mb, mb, w.AX.p, ld, st);
                src.S[0] = w.KY.p;
                launch_block_combine(p.dm, src, mb, mb, w.KX.p, ld, st);
                FS_HIP(hipGetLastError());
            }
            have_mu = true;
            fresh = false;
        }
        res.iterations = it;
        res.block = mb;
        res.mu.assign(mu.begin(), mu.begin() + n_modes);
        res.rho.assign(rho.begin(), rho.begin() + n_modes);
        res.converged = 0;
        res.rho_max = 0.0;
        for (int j = 0; j < n_modes; j++) {
            res.converged += rho[(size_t)j] <= p.tol ? 1 : 0;
            res.rho_max = std::max(res.rho_max, rho[(size_t)j]);
        }
        res.X = w.X.p;
        return FEMSHELL_OK;
    }
};

} // namespace

int buckling_inverse_iteration(const BucklingProblem &p, BucklingResult *result, std::unique_ptr<BucklingWork, BucklingWorkDeleter> *work)
{
    work->reset(new BucklingWork);
    *result = BucklingResult();
    Solver s{p, **work, *result, p.stream, p.n_modes + p.guard, p.ld};
    return s.run();
}

} // namespace femshell
