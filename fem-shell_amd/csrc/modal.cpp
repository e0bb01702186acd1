// modal.cpp -- LOBPCG for the lowest eigenpairs of A x = theta M x, A = K + shift M as it lies in HBM, M the lumped mass on the free
// dofs (femshell_modes; Knyazev 2001, basis handling after Duersch, Shao, Yang, Gu 2018).
//
// The basis of an iteration is S = [X P W], stored as ONE block of q = mb + np + nw columns with its image AS beside it:
//   X   mb = n_modes + guard Ritz vectors, M-orthonormal;
//   W   the preconditioned residuals of the ACTIVE columns (soft locking: a converged column leaves the active set and stays in
//       X), masked, M-orthogonalised against X twice and M-orthonormalised by Cholesky of their Gram matrix;
//   P   the previous search directions, made M-orthonormal and M-orthogonal to X in coefficient space when they are formed.
// Rayleigh-Ritz on S with S^T A S and S^T M S from the Gram kernel; the new X and P -- and A X, A P by the same rotation, so the
// only product with K per iteration is A W -- come by k_block_combine into the other of two basis buffers.  The small dense work
// is the host's (modal_dense.hpp): one synchronisation per Gram matrix, nothing spins on the device.  When the wanted pairs have
// converged by the recurrence, A X is recomputed from X, X is rotated once more and the residuals are evaluated again: the pairs
// returned passed the test with a product of their own.
#include "modal.hpp"
#include "modal_dense.hpp"

#include "context.hpp"
#include "trace.hpp"

#include <cmath>
#include <cstring>

namespace femshell {

struct ModalWork {
    DevBuf<double> S[2], AS[2]; // the basis and its image, 3 mb columns each
    DevBuf<double> Wa, Wb;      // residuals / raw and half-orthogonalised W, mb columns each
    DevBuf<double> tbuf;        // transposed products of the block product
    DevBuf<double> gram_partials, G, coef, theta, norms, res_partials;
    DevBuf<int32_t> cols;
};
void ModalWorkDeleter::operator()(ModalWork *w) const { delete w; }

namespace {

struct Solver {
    const ModalProblem &p;
    ModalWork &w;
    ModalResult &res;
    hipStream_t st;
    int mb;
    int64_t ld;
    std::vector<double> hG; // host landing place of a Gram matrix

    // device time of a phase: the host synchronises at the end of each anyway (Gram matrices and norms come back)
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

    int gram(int qa, const double *A, int qb, const double *B, bool weighted, double *out)
    {
        launch_gram(p.dm, qa, A, qb, B, ld, weighted ? p.mass : nullptr, w.gram_partials.p, w.G.p, st);
        FS_HIP(hipGetLastError());
        FS_HIP(hipMemcpyAsync(out, w.G.p, (size_t)qa * qb * sizeof(double), hipMemcpyDeviceToHost, st));
        FS_HIP(hipStreamSynchronize(st));
        return FEMSHELL_OK;
    }
    // the coefficient matrices of one combine, uploaded behind each other into w.coef (the stream orders the copy before the
    // kernel; the host buffer must outlive the copy: synchronised here, the matrices are a few KB)
    int upload_coef(const std::vector<double> &c)
    {
        FS_HIP(hipMemcpyAsync(w.coef.p, c.data(), c.size() * sizeof(double), hipMemcpyHostToDevice, st));
        FS_HIP(hipStreamSynchronize(st));
        return FEMSHELL_OK;
    }
    int product(const double *X, double *Y, int n)
    {
        Lap lap(*this, res.seconds_product, "femshell_modes product");
        block_product(p.dm, X, Y, ld, n, w.tbuf.p, p.total_slots * 6, st, &res.fused_product);
        FS_HIP(hipGetLastError());
        return FEMSHELL_OK;
    }
    static int breakdown(const char *what)
    {
        return set_err(FEMSHELL_ERR_BREAKDOWN, std::string("femshell_modes: ") + what +
                                                   " (K + shift M is not positive definite on the free dofs: an unconstrained shell needs shift > 0)");
    }

    // residuals of the columns `cols` of basis buffer b (R into w.Wb), their M^-1 norms squared into out
    int residuals(int b, const std::vector<double> &theta, const std::vector<int32_t> &cols, std::vector<double> *out)
    {
        Lap lap(*this, res.seconds_update, "femshell_modes residual");
        const int n = (int)cols.size();
        FS_HIP(hipMemcpyAsync(w.theta.p, theta.data(), (size_t)mb * sizeof(double), hipMemcpyHostToDevice, st));
        FS_HIP(hipMemcpyAsync(w.cols.p, cols.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        launch_block_residual(p.dm, w.AS[b].p, w.S[b].p, p.mass, w.theta.p, w.cols.p, n, w.Wb.p, ld, w.res_partials.p, w.norms.p, st);
        FS_HIP(hipGetLastError());
        out->assign((size_t)n, 0.0);
        FS_HIP(hipMemcpyAsync(out->data(), w.norms.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
        FS_HIP(hipStreamSynchronize(st));
        return FEMSHELL_OK;
    }

    // Rayleigh-Ritz on the mb columns X of buffer b alone: X and A X rotated into buffer b ^ 1, theta = the Ritz values
    int ritz_on_x(int b, std::vector<double> *theta)
    {
        std::vector<double> A((size_t)mb * mb), B((size_t)mb * mb), Z((size_t)mb * mb);
        {
            Lap lap(*this, res.seconds_gram, "femshell_modes gram");
            int rc = gram(mb, w.S[b].p, mb, w.AS[b].p, false, A.data());
            if (!rc) rc = gram(mb, w.S[b].p, mb, w.S[b].p, true, B.data());
            if (rc) return rc;
        }
        theta->assign((size_t)mb, 0.0);
        double cond = 0.0;
        const int e = dense::pencil_eigh(mb, A.data(), B.data(), theta->data(), Z.data(), &cond);
        if (e) return breakdown(e == 1 ? "the Gram matrix X^T M X of the block is not positive definite" : "the Ritz problem did not converge");
        for (double t : *theta)
            if (!(t > 0.0) || !std::isfinite(t)) return breakdown("a Ritz value x.(K + shift M)x is not positive");
        Lap lap(*this, res.seconds_update, "femshell_modes update");
        int rc = upload_coef(Z);
        if (rc) return rc;
        CombineSources src;
        src.S[0] = w.S[b].p;
        src.C[0] = w.coef.p;
        src.q[0] = mb;
        launch_block_combine(p.dm, src, mb, mb, w.S[b ^ 1].p, ld, st);
        src.S[0] = w.AS[b].p;
        launch_block_combine(p.dm, src, mb, mb, w.AS[b ^ 1].p, ld, st);
        FS_HIP(hipGetLastError());
        return FEMSHELL_OK;
    }

    int run()
    {
        const int n_modes = p.n_modes;
        const size_t col = (size_t)ld;
        for (int i = 0; i < 2; i++) {
            FS_HIP(w.S[i].alloc(3 * (size_t)mb * col));
            FS_HIP(w.AS[i].alloc(3 * (size_t)mb * col));
            FS_HIP(w.S[i].zero(st)); // (ghost space and the columns not written yet)
            FS_HIP(w.AS[i].zero(st));
        }
        FS_HIP(w.Wa.alloc((size_t)mb * col));
        FS_HIP(w.Wb.alloc((size_t)mb * col));
        FS_HIP(w.Wa.zero(st));
        FS_HIP(w.Wb.zero(st));
        if (p.dm.symmetric) FS_HIP(w.tbuf.alloc((size_t)kSpmmMaxCols * p.total_slots * 6));
        FS_HIP(w.gram_partials.alloc((size_t)kGramGrid * kModalMaxCols * kModalMaxCols));
        FS_HIP(w.G.alloc((size_t)kModalMaxCols * kModalMaxCols));
        FS_HIP(w.coef.alloc((size_t)kModalMaxCols * kModalMaxCols));
        FS_HIP(w.theta.alloc((size_t)mb));
        FS_HIP(w.norms.alloc((size_t)mb));
        FS_HIP(w.res_partials.alloc((size_t)mb * kGramGrid));
        FS_HIP(w.cols.alloc((size_t)mb));
        hG.resize((size_t)kModalMaxCols * kModalMaxCols);

        int cur = 0, np = 0, rc;
        std::vector<double> theta;
        // start: hashed vectors, their image, Rayleigh-Ritz on them
        launch_modal_init(p.dm, p.node_ids, mb, w.S[cur].p, ld, st);
        FS_HIP(hipGetLastError());
        if ((rc = product(w.S[cur].p, w.AS[cur].p, mb))) return rc;
        if ((rc = ritz_on_x(cur, &theta))) return rc;
        cur ^= 1;

        std::vector<uint8_t> conv((size_t)mb, 0);
        std::vector<double> relres((size_t)mb, 0.0), norms;
        std::vector<int32_t> all_cols((size_t)mb);
        for (int j = 0; j < mb; j++) all_cols[(size_t)j] = j;
        bool fresh = true; // A X of the current buffer is a product of its own (not a rotated one)
        int it = 0;
        auto test = [&]() {
            int lowest = 0;
            for (int j = 0; j < mb; j++) {
                relres[(size_t)j] = std::sqrt(norms[(size_t)j]) / theta[(size_t)j];
                conv[(size_t)j] = relres[(size_t)j] <= p.tol;
            }
            while (lowest < n_modes && conv[(size_t)lowest]) lowest++;
            return lowest;
        };
        for (;;) {
            // residuals of all columns with theta = the Ritz values (x_j^T M x_j = 1): ||r_j||_{M^-1} <= tol theta_j
            if ((rc = residuals(cur, theta, all_cols, &norms))) return rc;
            for (double v : norms)
                if (!std::isfinite(v)) return breakdown("a residual is not finite");
            int done = test();
            if (done == n_modes && !fresh) {
                // the verdict of the recurrence is checked with A X computed from X, after one more rotation of X alone
                if ((rc = product(w.S[cur].p, w.AS[cur].p, mb))) return rc;
                if ((rc = ritz_on_x(cur, &theta))) return rc;
                // P and A P move along unchanged
                if (np > 0) {
                    FS_HIP(hipMemcpyAsync(w.S[cur ^ 1].p + (size_t)mb * col, w.S[cur].p + (size_t)mb * col, (size_t)np * col * sizeof(double),
                                          hipMemcpyDeviceToDevice, st));
                    FS_HIP(hipMemcpyAsync(w.AS[cur ^ 1].p + (size_t)mb * col, w.AS[cur].p + (size_t)mb * col, (size_t)np * col * sizeof(double),
                                          hipMemcpyDeviceToDevice, st));
                }
                cur ^= 1;
                fresh = true;
                if ((rc = residuals(cur, theta, all_cols, &norms))) return rc;
                done = test();
            }
            if (done == n_modes || it >= p.max_it) break;
            it++;
            fresh = false;

            std::vector<int32_t> active;
            for (int j = 0; j < mb; j++)
                if (!conv[(size_t)j]) active.push_back(j);
            int nw = (int)active.size();
            double *X = w.S[cur].p, *AX = w.AS[cur].p;
            double *Pn = X + (size_t)mb * col, *Wn = X + (size_t)(mb + np) * col;
            // R of the active columns (again, compacted: w.Wb), W = T R
            if (nw < mb && (rc = residuals(cur, theta, active, &norms))) return rc;
            {
                Lap lap(*this, res.seconds_precond, "femshell_modes preconditioner");
                if (p.block_jacobi) {
                    launch_block_bj(p.dm, w.Wb.p, w.Wa.p, ld, nw, st);
                } else {
                    for (int j = 0; j < nw; j++) {
                        FS_HIP(hipMemsetAsync(w.Wa.p + (size_t)j * col, 0, col * sizeof(double), st));
                        if ((rc = p.precond(w.Wb.p + (size_t)j * col, w.Wa.p + (size_t)j * col))) return rc;
                    }
                    launch_block_mask(p.dm, w.Wa.p, ld, nw, st);
                }
                FS_HIP(hipGetLastError());
            }
            // W <- W - X (X^T M W), twice; then W <- W R^-1 with R^T R = W^T M W
            {
                double *from = w.Wa.p, *to = w.Wb.p;
                for (int pass = 0; pass < 2; pass++) {
                    {
                        Lap lap(*this, res.seconds_gram, "femshell_modes gram");
                        if ((rc = gram(mb, X, nw, from, true, hG.data()))) return rc;
                    }
                    Lap lap(*this, res.seconds_update, "femshell_modes update");
                    std::vector<double> c((size_t)(mb + nw) * nw, 0.0); // [-X^T M W ; I]
                    for (int i = 0; i < mb; i++)
                        for (int j = 0; j < nw; j++) {
                            if (!std::isfinite(hG[(size_t)i * nw + j])) return breakdown("the preconditioned residuals are not finite");
                            c[(size_t)i * nw + j] = -hG[(size_t)i * nw + j];
                        }
                    for (int j = 0; j < nw; j++) c[(size_t)(mb + j) * nw + j] = 1.0;
                    if ((rc = upload_coef(c))) return rc;
                    CombineSources src;
                    src.S[0] = X;
                    src.C[0] = w.coef.p;
                    src.q[0] = mb;
                    src.S[1] = from;
                    src.C[1] = w.coef.p + (size_t)mb * nw;
                    src.q[1] = nw;
                    launch_block_combine(p.dm, src, nw, nw, to, ld, st);
                    FS_HIP(hipGetLastError());
                    std::swap(from, to);
                }
                // (from == w.Wa again)
                {
                    Lap lap(*this, res.seconds_gram, "femshell_modes gram");
                    if ((rc = gram(nw, from, nw, from, true, hG.data()))) return rc;
                }
                std::vector<double> Gw(hG.begin(), hG.begin() + (size_t)nw * nw), d((size_t)nw), L((size_t)nw * nw), c((size_t)nw * nw, 0.0);
                bool ok = true;
                for (int i = 0; i < nw; i++) {
                    ok = ok && Gw[(size_t)i * nw + i] > 0.0 && std::isfinite(Gw[(size_t)i * nw + i]);
                    d[(size_t)i] = ok ? 1.0 / std::sqrt(Gw[(size_t)i * nw + i]) : 0.0;
                }
                if (ok) {
                    for (int i = 0; i < nw; i++)
                        for (int j = 0; j < nw; j++) Gw[(size_t)i * nw + j] = 0.5 * (hG[(size_t)i * nw + j] + hG[(size_t)j * nw + i]) * d[(size_t)i] * d[(size_t)j];
                    ok = dense::cholesky(nw, Gw.data(), L.data()) && dense::cholesky_condition(nw, L.data()) <= 1e12;
                }
                if (!ok) return breakdown("the preconditioned residuals are linearly dependent or not finite");
                // C = D L^-T
                for (int i = 0; i < nw; i++) c[(size_t)i * nw + i] = 1.0;
                dense::solve_lower_transposed(nw, L.data(), nw, c.data());
                for (int i = 0; i < nw; i++)
                    for (int j = 0; j < nw; j++) c[(size_t)i * nw + j] *= d[(size_t)i];
                Lap lap(*this, res.seconds_update, "femshell_modes update");
                if ((rc = upload_coef(c))) return rc;
                CombineSources src;
                src.S[0] = from;
                src.C[0] = w.coef.p;
                src.q[0] = nw;
                launch_block_combine(p.dm, src, nw, nw, Wn, ld, st);
                FS_HIP(hipGetLastError());
            }
            if ((rc = product(Wn, AX + (size_t)(mb + np) * col, nw))) return rc;

            // Rayleigh-Ritz on [X P W]; without P when the basis is too ill-conditioned (restart)
            int q = mb + np + nw;
            std::vector<double> A, B, Z, th;
            for (;;) { // (at most twice: the second round has no P)
                A.assign((size_t)q * q, 0.0);
                B.assign((size_t)q * q, 0.0);
                {
                    Lap lap(*this, res.seconds_gram, "femshell_modes gram");
                    if ((rc = gram(q, X, q, AX, false, A.data()))) return rc;
                    if ((rc = gram(q, X, q, X, true, B.data()))) return rc;
                }
                Z.assign((size_t)q * q, 0.0);
                th.assign((size_t)q, 0.0);
                double cond = 0.0;
                const int e = dense::pencil_eigh(q, A.data(), B.data(), th.data(), Z.data(), &cond);
                if (e == 0 && cond <= 1e12) break;
                if (np == 0) return breakdown(e == 2 ? "the Ritz problem did not converge" : "the basis [X W] is not M-independent");
                // drop P: W moves up behind X (its image too) and the Gram matrices are formed again
                res.restarts++;
                // (through the W buffers, free by now: source and destination may overlap)
                const size_t bytes = (size_t)nw * col * sizeof(double);
                FS_HIP(hipMemcpyAsync(w.Wa.p, Wn, bytes, hipMemcpyDeviceToDevice, st));
                FS_HIP(hipMemcpyAsync(Pn, w.Wa.p, bytes, hipMemcpyDeviceToDevice, st));
                FS_HIP(hipMemcpyAsync(w.Wb.p, AX + (size_t)(mb + np) * col, bytes, hipMemcpyDeviceToDevice, st));
                FS_HIP(hipMemcpyAsync(AX + (size_t)mb * col, w.Wb.p, bytes, hipMemcpyDeviceToDevice, st));
                np = 0;
                q = mb + nw;
            }
            for (int j = 0; j < mb; j++)
                if (!(th[(size_t)j] > 0.0) || !std::isfinite(th[(size_t)j])) return breakdown("a Ritz value x.(K + shift M)x is not positive");

            // coefficients of the new X (all mb columns) and of the new P (the active columns, without their X part), P made
            // M-orthogonal to the new X and M-orthonormal in coefficient space: with G = S^T M S, <a, b> = a^T G b
            const int n_out_p = nw;
            std::vector<double> Cx((size_t)q * mb), Cp((size_t)q * n_out_p, 0.0), Bsym((size_t)q * q);
            for (int i = 0; i < q; i++)
                for (int j = 0; j < q; j++) Bsym[(size_t)i * q + j] = 0.5 * (B[(size_t)i * q + j] + B[(size_t)j * q + i]);
            for (int i = 0; i < q; i++)
                for (int j = 0; j < mb; j++) Cx[(size_t)i * mb + j] = Z[(size_t)i * q + j];
            for (int i = mb; i < q; i++)
                for (int j = 0; j < n_out_p; j++) Cp[(size_t)i * n_out_p + j] = Z[(size_t)i * q + active[(size_t)j]];
            auto g_times = [&](const std::vector<double> &C, int nc) { // G C
                std::vector<double> out((size_t)q * nc, 0.0);
                for (int i = 0; i < q; i++)
                    for (int k = 0; k < q; k++) {
                        const double g = Bsym[(size_t)i * q + k];
                        for (int j = 0; j < nc; j++) out[(size_t)i * nc + j] += g * C[(size_t)k * nc + j];
                    }
                return out;
            };
            bool have_p = true;
            for (int pass = 0; pass < 2 && have_p; pass++) { // Cp -= Cx (Cx^T G Cp), twice
                const std::vector<double> GCp = g_times(Cp, n_out_p);
                std::vector<double> o((size_t)mb * n_out_p, 0.0);
                for (int k = 0; k < q; k++)
                    for (int i = 0; i < mb; i++)
                        for (int j = 0; j < n_out_p; j++) o[(size_t)i * n_out_p + j] += Cx[(size_t)k * mb + i] * GCp[(size_t)k * n_out_p + j];
                for (int k = 0; k < q; k++)
                    for (int i = 0; i < mb; i++)
                        for (int j = 0; j < n_out_p; j++) Cp[(size_t)k * n_out_p + j] -= Cx[(size_t)k * mb + i] * o[(size_t)i * n_out_p + j];
            }
            {
                const std::vector<double> GCp = g_times(Cp, n_out_p);
                std::vector<double> Gp((size_t)n_out_p * n_out_p, 0.0), d((size_t)n_out_p), L((size_t)n_out_p * n_out_p);
                for (int k = 0; k < q; k++)
                    for (int i = 0; i < n_out_p; i++)
                        for (int j = 0; j < n_out_p; j++) Gp[(size_t)i * n_out_p + j] += Cp[(size_t)k * n_out_p + i] * GCp[(size_t)k * n_out_p + j];
                for (int i = 0; i < n_out_p && have_p; i++) {
                    have_p = Gp[(size_t)i * n_out_p + i] > 0.0 && std::isfinite(Gp[(size_t)i * n_out_p + i]);
                    if (have_p) d[(size_t)i] = 1.0 / std::sqrt(Gp[(size_t)i * n_out_p + i]);
                }
                if (have_p) {
                    std::vector<double> Gs((size_t)n_out_p * n_out_p);
                    for (int i = 0; i < n_out_p; i++)
                        for (int j = 0; j < n_out_p; j++)
                            Gs[(size_t)i * n_out_p + j] = 0.5 * (Gp[(size_t)i * n_out_p + j] + Gp[(size_t)j * n_out_p + i]) * d[(size_t)i] * d[(size_t)j];
                    have_p = dense::cholesky(n_out_p, Gs.data(), L.data()) && dense::cholesky_condition(n_out_p, L.data()) <= 1e12;
                }
                if (have_p) {
                    // Cp <- Cp D L^-T: (Cp D) L^-T = (L^-1 (Cp D)^T)^T
                    std::vector<double> T((size_t)n_out_p * q);
                    for (int k = 0; k < q; k++)
                        for (int j = 0; j < n_out_p; j++) T[(size_t)j * q + k] = Cp[(size_t)k * n_out_p + j] * d[(size_t)j];
                    dense::solve_lower(n_out_p, L.data(), q, T.data());
                    for (int k = 0; k < q; k++)
                        for (int j = 0; j < n_out_p; j++) Cp[(size_t)k * n_out_p + j] = T[(size_t)j * q + k];
                } else {
                    res.restarts++; // the next iteration runs without P
                }
            }
            const int np_new = have_p ? n_out_p : 0, n_out = mb + np_new;
            {
                Lap lap(*this, res.seconds_update, "femshell_modes update");
                std::vector<double> C((size_t)q * n_out);
                for (int i = 0; i < q; i++) {
                    for (int j = 0; j < mb; j++) C[(size_t)i * n_out + j] = Cx[(size_t)i * mb + j];
                    for (int j = 0; j < np_new; j++) C[(size_t)i * n_out + mb + j] = Cp[(size_t)i * n_out_p + j];
                }
                if ((rc = upload_coef(C))) return rc;
                CombineSources src;
                src.S[0] = X;
                src.C[0] = w.coef.p;
                src.q[0] = q;
                launch_block_combine(p.dm, src, n_out, n_out, w.S[cur ^ 1].p, ld, st);
                src.S[0] = AX;
                launch_block_combine(p.dm, src, n_out, n_out, w.AS[cur ^ 1].p, ld, st);
                FS_HIP(hipGetLastError());
            }
            for (int j = 0; j < mb; j++) theta[(size_t)j] = th[(size_t)j];
            np = np_new;
            cur ^= 1;
        }
        res.iterations = it;
        res.block = mb;
        res.theta.assign(theta.begin(), theta.begin() + n_modes);
        res.residual.assign(relres.begin(), relres.begin() + n_modes);
        res.converged = 0;
        res.residual_max = 0.0;
        for (int j = 0; j < n_modes; j++) {
            res.converged += conv[(size_t)j] ? 1 : 0;
            res.residual_max = std::max(res.residual_max, relres[(size_t)j]);
        }
        res.X = w.S[cur].p;
        return FEMSHELL_OK;
    }
};

} // namespace

int modal_lobpcg(const ModalProblem &p, ModalResult *result, std::unique_ptr<ModalWork, ModalWorkDeleter> *work)
{
    work->reset(new ModalWork);
    *result = ModalResult();
    Solver s{p, **work, *result, p.stream, p.n_modes + p.guard, p.ld, {}};
    return s.run();
}

} // namespace femshell
