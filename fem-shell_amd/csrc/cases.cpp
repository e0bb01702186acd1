// cases.cpp -- the driver of the load cases (cases.hpp): classic preconditioned CG with block-Jacobi for several
// right-hand sides in lockstep.  The cases run in passes of spmm_pass_cols columns; per iteration and pass one block product, the
// vector kernels of cases.hip over all columns of the pass, and a scalar step per column that holds alpha, beta, the sums and the
// done flag in HBM.  The host reads the done flags at the cadence of the single solve (8, 16, 32, then every 64 iterations).
#include "cases.hpp"
#include "context.hpp"

#include <algorithm>

namespace femshell {

namespace {

// host side of the stopping test: DonePoll of cg_driver.cpp for the columns of a pass
struct PassPoll {
    int32_t next_check = 8, check_step = 8;
    // returns 1 when every column of the pass has finished, 0 to go on, < 0 on error
    int operator()(hipStream_t st, const CaseScalars *dev, int nb, int32_t it, int32_t max_it, CaseScalars *hs)
    {
        if (it + 1 != next_check || it + 1 >= max_it) return 0;
        FS_HIP(hipMemcpyAsync(hs, dev, (size_t)nb * sizeof *hs, hipMemcpyDeviceToHost, st));
        FS_HIP(hipStreamSynchronize(st));
        bool all = true;
        for (int j = 0; j < nb; j++) all = all && hs[j].done != 0;
        if (all) return 1;
        if (check_step < 64) check_step *= 2;
        next_check += check_step;
        return 0;
    }
};

} // namespace

int cases_lockstep_cg(const CasesProblem &p, CasesResult *result)
{
    const DeviceMatrix &m = p.dm;
    hipStream_t st = p.stream;
    const int64_t ld = p.ld;
    const int kb = spmm_pass_cols(m), G = cases_grid(m);
    result->passes = 0;
    result->fused_product = 0;
    result->cases.assign((size_t)p.n_cases, CaseScalars{});
    if (p.n_cases <= 0 || m.n_slices == 0) return FEMSHELL_OK;

    const int width = std::min(kb, p.n_cases);
    DevBuf<double> Z, P, Q, tbuf, partials;
    DevBuf<CaseScalars> scal;
    FS_HIP(Z.alloc((size_t)width * ld));
    FS_HIP(P.alloc((size_t)width * ld));
    FS_HIP(Q.alloc((size_t)width * ld));
    FS_HIP(P.zero(st)); // (ghost space: the product's input)
    FS_HIP(Q.zero(st));
    if (m.symmetric) FS_HIP(tbuf.alloc((size_t)kSpmmMaxCols * p.total_slots * 6));
    FS_HIP(partials.alloc((size_t)2 * kSpmmMaxCols * G));
    FS_HIP(scal.alloc((size_t)p.n_cases));
    FS_HIP(scal.zero(st));

    for (int j0 = 0; j0 < p.n_cases; j0 += kb) {
        const int nb = std::min(kb, p.n_cases - j0);
        double *X = p.X + (int64_t)j0 * ld, *R = p.R + (int64_t)j0 * ld;
        CaseScalars *s = scal.p + j0;
        launch_cases_init(m, nb, X, R, Z.p, P.p, ld, partials.p, st);
        launch_cases_scalar(nb, s, partials.p, G, CASES_PHASE_INIT, p.rtol, st);
        CaseScalars hs[kSpmmMaxCols];
        PassPoll poll;
        for (int32_t it = 0; it < p.max_it; it++) {
            int fused = 0;
            block_product(m, P.p, Q.p, ld, nb, tbuf.p, p.total_slots * 6, st, &fused);
            result->fused_product = fused;
            launch_cases_dot(m, nb, s, P.p, Q.p, ld, partials.p, st);
            launch_cases_scalar(nb, s, partials.p, G, CASES_PHASE_ALPHA, p.rtol, st);
            launch_cases_update(m, nb, s, P.p, Q.p, X, R, Z.p, ld, partials.p, st);
            launch_cases_scalar(nb, s, partials.p, G, CASES_PHASE_BETA, p.rtol, st);
            launch_cases_direction(m, nb, s, Z.p, P.p, ld, st);
            const int rc = poll(st, s, nb, it, p.max_it, hs);
            if (rc < 0) return rc;
            if (rc == 1) break;
        }
        FS_HIP(hipGetLastError());
        result->passes++;
    }
    FS_HIP(hipMemcpyAsync(result->cases.data(), scal.p, (size_t)p.n_cases * sizeof(CaseScalars), hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st)); // (the work vectors go out of scope)
    return FEMSHELL_OK;
}

} // namespace femshell
