// api_modal_probe.cpp -- femshell_modal_combine / _residual / _block_jacobi / _mask / _start: the block kernels of the eigen-solvers
// (modal.hip) that otherwise run only inside femshell_modes and femshell_buckling, one launch at a time, for tests (DESIGN section
// 8i).  Each entry point uploads its blocks in the caller's numbering into device buffers of its own, calls the production launcher
// of modal.hpp once and downloads: no arithmetic lives here, no production path runs through this file, and nothing the context
// keeps is written (the residual and block-Jacobi probes bring the lumped mass, K and its block-Jacobi inverse up to date, as
// femshell_modal_gram and femshell_modes do).  Every output buffer is filled with bytes that read as NaN before the launch, so a
// row the kernel does not write shows; `stray` counts the words of the rows behind the owned ones that are not +0.0.
#include "api_internal.hpp"
#include "modal.hpp"

#include <cstring>
#include <string>
#include <vector>

using namespace femshell;

namespace {

// what the five entry points refuse alike, as femshell_modal_gram does; the context is as it was when this returns an error
int probe_ready(femshell_ctx *c, const char *what)
{
    const std::string w(what);
    if (!c) return set_err(FEMSHELL_ERR_INVALID, w + ": null argument");
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, w + ": no mesh set");
    if (c->cfg.world_size != 1) return set_err(FEMSHELL_ERR_UNSUPPORTED, w + ": single-rank contexts only");
    return select_device(c);
}

// a buffer of n_cols columns whose every byte is 0xFF: a NaN wherever the kernel writes nothing
int nan_block(DevBuf<double> &b, size_t words, hipStream_t st)
{
    FS_HIP(b.alloc(words));
    FS_HIP(hipMemsetAsync(b.p, 0xFF, words * sizeof(double), st));
    return FEMSHELL_OK;
}

// the words of rows [6 n_own, ld) of n_cols columns at dev that are not +0.0 bit for bit, counted on the host from a copy
int count_stray(femshell_ctx *c, const double *dev, size_t ld, int32_t n_cols, int64_t *stray)
{
    const size_t own = (size_t)c->dm.n_own * 6;
    *stray = 0;
    if (ld <= own || n_cols <= 0) return FEMSHELL_OK;
    const size_t tail = ld - own;
    std::vector<uint64_t> h(tail * (size_t)n_cols);
    FS_HIP(hipMemcpy2DAsync(h.data(), tail * sizeof(double), dev + own, ld * sizeof(double), tail * sizeof(double), (size_t)n_cols,
                            hipMemcpyDeviceToHost, c->stream));
    FS_HIP(hipStreamSynchronize(c->stream));
    int64_t n = 0;
    for (uint64_t word : h) n += word != 0;
    *stray = n;
    return FEMSHELL_OK;
}

} // namespace

extern "C" {

int femshell_modal_combine(femshell_ctx *c, int32_t n_src, const int32_t *q, const double *const *S, const double *C, int32_t ldc,
                           int32_t n_out, double *Y, int64_t *stray)
{
    const char *what = "femshell_modal_combine";
    if (!c || !q || !S || !C || !Y || !stray) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_combine: null argument");
    if (n_src < 1 || n_src > 3) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_combine: n_src must be in 1 .. 3");
    int64_t q_all = 0;
    for (int k = 0; k < n_src; k++) {
        if (q[k] < 0 || q[k] > kModalMaxCols) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_combine: every q must be in 0 .. 96");
        if (q[k] > 0 && !S[k]) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_combine: a source with columns is null");
        q_all += q[k];
    }
    if (q_all == 0) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_combine: no source column");
    if (n_out < 1 || n_out > 64) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_combine: n_out must be in 1 .. 64");
    if (ldc < n_out) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_combine: ldc < n_out");
    int rc = probe_ready(c, what);
    if (rc) return rc;
    hipStream_t st = c->stream;
    const size_t ld = (size_t)c->plan.n_local_nodes() * 6;
    DevBuf<double> ds[3], dc, dy;
    std::vector<double> stage[3]; // (synchronised below)
    CombineSources src;
    FS_HIP(dc.alloc((size_t)q_all * (size_t)ldc));
    FS_HIP(hipMemcpyAsync(dc.p, C, (size_t)q_all * (size_t)ldc * sizeof(double), hipMemcpyHostToDevice, st));
    int64_t row = 0;
    for (int k = 0; k < n_src; k++) {
        src.q[k] = q[k];
        src.C[k] = dc.p + row * ldc; // the rows of source k follow those of source k - 1
        row += q[k];
        if (q[k] == 0) continue;
        FS_HIP(ds[k].alloc((size_t)q[k] * ld));
        if ((rc = upload_node_block(c, NodeOrder::caller, q[k], S[k], ds[k].p, ld, &stage[k]))) return rc;
        src.S[k] = ds[k].p;
    }
    if ((rc = nan_block(dy, (size_t)n_out * ld, st))) return rc;
    launch_block_combine(c->dm, src, ldc, n_out, dy.p, (int64_t)ld, st);
    FS_HIP(hipGetLastError());
    if ((rc = count_stray(c, dy.p, ld, n_out, stray))) return rc;
    return download_node_block(c, NodeOrder::caller, n_out, dy.p, ld, Y);
}

int femshell_modal_residual(femshell_ctx *c, int32_t mb, const double *KX, const double *X, const double *theta, int32_t n,
                            const int32_t *cols, double *R, double *norms, double *partials, int64_t *stray)
{
    const char *what = "femshell_modal_residual";
    if (!c || !KX || !X || !theta || !cols || !R || !norms || !stray) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_residual: null argument");
    if (mb < 1 || mb > kModalMaxCols) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_residual: mb must be in 1 .. 96");
    if (n < 1 || n > kModalMaxCols) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_residual: n must be in 1 .. 96");
    for (int i = 0; i < n; i++)
        if (cols[i] < 0 || cols[i] >= mb) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_residual: a column index outside 0 .. mb - 1");
    int rc = probe_ready(c, what);
    if (rc) return rc;
    if (!c->have_density) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_residual: no density set (femshell_set_density)");
    if ((rc = ensure(c, kMass))) return rc;
    hipStream_t st = c->stream;
    const size_t ld = (size_t)c->plan.n_local_nodes() * 6;
    DevBuf<double> dkx, dx, dth, dr, dpart, dnorms;
    DevBuf<int32_t> dcols;
    std::vector<double> stage_kx, stage_x; // (synchronised below)
    FS_HIP(dkx.alloc((size_t)mb * ld));
    FS_HIP(dx.alloc((size_t)mb * ld));
    if ((rc = upload_node_block(c, NodeOrder::caller, mb, KX, dkx.p, ld, &stage_kx))) return rc;
    if ((rc = upload_node_block(c, NodeOrder::caller, mb, X, dx.p, ld, &stage_x))) return rc;
    FS_HIP(dth.alloc((size_t)mb));
    FS_HIP(hipMemcpyAsync(dth.p, theta, (size_t)mb * sizeof(double), hipMemcpyHostToDevice, st));
    FS_HIP(dcols.alloc((size_t)n));
    FS_HIP(hipMemcpyAsync(dcols.p, cols, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if ((rc = nan_block(dr, (size_t)n * ld, st))) return rc;
    if ((rc = nan_block(dpart, (size_t)n * kGramGrid, st))) return rc;
    if ((rc = nan_block(dnorms, (size_t)n, st))) return rc;
    launch_block_residual(c->dm, dkx.p, dx.p, c->mass.p, dth.p, dcols.p, n, dr.p, (int64_t)ld, dpart.p, dnorms.p, st);
    FS_HIP(hipGetLastError());
    FS_HIP(hipMemcpyAsync(norms, dnorms.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (partials) FS_HIP(hipMemcpyAsync(partials, dpart.p, (size_t)n * kGramGrid * sizeof(double), hipMemcpyDeviceToHost, st));
    if ((rc = count_stray(c, dr.p, ld, n, stray))) return rc;
    return download_node_block(c, NodeOrder::caller, n, dr.p, ld, R);
}

int femshell_modal_block_jacobi(femshell_ctx *c, int32_t n, const double *R, double *Z, int64_t *stray)
{
    const char *what = "femshell_modal_block_jacobi";
    if (!c || !R || !Z || !stray) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_block_jacobi: null argument");
    if (n < 1 || n > kModalMaxCols) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_block_jacobi: n must be in 1 .. 96");
    int rc = probe_ready(c, what);
    if (rc) return rc;
    if (c->dyn.active) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_block_jacobi: not while dynamics is active (femshell_dynamics_end first)");
    if (const int prc = finish_pending_assembly(c)) return prc;
    if ((rc = ensure(c, kK | kJacobi))) return rc;
    hipStream_t st = c->stream;
    const size_t ld = (size_t)c->plan.n_local_nodes() * 6;
    DevBuf<double> dr, dz;
    std::vector<double> stage; // (synchronised below)
    FS_HIP(dr.alloc((size_t)n * ld));
    if ((rc = upload_node_block(c, NodeOrder::caller, n, R, dr.p, ld, &stage))) return rc;
    if ((rc = nan_block(dz, (size_t)n * ld, st))) return rc;
    launch_block_bj(c->dm, dr.p, dz.p, (int64_t)ld, n, st);
    FS_HIP(hipGetLastError());
    if ((rc = count_stray(c, dz.p, ld, n, stray))) return rc;
    return download_node_block(c, NodeOrder::caller, n, dz.p, ld, Z);
}

int femshell_modal_mask(femshell_ctx *c, int32_t n, double *X, int64_t *stray)
{
    const char *what = "femshell_modal_mask";
    if (!c || !X || !stray) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_mask: null argument");
    if (n < 1 || n > kModalMaxCols) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_mask: n must be in 1 .. 96");
    int rc = probe_ready(c, what);
    if (rc) return rc;
    hipStream_t st = c->stream;
    const size_t ld = (size_t)c->plan.n_local_nodes() * 6;
    DevBuf<double> dx; // (in and out: the upload is the fill)
    std::vector<double> stage; // (synchronised below)
    FS_HIP(dx.alloc((size_t)n * ld));
    if ((rc = upload_node_block(c, NodeOrder::caller, n, X, dx.p, ld, &stage))) return rc;
    launch_block_mask(c->dm, dx.p, (int64_t)ld, n, st);
    FS_HIP(hipGetLastError());
    if ((rc = count_stray(c, dx.p, ld, n, stray))) return rc;
    return download_node_block(c, NodeOrder::caller, n, dx.p, ld, X);
}

int femshell_modal_start(femshell_ctx *c, int32_t n_cols, double *X, int64_t *stray)
{
    const char *what = "femshell_modal_start";
    if (!c || !X || !stray) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_start: null argument");
    if (n_cols < 1 || n_cols > kModalMaxCols) return set_err(FEMSHELL_ERR_INVALID, "femshell_modal_start: n_cols must be in 1 .. 96");
    int rc = probe_ready(c, what);
    if (rc) return rc;
    hipStream_t st = c->stream;
    const size_t ld = (size_t)c->plan.n_local_nodes() * 6;
    DevBuf<double> dx;
    DevBuf<int32_t> node_ids; // the caller's id of every owned row, exactly as femshell_modes passes it
    if (!c->perm.empty()) {
        FS_HIP(node_ids.upload(c->perm, st));
        FS_HIP(hipStreamSynchronize(st));
    }
    if ((rc = nan_block(dx, (size_t)n_cols * ld, st))) return rc;
    launch_modal_init(c->dm, c->perm.empty() ? nullptr : node_ids.p, n_cols, dx.p, (int64_t)ld, st);
    FS_HIP(hipGetLastError());
    if ((rc = count_stray(c, dx.p, ld, n_cols, stray))) return rc;
    return download_node_block(c, NodeOrder::caller, n_cols, dx.p, ld, X);
}

} // extern "C"
