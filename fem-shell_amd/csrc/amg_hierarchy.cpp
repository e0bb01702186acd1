// amg_hierarchy.cpp -- the hierarchy of the multigrid preconditioner (amg.hpp) into HBM, for one rank and for the replicated levels
// of a row partition (amg_dist.cpp): operator uploads, the clusters of the patch smoother, the power iteration, amg_setup and
// amg_finish_hierarchy step by step, and the block-Jacobi entry points of the tests.  The cycle that runs on it: amg_solve.cpp.
#include "amg_device.hpp"
#include "amg_pattern.hpp"
#include <thread>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

namespace femshell {

namespace {

bool has_lowp_copy(const AmgLevel &L) { return L.A32.p != nullptr; }

// FEMSHELL_AMG_VEC_F32: what a smoothing product on the single-precision copy of a level operator (symmetric storage) keeps
// in single precision besides the values -- 2 (default): its results (direct part, transposed products) and its input, the
// Chebyshev direction; 1: the results only; 0: nothing.  Residuals and iterates stay FP64.  Read per setup.
int smooth_vectors_f32()
{
    const int v = (int)knob_long("FEMSHELL_AMG_VEC_F32", 2);
    return v < 0 ? 0 : (v > 2 ? 2 : v);
}

constexpr const char *kLapPrefix = "[femshell amg setup]";

int upload_operator(AmgOperator &op, const SlicedEll &S, int32_t n_cols_pad, int64_t nnzb, hipStream_t st)
{
    FS_HIP(op.slice_width.upload(S.slice_width, st));
    FS_HIP(op.slice_base.upload(S.slice_base, st));
    FS_HIP(op.cols.upload(S.cols, st));
    FS_HIP(op.vals.upload(S.vals, st));
    FS_HIP(hipStreamSynchronize(st));
    op.nnzb = nnzb;
    op.n_cols_pad = n_cols_pad;
    op.dm = DeviceMatrix();
    op.dm.n_own = S.n_rows;
    op.dm.n_pad = S.n_pad;
    op.dm.n_slices = S.n_slices;
    op.dm.slice_width = op.slice_width.p;
    op.dm.slice_base = op.slice_base.p;
    op.dm.cols = op.cols.p;
    op.dm.vals = op.vals.p;
    op.dm.max_slice_width = S.max_width;
    return FEMSHELL_OK;
}

// the in-lists of op are in HBM: the buffer of the transposed products, and the lists into op.dm
int in_lists_attached(AmgOperator &op, int32_t max_in_width, int64_t total_slots, hipStream_t st)
{
    FS_HIP(op.tbuf.alloc((size_t)total_slots * 6));
    FS_HIP(op.tbuf.zero(st));
    FS_HIP(hipStreamSynchronize(st));
    op.dm.symmetric = 1;
    op.dm.max_in_width = max_in_width;
    op.dm.in_width = op.in_width.p;
    op.dm.in_base = op.in_base.p;
    op.dm.in_slots = op.in_slots.p;
    op.dm.in_rows = op.in_rows.p;
    op.dm.gat_slots = op.in_slots.p; // (level operators: every transposed product through tbuf)
    op.dm.tbuf = op.tbuf.p;
    return FEMSHELL_OK;
}

} // namespace

int attach_in_lists(AmgOperator &op, const SlicedEllSym &S, int64_t total_slots, hipStream_t st)
{
    FS_HIP(op.in_width.upload(S.in_width, st));
    FS_HIP(op.in_base.upload(S.in_base, st));
    FS_HIP(op.in_slots.upload(S.in_slots, st));
    FS_HIP(op.in_rows.upload(S.in_rows, st));
    return in_lists_attached(op, S.max_in_width, total_slots, st);
}

int attach_in_lists_device(AmgOperator &op, DevBuf<int32_t> &in_width, DevBuf<int64_t> &in_base, DevBuf<int32_t> &in_slots, DevBuf<int32_t> &in_rows,
                           int32_t max_in_width, int64_t total_slots, hipStream_t st)
{
    op.in_width.swap(in_width);
    op.in_base.swap(in_base);
    op.in_slots.swap(in_slots);
    op.in_rows.swap(in_rows);
    return in_lists_attached(op, max_in_width, total_slots, st);
}

namespace {

// a level operator from the host into HBM: diagonal and upper blocks with their in-lists, like K, or every block
int upload_level_operator(AmgOperator &op, const Bsr &A, bool symmetric, hipStream_t st)
{
    if (!symmetric) {
        SlicedEll S;
        pack_sliced_ell(A, true, &S);
        return upload_operator(op, S, S.n_pad, A.nnzb(), st);
    }
    SlicedEllSym S;
    pack_sliced_ell_sym(A, &S);
    const int rc = upload_operator(op, S, S.n_pad, (A.nnzb() + A.nr) / 2, st); // stored: diagonal + one block per pair
    return rc ? rc : attach_in_lists(op, S, S.slice_base.back(), st);
}

// FEMSHELL_AMG_PATCH_TAU (default 0.8; 0: no patch smoother) and FEMSHELL_AMG_PATCH_MAX (nodes per cluster, default 8): amg_patch.hpp
double patch_tau()
{
    const char *e = knob_text("FEMSHELL_AMG_PATCH_TAU"); // (read per setup: the tests switch it inside one process)
    return e && *e ? atof(e) : 0.8;
}
int patch_max_nodes()
{
    const char *e = knob_text("FEMSHELL_AMG_PATCH_MAX");
    const int m = e && *e ? atoi(e) : 8;
    return m < 2 ? 2 : (m > kPatchMaxNodes ? kPatchMaxNodes : m);
}

// When is a mesh one of poor element quality?  Edges above tau = 0.8 are ordinary on stretched structured elements (a third of the
// edges of the pinched cylinder's 3 : 1 cells reach 0.836, the coupled flap's 5 : 1 cells 0.965) where the point-block method works;
// what it does not cope with are NEARLY COINCIDENT nodes, sigma > 0.98: 2.6 % of the edges of the random-point shells, 0.13 % of a
// jittered-grid Delaunay shell (which converges in 90 iterations without cluster blocks), none of any structured mesh.  The
// clusters are built when more than FEMSHELL_AMG_PATCH_TRIGGER (default 0.01) of the pairs exceed 0.98; 0: whenever an edge exceeds tau.
double patch_trigger()
{
    const char *e = knob_text("FEMSHELL_AMG_PATCH_TRIGGER");
    return e && *e ? atof(e) : 0.01;
}
constexpr double kPatchTriggerSigma = 0.98;

} // namespace

// The clusters of rigidly coupled nodes of a level whose operator is in HBM (block-Jacobi inverse valid) and their smoother
// blocks M_c: detection on the device (k_patch_sigma), the union of the edges and the 36 x 36 inverses on the host.  A level
// without a rigid edge -- every structured mesh -- costs one kernel over its blocks and a four-byte copy, and keeps L.patches null.
int amg_build_patches(femshell_ctx *c, const DeviceMatrix &A, AmgLevel &L, bool collective, const std::vector<uint8_t> *excluded)
{
    L.patches.reset();
    const double tau = patch_tau();
    if (!(tau > 0.0) || A.n_own < 2 || A.minv == nullptr) return FEMSHELL_OK;
    hipStream_t st = c->stream;
    DevBuf<unsigned int> counter;
    DevBuf<PatchEdge> edges;
    FS_HIP(counter.alloc(4));
    unsigned int cap = (unsigned int)std::max<int64_t>(65536, A.n_own), found = 0;
    unsigned int counts[4] = {0, 0, 0, 0};
    for (int attempt = 0; attempt < 2; attempt++) {
        FS_HIP(edges.alloc(cap));
        FS_HIP(counter.zero(st));
        launch_patch_sigma(A, tau, kPatchTriggerSigma, edges.p, counter.p, cap, st);
        FS_HIP(hipGetLastError());
        FS_HIP(hipMemcpyAsync(counts, counter.p, sizeof counts, hipMemcpyDeviceToHost, st));
        FS_HIP(hipStreamSynchronize(st));
        found = counts[0];
        if (found <= cap) break;
        cap = found; // (more rigid edges than nodes: once more with room for all of them)
    }
    // the decision belongs to the whole mesh: the ranks of a row partition add their counts up
    double high = counts[1], pairs = counts[2];
    if (collective && c->comm.active()) {
        DevBuf<double> sums;
        FS_HIP(sums.alloc(2));
        const double mine[2] = {high, pairs};
        FS_HIP(hipMemcpyAsync(sums.p, mine, sizeof mine, hipMemcpyHostToDevice, st));
        std::string e;
        if (!comm_allreduce_sum(c->comm, sums.p, 2, st, &e)) return set_err(FEMSHELL_ERR_COMM, e);
        double all[2] = {0.0, 0.0};
        FS_HIP(hipMemcpyAsync(all, sums.p, sizeof all, hipMemcpyDeviceToHost, st));
        FS_HIP(hipStreamSynchronize(st));
        high = all[0];
        pairs = all[1];
    }
    if (setup_verbose())
        fprintf(stderr, "[femshell amg setup] patch smoother: %u of %.0f pairs above sigma %.2f (%.0f above %.2f: %s)\n", found, pairs, tau, high,
                kPatchTriggerSigma, high > patch_trigger() * pairs || (patch_trigger() <= 0.0 && found > 0) ? "a mesh of poor element quality" : "no clusters");
    if (patch_trigger() > 0.0 ? !(high > patch_trigger() * pairs) : found == 0) return FEMSHELL_OK;
    if (found == 0) return FEMSHELL_OK;
    std::vector<PatchEdge> h((size_t)found);
    FS_HIP(hipMemcpyAsync(h.data(), edges.p, h.size() * sizeof(PatchEdge), hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st));
    auto P = std::make_shared<AmgPatches>();
    P->tau = tau;
    P->max_nodes = patch_max_nodes();
    P->edges = found;
    P->n_clusters = patch_clusters(A.n_own, std::move(h), P->max_nodes, &P->label, &P->h_ptr, &P->h_nodes);
    if (P->n_clusters == 0) return FEMSHELL_OK;
    P->n_members = (int32_t)P->h_nodes.size();
    // Row-partitioned levels: a cluster that holds a node another rank reads (the nodes of the halo's send lists) smooths like the
    // others -- z_c += M_c r_c is local -- but stays out of the smoothing of P and of the gluing.  A cluster couples the row of P of
    // each of its members to the aggregates ALL its members see; were a member adjacent to another rank's nodes, a cluster-mate one
    // node further from the cut would get a block in a column of that rank -- a fine row the rank does not hold among its ghosts,
    // whose share of P^T A P it could not add (measured: "coarsest operator is not positive definite").
    P->label_p = P->label;
    std::vector<uint8_t> in_p; // (source of an upload: lives until the synchronisations below)
    if (excluded != nullptr && !excluded->empty()) {
        in_p.assign((size_t)P->n_clusters, 1);
        for (int32_t i = 0; i < A.n_own; i++)
            if (P->label[(size_t)i] >= 0 && (*excluded)[(size_t)i]) in_p[(size_t)P->label[(size_t)i]] = 0;
        for (int32_t i = 0; i < A.n_own; i++)
            if (P->label[(size_t)i] >= 0 && !in_p[(size_t)P->label[(size_t)i]]) P->label_p[(size_t)i] = -1;
        FS_HIP(P->in_p.upload(in_p, st));
    }
    std::vector<int64_t> moff((size_t)P->n_clusters);
    std::vector<int32_t> cluster_of((size_t)P->n_members);
    int64_t total = 0;
    for (int32_t k = 0; k < P->n_clusters; k++) {
        const int64_t m = P->h_ptr[(size_t)k + 1] - P->h_ptr[(size_t)k];
        moff[(size_t)k] = total;
        total += 36 * m * m;
        for (int32_t t = P->h_ptr[(size_t)k]; t < P->h_ptr[(size_t)k + 1]; t++) cluster_of[(size_t)t] = k;
    }
    FS_HIP(P->ptr.upload(P->h_ptr, st));
    FS_HIP(P->nodes.upload(P->h_nodes, st));
    FS_HIP(P->moff.upload(moff, st));
    FS_HIP(P->cluster_of.upload(cluster_of, st));
    FS_HIP(P->M.alloc((size_t)total));
    DevBuf<double> dinv;
    FS_HIP(dinv.alloc((size_t)P->n_members * 36));
    launch_patch_gather(A, P->view(), P->M.p, dinv.p, st);
    FS_HIP(hipGetLastError());
    std::vector<double> hB((size_t)total), hD((size_t)P->n_members * 36);
    FS_HIP(hipMemcpyAsync(hB.data(), P->M.p, hB.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    FS_HIP(hipMemcpyAsync(hD.data(), dinv.p, hD.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st));
    P->fell_back = patch_matrices(P->h_ptr, moff, hD.data(), hB.data());
    FS_HIP(hipMemcpyAsync(P->M.p, hB.data(), hB.size() * sizeof(double), hipMemcpyHostToDevice, st));
    FS_HIP(hipStreamSynchronize(st)); // (hB goes out of scope)
    if (setup_verbose())
        fprintf(stderr, "[femshell amg setup] patch smoother: %lld rigid edges (sigma > %.2f), %d clusters of %d nodes (at most %d each), %d not positive definite\n",
                (long long)P->edges, tau, P->n_clusters, P->n_members, P->max_nodes, P->fell_back);
    L.patches = P;
    return FEMSHELL_OK;
}

// lambda_max(D^-1 A) of a level by power iteration on the device (x <- D^-1 A x, ratio of consecutive norms).  In two halves:
// the launches, and -- when lambda is needed -- the one synchronisation that brings the last two norms back; a coarsening
// step on the device does its host-side graph work (aggregation, patterns: 0.16 s on the 4M-triangle meshes) in between
// while the GPU iterates.
// (beside: on the context's second stream, behind everything the first one holds at this moment -- the symbolic kernels of the
//  coarsening step, which the first stream gets next, then run beside the products instead of behind them: 30 products of K are
//  22 ms at 4M triangles, the patterns 10)
// (a row-partitioned level: the halo exchange in front of every product and the two last norms summed over the ranks -- its
//  collectives run on the context's stream, so it never runs beside)
int power_iteration_start(femshell_ctx *c, AmgLevel &L, const DeviceMatrix &A, int iterations, PowerIteration *pw, bool beside)
{
    hipStream_t st = c->stream;
    pw->dist = L.dist;
    if (beside && !L.dist && c->aux_stream != nullptr) {
        hipEvent_t ev;
        FS_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        FS_HIP(hipEventRecord(ev, c->stream));
        FS_HIP(hipStreamWaitEvent(c->aux_stream, ev, 0));
        FS_HIP(hipEventDestroy(ev));
        st = c->aux_stream;
    }
    pw->st = st;
    pw->G = slice_grid(A);
    // lambda is the ratio of the last two norms: only those come back to the host (one synchronisation instead of one per
    // step; without normalisation the iterate grows like lambda^k, lambda ~ 2, which 30 steps of FP64 take easily)
    FS_HIP(pw->part.alloc(2 * (size_t)pw->G + 2));
    double *x = L.d.p, *z = L.r.p;
    launch_fill_hash(x, 6ll * L.n, 6ll * L.n_pad, st);
    if (iterations < 2) iterations = 2;
    pw->iterations = iterations;
    for (int it = 0; it < iterations; it++) {
        if (L.dist) {
            const int rc = level_halo_exchange(c, *L.halo, x, 6, st);
            if (rc) return rc;
        }
        launch_spmv(A, x, L.q.p, SpmvEpilogue(), nullptr, st);
        launch_minv_apply_norm(A, L.q.p, z, pw->part.p + (size_t)(it & 1) * pw->G, st);
        if (L.patches) { // the level's smoother applies the cluster blocks: lambda_max of THAT operator
            launch_patch_correct(L.patches->view(), L.q.p, 1.0, z, false, nullptr, nullptr, st);
            launch_sqnorm_partials(z, 6ll * L.n_pad, pw->part.p + (size_t)(it & 1) * pw->G, pw->G, st);
        }
        std::swap(x, z);
    }
    FS_HIP(hipGetLastError());
    return FEMSHELL_OK;
}

int power_iteration_finish(femshell_ctx *c, PowerIteration &pw, double *lam_out)
{
    hipStream_t st = pw.st != nullptr ? pw.st : c->stream;
    const int G = pw.G, iterations = pw.iterations;
    // the two norms are sums over the G partials in index order, taken on the device (launch_sums_in_order: the host's loop of
    // rounds 3-5, same bits): 16 bytes come back instead of 16 G.  sums[j] = the sum over part[j G, (j + 1) G); the ranks of a
    // row partition all-reduce them as they lie, which of the two is the last norm is sorted out afterwards
    double *sums = pw.part.p + 2 * (size_t)G;
    launch_sums_in_order(pw.part.p, G, sums, st);
    FS_HIP(hipGetLastError());
    if (pw.dist) {
        std::string e;
        if (!comm_allreduce_sum(c->comm, sums, 2, st, &e)) return set_err(FEMSHELL_ERR_COMM, e);
    }
    double h[2] = {0.0, 0.0};
    FS_HIP(hipMemcpyAsync(h, sums, sizeof h, hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st));
    const double n_last = std::sqrt(h[(iterations - 1) & 1]), n_prev = std::sqrt(h[(iterations - 2) & 1]);
    if (!(n_prev > 0.0) || !std::isfinite(n_last) || !(n_last > 0.0))
        return set_err(FEMSHELL_ERR_BREAKDOWN, "multigrid setup: power iteration broke down");
    *lam_out = n_last / n_prev;
    return FEMSHELL_OK;
}

// (row-partitioned levels: every vector carries ghost space -- any of them may be the input of a halo product)
int alloc_level_vectors(AmgLevel &L, bool top, bool kcycle, hipStream_t st)
{
    const size_t n6 = (size_t)(L.n_pad + (L.dist ? L.n_ghost : 0)) * 6;
    if (!top) {
        FS_HIP(L.b.alloc(n6));
        FS_HIP(L.x.alloc(n6));
        FS_HIP(L.b.zero(st));
        FS_HIP(L.x.zero(st));
    }
    FS_HIP(L.r.alloc(n6));
    FS_HIP(L.d.alloc(n6));
    FS_HIP(L.q.alloc(n6));
    FS_HIP(L.r.zero(st));
    FS_HIP(L.d.zero(st));
    FS_HIP(L.q.zero(st));
    if (!top && kcycle) {
        FS_HIP(L.c1.alloc(n6));
        FS_HIP(L.v1.alloc(n6));
        FS_HIP(L.r2.alloc(n6));
        FS_HIP(L.c2.alloc(n6));
        FS_HIP(L.v2.alloc(n6));
        FS_HIP(L.c1.zero(st));
        FS_HIP(L.v1.zero(st));
        FS_HIP(L.r2.zero(st));
        FS_HIP(L.c2.zero(st));
        FS_HIP(L.v2.zero(st));
        FS_HIP(L.ks.alloc(1));
        FS_HIP(L.ks.zero(st));
        FS_HIP(L.kscratch.alloc(3 * 128));
        if (L.dist) {
            FS_HIP(L.ksums.alloc(8)); // (three sums, a spare; word 4: the ticket of the last-workgroup reduction, amg_kernels.hip)
            FS_HIP(L.ksums.zero(st));
        }
    }
    return FEMSHELL_OK;
}

double amg_lambda_safety()
{
    const double v = knob_double("FEMSHELL_AMG_LAMBDA_SAFETY", 1.1);
    return v >= 1.0 && v <= 4.0 ? v : 1.1;
}

int amg_power_iterations()
{
    const int v = (int)knob_long("FEMSHELL_AMG_POWER_ITS", 30);
    return v >= 2 && v <= 10000 ? v : 30;
}

bool coarse_symmetric_storage(int32_t n_nodes)
{
    // levels of at least 100,000 nodes (FEMSHELL_AMG_COARSE_SYM overrides; 1 = all levels, 0 = none) are stored like K,
    // diagonal + upper blocks: their products are HBM-bound (4M-triangle panel, level 1 of 222k nodes: 1.63 s against
    // 1.71 s per solve); the smaller levels are launch- and latency-bound, where the two-phase product loses (all
    // levels symmetric: 1.80 s)
    const long min_nodes = knob_long("FEMSHELL_AMG_COARSE_SYM", 100000l); // (read per call: the tests switch it inside one process)
    return min_nodes > 0 && n_nodes >= min_nodes && default_symmetric_storage();
}

void amg_default_options(femshell_pc_options *o)
{
    std::memset(o, 0, sizeof *o);
    o->type = FEMSHELL_PC_AMG;
    o->cycle = FEMSHELL_CYCLE_K;
    o->smoother_degree = 3; // tools/lab/amg_degree_probe.py, 4M triangles, rtol 1e-10 with the refinement pass: degrees 3 / 4
    o->coarse_degree = 4;   // against 2 / 4: panel 104 against 132 iterations, 0.98 against 1.04 s; cylinder 97 / 119, 0.91 /
                            // 0.94 s; roof 99 / 112, 0.087 / 0.089 s (3 / 3: 1.04 s on the panel; V cycles: twice the time)
    o->coarsest_nodes = 1400; // the K cycle's last levels cost launches, not bytes: end with an exact solve early (amg_dense.hip)
    o->max_levels = 12;
    o->refine_passes = 1;
    o->eig_ratio = 30.0;
}

const DeviceMatrix &amg_level_matrix(const femshell_ctx *c, int l) { return l == 0 ? c->dm : c->amg->levels[l]->A.dm; }

// ---- the block-Jacobi inverse by itself (tests: femshell_amg_device_block_jacobi, api.cpp) -------------------------------------
// A is packed and uploaded the way amg_finish_hierarchy packs a coarse level operator (storage 0: full, pack_sliced_ell; 1:
// diagonal + upper blocks, pack_sliced_ell_sym + in-lists; 2: as 1 with DeviceMatrix::diag_upper set, K's own layout, in which
// k_block_jacobi takes the strict lower triangle of a diagonal block from its mirror image), k_block_jacobi runs on it with a
// status word of this call, and the 21 packed words per node come back: minv_out[(slice * 21 + word) * 32 + node], n_pad nodes.
int amg_block_jacobi_device(femshell_ctx *c, const Bsr &A, int storage, std::vector<double> *minv_out, int32_t *status_out)
{
    hipStream_t st = c->stream;
    AmgOperator op;
    const int rc = upload_level_operator(op, A, storage != 0, st);
    if (rc) return rc;
    DevBuf<double> minv;
    DevBuf<int32_t> status;
    FS_HIP(minv.alloc((size_t)op.dm.n_slices * 21 * kSliceNodes));
    FS_HIP(status.alloc(1));
    FS_HIP(status.zero(st));
    op.dm.minv = minv.p;
    op.dm.status = status.p;
    op.dm.diag_upper = storage == 2 ? 1 : 0;
    launch_block_jacobi(op.dm, st);
    FS_HIP(hipGetLastError());
    minv_out->resize(minv.n);
    FS_HIP(hipMemcpyAsync(minv_out->data(), minv.p, minv.n * sizeof(double), hipMemcpyDeviceToHost, st));
    FS_HIP(hipMemcpyAsync(status_out, status.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st));
    return FEMSHELL_OK;
}

// ---- the inverse a level holds, and its two readers (tests: femshell_block_jacobi_export / _apply, api.cpp) ------------------
// the level's matrix as the smoothers see it (minv32 set where the level has the copy); levels without a smoother and
// block-Jacobi contexts: the operator itself
static const DeviceMatrix &inspected_level_matrix(const femshell_ctx *c, int level)
{
    if (c->amg && c->amg->valid && level < (int)c->amg->levels.size() && c->amg->levels[(size_t)level]->smooth_ready)
        return c->amg->levels[(size_t)level]->smooth_dm;
    return amg_level_matrix(c, level);
}

int amg_block_jacobi_words(femshell_ctx *c, int level, bool single_precision, std::vector<double> *words, int32_t *n_nodes, int32_t *n_pad)
{
    const DeviceMatrix &m = inspected_level_matrix(c, level);
    *n_nodes = m.n_own;
    *n_pad = m.n_pad;
    const size_t nw = (size_t)m.n_slices * 21 * kSliceNodes;
    words->assign(nw, 0.0);
    if (single_precision) {
        if (m.minv32 == nullptr) return set_err(FEMSHELL_ERR_INVALID, "femshell_block_jacobi_export: the level keeps no single-precision copy of its block-Jacobi inverse");
        std::vector<float> h(nw);
        FS_HIP(hipMemcpyAsync(h.data(), m.minv32, nw * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        FS_HIP(hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < nw; i++) (*words)[i] = (double)h[i];
    } else {
        if (m.minv == nullptr) return set_err(FEMSHELL_ERR_INVALID, "femshell_block_jacobi_export: the level has no block-Jacobi inverse");
        FS_HIP(hipMemcpyAsync(words->data(), m.minv, nw * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        FS_HIP(hipStreamSynchronize(c->stream));
    }
    return FEMSHELL_OK;
}

int amg_block_jacobi_apply(femshell_ctx *c, int level, int path, const double *r, double *z)
{
    const DeviceMatrix &m = inspected_level_matrix(c, level);
    if (m.minv == nullptr) return set_err(FEMSHELL_ERR_INVALID, "femshell_block_jacobi_apply: the level has no block-Jacobi inverse");
    hipStream_t st = c->stream;
    const size_t n6 = (size_t)m.n_pad * 6;
    DevBuf<double> dr, dz, dd, part;
    FS_HIP(dr.alloc(n6));
    FS_HIP(dz.alloc(n6));
    FS_HIP(hipMemcpyAsync(dr.p, r, n6 * sizeof(double), hipMemcpyHostToDevice, st));
    FS_HIP(hipMemsetAsync(dz.p, 0xff, n6 * sizeof(double), st)); // (NaN: every entry of z has to be written by the reader)
    if (path == 0) {
        FS_HIP(part.alloc((size_t)slice_grid(m)));
        launch_minv_apply_norm(m, dr.p, dz.p, part.p, st);
    } else {
        FS_HIP(dd.alloc(n6));
        launch_cheb_start(m, dr.p, dd.p, dz.p, 1.0, false, nullptr, st, 0);
    }
    FS_HIP(hipGetLastError());
    FS_HIP(hipMemcpyAsync(z, dz.p, n6 * sizeof(double), hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st));
    return FEMSHELL_OK;
}

namespace {

// which levels are coarsened where, and where the hierarchy ends
struct SetupRules {
    femshell_pc_options opt{};
    bool host_only = false;
    int32_t device_min = 5000;
    // Levels of more than device_min nodes are coarsened with the numerics on the device (amg_device_setup.cpp): their
    // operator is in HBM already and only its pattern is needed on the host.  The coarse operator of such a step comes
    // back as a host matrix only when the next step runs on the host (a small level, the coarsest one, the last allowed).
    bool device_step(int l, int32_t n_nodes) const
    {
        return !host_only && n_nodes > std::max(device_min, opt.coarsest_nodes) && l + 2 < opt.max_levels;
    }
    // The hierarchy ends at the first level of at most coarsest_nodes nodes -- but K itself is only "solved" by a dense
    // inverse when it is really small (kDirectNodes): the explicit FP64 inverse of a thin-shell K of a thousand nodes is not
    // a positive definite operator any more (coupled flap of 2,000 triangles, 6666 dofs: one pivot dropped, the CG residual
    // grows to 1e14), while the Galerkin operators below it are harmless (7386 dofs at 4M triangles).
    bool is_coarsest(int l, int32_t n_nodes) const
    {
        const int32_t limit = l == 0 ? std::min(opt.coarsest_nodes, kDirectNodes) : opt.coarsest_nodes;
        return n_nodes <= limit || l + 1 >= opt.max_levels;
    }
};

SetupRules setup_rules(const femshell_pc_options &opt)
{
    SetupRules r;
    r.opt = opt;
    // the first coarsening step runs its numerics on the device unless FEMSHELL_AMG_SETUP=host (amg_device_setup.cpp)
    r.host_only = knob_is("FEMSHELL_AMG_SETUP", "host");
    // nodes; levels at or below it are coarsened on the host (5000 since round 4: the 18.6k-node level of the 4M-triangle
    // meshes on the device as well, 46 -> 32 ms for the two steps below level 0)
    r.device_min = (int32_t)knob_long("FEMSHELL_AMG_DEVICE_MIN", 5000);
    return r;
}

// level 0 of a single-rank hierarchy: K as the plan describes it, and its work vectors
int create_level0(Amg &H, const Plan &pl, bool kcycle, hipStream_t st)
{
    H.levels.emplace_back(new AmgLevel());
    AmgLevel &L0 = *H.levels.back();
    L0.n = pl.n_own;
    L0.n_pad = pl.n_pad;
    L0.nnzb = pl.nnz_blocks;
    return alloc_level_vectors(L0, true, kcycle, st);
}

// ||A (inv32 v) - v|| / ||v|| for one vector v of mixed frequencies: what single precision did to the coarsest inverse
int dense_inverse_defect(femshell_ctx *c, AmgLevel &L, const DeviceMatrix &A, Amg &H, double *rel_out)
{
    hipStream_t st = c->stream;
    const int64_t n6 = 6ll * L.n_pad;
    launch_fill_hash(L.r.p, 6ll * L.n, n6, st);
    launch_dense_gemv_big(H.coarse_inv.p, H.coarse_inv32.p, H.coarse_lda, L.r.p, L.d.p, 6 * L.n, 6 * L.n_pad, nullptr, st);
    launch_spmv(A, L.d.p, L.q.p, SpmvEpilogue(), nullptr, st);
    launch_sub(L.q.p, L.r.p, L.q.p, n6, st);
    DevBuf<double> scratch;
    FS_HIP(scratch.alloc(3 * 128));
    const int groups = launch_two_dots(L.q.p, L.q.p, L.r.p, L.r.p, n6, scratch.p, st);
    double hp[2 * 128];
    FS_HIP(hipMemcpyAsync(hp, scratch.p, sizeof hp, hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st));
    FS_HIP(hipGetLastError());
    double ee = 0.0, vv = 0.0;
    for (int g = 0; g < groups; g++) {
        ee += hp[g];
        vv += hp[128 + g];
    }
    *rel_out = vv > 0.0 ? std::sqrt(ee / vv) : 0.0; // (NaN: the caller's test fails and the FP64 inverse is taken)
    return FEMSHELL_OK;
}
} // namespace

bool amg_keep_host(int64_t nnz_blocks)
{
    return nnz_blocks <= (knob_flag("FEMSHELL_AMG_KEEP_HOST", false) ? (int64_t)2000000 : (int64_t)300000); // (read per setup)
}

bool amg_uses_single_precision(const Amg &H)
{
    if (H.coarse_inv32.p != nullptr) return true;
    for (const auto &L : H.levels)
        if (L->A32.p != nullptr) return true;
    return false;
}

// Builds the hierarchy for the matrix currently in HBM.  Host: aggregation, prolongators, Galerkin products
// (amg_setup.cpp); device: lambda_max of every level, block-Jacobi inverses of the coarse operators.
int amg_setup(femshell_ctx *c)
{
    TraceRange trace("femshell multigrid setup");
    const double t0 = now_s();
    DevPool::Defer no_sync_per_free; // (buffers released during the setup join the pool at its end: dev_pool.hpp)
    hipStream_t st = c->stream;
    const femshell_pc_options opt = c->pc;
    const bool kcycle = opt.cycle == FEMSHELL_CYCLE_K;
    c->amg.reset(new Amg());
    Amg &H = *c->amg;
    H.opt = opt;
    const Plan &pl = c->plan;
    if (setup_verbose()) {
        double ps[6];
        DevPool::get().stats(ps); // (clears the counters: what follows belongs to this setup)
    }

    SetupLap lap{kLapPrefix, 28};
    const SetupRules rules = setup_rules(opt);
    const bool host_only = rules.host_only;
    const bool keep_host = amg_keep_host(pl.nnz_blocks); // inspection exports (tests)
    Bsr A;
    std::vector<double> B;  // near-null space of the current level on the host (levels coarsened on the host) ...
    DevBuf<double> Bdev;    // ... and in HBM (levels coarsened on the device, from the second one on)
    static const bool plain = amg_plain_rbm();
    // the node normals (48 MB to bring over at 4M triangles) on a thread of their own, beside the search for
    // clusters, the copy of the pattern and the greedy passes of the aggregation: the thread computes them and -- when a coarsening
    // step on the device will read them -- copies them into HBM on a stream of its own; whoever needs them first waits for the
    // thread (normals_ready: the host array is complete and the device copy has arrived)
    RawVec<double> normals;
    DevBuf<double> d_normals;
    std::thread normals_thread;
    hipError_t normals_err = hipSuccess;
    const bool normals_to_device = !plain && !host_only && opt.max_levels > 1 && pl.n_own > kDirectNodes;
    if (normals_to_device) FS_HIP(d_normals.alloc((size_t)pl.n_own * 3));
    if (!plain)
        normals_thread = std::thread([&] {
            node_normals_plan(pl, &normals);
            if (!normals_to_device) return;
            normals_err = hipSetDevice(c->device);
            if (normals_err == hipSuccess && c->copy_stream == nullptr) normals_err = hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking);
            hipStream_t s = c->copy_stream; // (see context.hpp)
            // (through the pinned staging buffer, region 1: `normals` is freed when the first step is through -- context.hpp stage_host)
            if (normals_err == hipSuccess && staged_upload(c, d_normals.p, normals.data(), normals.size() * sizeof(double), s, 1) != FEMSHELL_OK)
                normals_err = hipErrorUnknown;
        });
    auto normals_ready = [&] {
        if (normals_thread.joinable()) normals_thread.join();
    };
    struct JoinAtExit { // (every early return below)
        std::function<void()> f;
        ~JoinAtExit() { f(); }
    } join_at_exit{normals_ready};
    // (decided by amg_device_coarsen for the level it creates: it knows the coarse size only after the aggregation)
    auto want_host_matrix = [&](int next_level) {
        return std::function<bool(int32_t)>([&, next_level](int32_t na) { return !rules.device_step(next_level, na); });
    };
    int rc = FEMSHELL_OK;
    int first_level = 0;
    // clusters of rigidly coupled nodes (amg_patch.hpp: none on a mesh of decent element quality); a mesh that has them takes the
    // device path below whatever its size -- the host path has no cluster blocks
    std::shared_ptr<AmgPatches> patches0;
    // A mesh that is certain to take its first coarsening step on the device starts the power iteration of level 0 -- 30 products
    // of K on the second stream, 22 ms at 4M triangles, the longest thing the GPU has to do in a setup -- before anything else; the
    // search for clusters, the host's copy of the pattern, the aggregation and the symbolic kernels all run beside it.  (A mesh that
    // turns out to have clusters starts it again: lambda_max is then that of the smoother with the cluster blocks.)
    PowerIteration pw_early;
    bool early = false;
    if (!host_only && opt.max_levels > 1 && pl.n_own > opt.coarsest_nodes && pl.n_own > kDirectNodes) {
        rc = create_level0(H, pl, kcycle, st);
        if (rc) return rc;
        rc = power_iteration_start(c, *H.levels[0], c->dm, amg_power_iterations(), &pw_early, true);
        if (rc) return rc;
        early = true;
    }
    if (!host_only && opt.max_levels > 1 && pl.n_own > kDirectNodes) {
        AmgLevel probe;
        probe.n = pl.n_own;
        rc = amg_build_patches(c, c->dm, probe, false);
        if (rc) return rc;
        patches0 = probe.patches;
        lap("patch smoother: clusters", 0);
    }
    if (!host_only && (pl.n_own > opt.coarsest_nodes || patches0) && opt.max_levels > 1) { // (small meshes: host algebra below)
        if (!early) {
            rc = create_level0(H, pl, kcycle, st);
            if (rc) return rc;
        }
        AmgLevel &L0 = *H.levels[0];
        L0.patches = patches0;
        if (early && patches0) { // (the early power iteration ran without the cluster blocks)
            FS_HIP(hipStreamSynchronize(pw_early.st));
            early = false;
        }
        H.levels.emplace_back(new AmgLevel());
        AmgLevel &L1 = *H.levels.back();
        std::vector<double> Bc;
        pattern_of_plan(pl, &L0.pattern, /*light=*/true); // (amg_device_coarsen fills the slot arrays if it needs the host's lists)
        lap("pattern of K", 0);
        // the near-null space of the finest level is generated from the mesh in HBM (never stored: n x 36 doubles)
        NearNullSrc src;
        src.xyz = c->xyz.p;
        src.dmask = c->dmask.p;
        if (!plain) src.normals = d_normals.p;
        // (amg_device_coarsen calls this when the tentative prolongator is about to read them)
        auto upload_normals = [&]() -> int {
            if (plain) return (int)FEMSHELL_OK;
            normals_ready();
            FS_HIP(normals_err);
            return (int)FEMSHELL_OK;
        };
        double ctr[3];
        mesh_centre(pl.n_own, pl.xyz_local.data(), ctr);
        src.cx = ctr[0];
        src.cy = ctr[1];
        src.cz = ctr[2];
        // (with clusters: glued into aggregates; should an aggregate then be seen by more fine rows than a row of R holds, once more
        //  without the gluing, and without the cluster blocks at all if that fails too)
        for (int attempt = 0;; attempt++) {
            PowerIteration pw_now; // (its launches now, its result when the prolongator is smoothed: amg_device_coarsen asks for it)
            const bool reuse_early = attempt == 0 && early;
            PowerIteration &pw0 = reuse_early ? pw_early : pw_now;
            if (!reuse_early) {
                rc = power_iteration_start(c, L0, c->dm, amg_power_iterations(), &pw0, true);
                if (rc) return rc;
            }
            auto lam0 = [&](double *out) {
                double lam = 0.0;
                const int r2 = power_iteration_finish(c, pw0, &lam);
                if (r2) return r2;
                *out = L0.lam = amg_lambda_safety() * lam;
                return (int)FEMSHELL_OK;
            };
            rc = amg_device_coarsen(c, c->dm, L0.pattern, L0, L1, src, lam0, keep_host, want_host_matrix(1), &A, &Bc, &Bdev, std::ref(lap), upload_normals);
            if (rc == FEMSHELL_ERR_UNSUPPORTED && L0.patches && attempt < 2) {
                FS_HIP(hipStreamSynchronize(pw0.st)); // (the power iteration of this attempt)
                FS_HIP(hipStreamSynchronize(st));
                if (L0.patches->glue) L0.patches->glue = false;
                else L0.patches.reset();
                if (setup_verbose()) fprintf(stderr, "[femshell amg setup] patch smoother: %s\n", L0.patches ? "once more without gluing the clusters" : "given up for this mesh");
                continue;
            }
            break;
        }
        if (rc) return rc;
        L0.pattern = HostEllPattern(); // (the plan holds it)
        L1.A_on_device = true;
        if (keep_host) {
            rc = download_matrix(c, &L0.hA);
            if (rc) return rc;
        }
        B.swap(Bc);
        first_level = 1;
    } else {
        rc = download_matrix(c, &A);
        if (rc) return rc;
        normals_ready();
        rigid_body_modes(pl.n_own, pl.xyz_local.data(), c->dmask_global.data() + pl.row_begin, &B, plain ? nullptr : normals.data());
        lap("download K", 0);
    }
    normals_ready();
    RawVec<double>().swap(normals);

    rc = amg_finish_hierarchy(c, A, B, Bdev, first_level);
    if (rc) return rc;
    H.setup_seconds = now_s() - t0;
    if (setup_verbose()) {
        double ps[6];
        DevPool::get().stats(ps);
        fprintf(stderr, "[femshell amg setup] device allocator during this setup (and whatever ran since the last one): %.0f hipMalloc %.1f ms, %.0f hipFree %.1f ms, "
                        "%.0f blocks to the pool behind a device synchronisation %.1f ms\n", ps[0], ps[1], ps[2], ps[3], ps[4], ps[5]);
    }
    return FEMSHELL_OK;
}

int level_block_jacobi(femshell_ctx *c, AmgLevel &L, int level, bool *bad)
{
    hipStream_t st = c->stream;
    FS_HIP(L.minv.alloc((size_t)L.A.dm.n_slices * 21 * kSliceNodes));
    L.A.dm.minv = L.minv.p;
    L.A.dm.status = c->status_word;
    launch_block_jacobi(L.A.dm, st);
    FS_HIP(hipGetLastError());
    int32_t status_now = 0;
    int rc = fetch_status_word(c, st, &status_now);
    if (rc) return rc;
    *bad = status_now != 0;
    if (!*bad) return FEMSHELL_OK;
    rc = clear_status_word(c, st);
    if (rc) return rc;
    (void)set_err(FEMSHELL_ERR_BREAKDOWN, "multigrid setup: a diagonal block of coarse level " + std::to_string(level) + " is not positive definite");
    return FEMSHELL_OK;
}

// ---- the steps of amg_finish_hierarchy ------------------------------------------------------------------------------------------
namespace {

// nodes and blocks of a level from its operator: the host matrix, or the pattern of the one in HBM
void set_level_sizes(AmgLevel &L, const Bsr &A, bool have_host)
{
    if (have_host) {
        L.n = A.nr;
        L.nnzb = A.nnzb();
    } else {
        L.n = L.pattern.n;
        int64_t stored = 0;
        for (int32_t a = 0; a < L.n; a++) stored += L.pattern.count[(size_t)a];
        L.nnzb = L.pattern.symmetric ? 2 * stored - L.n : stored;
    }
    L.n_pad = (L.n + kSliceNodes - 1) / kSliceNodes * kSliceNodes;
}

// the coarsest level: the dense inverse of its operator A (Adev: the same in HBM), on the host or on the matrix cores
int coarsest_inverse(femshell_ctx *c, AmgLevel &L, int l, Bsr &A, const DeviceMatrix &Adev, bool have_host, SetupLap &lap)
{
    hipStream_t st = c->stream;
    Amg &H = *c->amg;
    std::vector<double> inv;
    if (L.n > 4096) return set_err(FEMSHELL_ERR_UNSUPPORTED, "multigrid setup: coarsest level too large for a dense inverse");
    if (!have_host) return set_err(FEMSHELL_ERR_INVALID, "multigrid setup: the coarsest operator was not brought to the host");
    // the smallest operators are inverted on the host; beyond FEMSHELL_AMG_DENSE_DEVICE_MIN nodes (default 64; 250
    // until the host's 0.19 s at 145 nodes and 0.35 s at 204 showed up as most of the setup of the small coupled
    // examples) the inverse is computed on the matrix cores (amg_dense.hip: n^3 flops, 0.4 TFLOP at 1231 nodes)
    // (read per setup: the tests switch them inside one process)
    const long dense_device_min = knob_long("FEMSHELL_AMG_DENSE_DEVICE_MIN", 64l);
    // (stored and applied in single precision unless FEMSHELL_AMG_DENSE_F32=0: the coarsest solve sits inside a K cycle
    //  inside a flexible Krylov method, 1e-7 there moves the iteration count by one or two and halves the 436 MB the
    //  four visits per iteration stream: panel 0.809 -> 0.785 s, cylinder 0.755 -> 0.744 s)
    const bool dense_f32 = !c->amg_fp64_only && knob_flag("FEMSHELL_AMG_DENSE_F32", true);
    H.coarse_lda = 0;
    H.dense = AmgDenseStats();
    H.coarse_inv32.release();
    int rc = FEMSHELL_OK;
    if (L.n > dense_device_min) {
        rc = amg_dense_inverse_device(c, A, dense_f32, &H.coarse_inv, &H.coarse_inv32, &H.coarse_lda, &H.dense);
        if (rc) return rc;
        if (dense_f32) {
            // Is the rounded inverse still an inverse?  Its entries are off by 6e-8 of the largest, the smallest
            // eigenvalue of A^-1 lies kappa(A) below that: beyond kappa ~ 1e6 the float copy is not positive definite
            // any more (a cantilever strip of t / L = 1 / 1600: CG breakdown).  ||A (inv32 v) - v|| / ||v|| on one
            // vector of mixed frequencies shows kappa eps; above 0.05 the inverse is computed again and kept FP64.
            double rel = 0.0;
            rc = dense_inverse_defect(c, L, Adev, H, &rel);
            if (rc) return rc;
            H.dense.f32_defect = rel;
            if (setup_verbose())
                fprintf(stderr, "[femshell amg setup] coarsest inverse rounded to single precision: ||A inv32 v - v|| / ||v|| = %.2e (%s)\n", rel,
                        rel <= 0.05 ? "kept" : "above 0.05: the FP64 inverse is kept instead");
            if (!(rel <= 0.05)) {
                H.coarse_inv32.release();
                rc = amg_dense_inverse_device(c, A, false, &H.coarse_inv, &H.coarse_inv32, &H.coarse_lda, &H.dense);
                if (rc) return rc;
                H.dense.f32_defect = rel;
            }
        }
        lap("dense inverse on the matrix cores", l);
    } else {
        if (!dense_inverse(A, &inv))
            return set_err(FEMSHELL_ERR_BREAKDOWN, "multigrid setup: coarsest operator is not positive definite");
        FS_HIP(H.coarse_inv.upload(inv, st));
        FS_HIP(hipStreamSynchronize(st));
        lap("dense inverse on the host", l);
    }
    L.hA = std::move(A); // (kept at every size: a few MB, and the operator the dense inverse is checked against)
    return FEMSHELL_OK;
}

// one coarsening step on the host (amg_setup.cpp) from the level's operator A, its near-null space B and its spectral bound L.lam:
// P and R of the level into HBM; A and B become those of the next level
int host_coarsen(femshell_ctx *c, AmgLevel &L, int l, Bsr &A, std::vector<double> &B, bool keep_host, SetupLap &lap)
{
    hipStream_t st = c->stream;
    std::vector<int32_t> agg;
    const int32_t na = aggregate_nodes(A, &agg);
    lap("aggregation", l);
    std::vector<double> Q, Bc, Dinv;
    tentative_prolongator(agg, na, B, &Q, &Bc);
    block_diagonal_inverse(A, &Dinv);
    lap("tentative P, D^-1", l);
    Bsr P, R, Ac;
    smoothed_prolongator(A, Dinv, agg, na, Q, (4.0 / 3.0) / L.lam, &P);
    std::vector<double>().swap(Q);
    std::vector<double>().swap(Dinv);
    lap("smoothed P", l);
    galerkin_product(A, P, &R, &Ac);
    lap("Galerkin product", l);
    {
        SlicedEll S;
        const int32_t nc_pad = (na + kSliceNodes - 1) / kSliceNodes * kSliceNodes;
        pack_sliced_ell(P, false, &S);
        int rc = upload_operator(L.P, S, nc_pad, P.nnzb(), st);
        if (rc) return rc;
        pack_sliced_ell(R, false, &S);
        rc = upload_operator(L.R, S, L.n_pad, R.nnzb(), st);
        if (rc) return rc;
    }
    lap("pack + upload P, R", l);
    if (keep_host) {
        L.hA = std::move(A);
        L.hP = std::move(P);
    }
    if (keep_host || l == 0) L.agg = std::move(agg);
    A = std::move(Ac);
    B.swap(Bc);
    return FEMSHELL_OK;
}

// Chebyshev coefficients per level
void chebyshev_coefficients(Amg &H)
{
    for (size_t l = 0; l + 1 < H.levels.size(); l++) {
        AmgLevel &L = *H.levels[l];
        const int deg = std::max(1, l == 0 ? H.opt.smoother_degree : H.opt.coarse_degree);
        const double lmax = L.lam, lmin = L.lam / H.opt.eig_ratio;
        const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sigma = theta / delta;
        L.inv_theta = 1.0 / theta;
        L.cheb_a.clear();
        L.cheb_c.clear();
        double rho = 1.0 / sigma;
        for (int k = 1; k < deg; k++) {
            const double rho_new = 1.0 / (2.0 * sigma - rho);
            L.cheb_a.push_back(rho_new * rho);
            L.cheb_c.push_back(2.0 * rho_new / delta);
            rho = rho_new;
        }
    }
}

// the single-precision copies of the levels, and what the smoothers and the transfers of the cycle multiply with (smooth_dm)
int single_precision_copies(femshell_ctx *c)
{
    hipStream_t st = c->stream;
    Amg &H = *c->amg;
    const Plan &pl = c->plan;
    // FEMSHELL_AMG_SMOOTH_F32: the Chebyshev products of the levels stream a single-precision copy of the operator's
    // values (half the bytes of the HBM-bound part of the cycle); residuals, the Krylov product, the K cycle's products,
    // the Galerkin operators themselves and the transfers stay FP64.  The soft modes of a shell sit twelve decades
    // below ||K||: only the smoother -- a polynomial in D^-1 A whose job is the upper end of the spectrum -- tolerates
    // 1e-7, and the flexible Krylov method around the cycle does not care that the preconditioner moved a little.
    // 1 (default): levels of at least 4096 nodes; 2: level 0 only, 3: every level, whatever their size (A/B runs, tests); 0: off.
    const int mode = c->amg_fp64_only ? 0 : (int)knob_long("FEMSHELL_AMG_SMOOTH_F32", 1);
    // (what the coarsening steps released -- A P, Q, the symbolic buffers -- joins the pool's kept blocks now: the copies below are
    //  carved from them instead of being fresh requests to the driver, dev_pool.hpp DevPool::alloc (3))
    if (mode != 0) (void)DevPool::get().flush_pending();
    for (size_t l = 0; l + 1 < H.levels.size(); l++) {
        AmgLevel &L = *H.levels[l];
        L.A32.release();
        const DeviceMatrix &A = amg_level_matrix(c, (int)l);
        // (the size of the WHOLE level decides on a row-partitioned one: every rank takes the same decision, which the
        //  fallback of femshell_solve -- a collective rebuild -- relies on)
        const int32_t level_nodes = L.dist ? std::max(L.n, L.n_global) : L.n;
        if (mode == 0 || (mode == 2 && l > 0) || (mode == 1 && level_nodes < 4096) || A.vals == nullptr) continue;
        // a level with clusters of rigidly coupled nodes keeps everything in double precision: what makes the clusters -- pairs of
        // blocks that nearly cancel -- is what a product in single precision loses (the flexible CG broke down under the copies on
        // every such shell tried, and the all-FP64 rebuild of femshell_solve did what this line does at once)
        if (L.patches) continue;
        const int64_t nv = (l == 0 ? (int64_t)pl.total_slots() : (int64_t)L.A.vals.n / 36) * 36;
        FS_HIP(L.A32.alloc((size_t)nv));
        launch_to_f32(A.vals, L.A32.p, nv, st);
        // the block-Jacobi inverse the smoothers apply, and the transfer operators (R = P^T value by value, so the
        // rounded pair is still a transposed pair and the cycle stays symmetric)
        const int64_t nm = (int64_t)A.n_slices * 21 * kSliceNodes;
        FS_HIP(L.minv32.alloc((size_t)nm));
        launch_to_f32(A.minv, L.minv32.p, nm, st);
        // (transfers onto a small level are bound by latency, where half-width loads lose: R onto the 1231-node level
        //  22 -> 36 us in single precision)
        const bool big_coarse = mode == 3 || H.levels[l + 1]->n >= 4096 || H.levels[l + 1]->n_global >= 4096;
        if (mode != 2 && big_coarse && L.P.vals.n > 0 && L.R.vals.n > 0) {
            FS_HIP(L.P32.alloc(L.P.vals.n));
            FS_HIP(L.R32.alloc(L.R.vals.n));
            launch_to_f32(L.P.vals.p, L.P32.p, (int64_t)L.P.vals.n, st);
            launch_to_f32(L.R.vals.p, L.R32.p, (int64_t)L.R.vals.n, st);
        }
        FS_HIP(hipGetLastError());
    }
    for (size_t l = 0; l + 1 < H.levels.size(); l++) { // what the smoothers and the transfers of the cycle multiply with
        AmgLevel &L = *H.levels[l];
        L.smooth_dm = amg_level_matrix(c, (int)l);
        L.smooth_dm.vals32 = L.A32.p;
        L.smooth_dm.minv32 = L.minv32.p;
        // a level whose vectors are exchanged with the neighbour ranks keeps the input of its products FP64 (the halo
        // exchange moves six doubles per node)
        L.smooth_dm.vec32 = !has_lowp_copy(L) ? 0 : std::min(smooth_vectors_f32(), L.dist ? 1 : 2);
        L.P.dm.vals32 = L.P32.p;
        L.R.dm.vals32 = L.R32.p;
        L.smooth_ready = true;
    }
    return FEMSHELL_OK;
}

} // namespace

// The levels from first_level on, on one rank or replicated on every rank of a row partition (amg_dist.cpp hands over the
// all-gathered operator of the first replicated level).  A: that level's operator as a host matrix (empty: the level is in
// HBM with its pattern and Bdev is its near-null space), B: its near-null space on the host.
int amg_finish_hierarchy(femshell_ctx *c, Bsr &A, std::vector<double> &B, DevBuf<double> &Bdev, int first_level)
{
    hipStream_t st = c->stream;
    Amg &H = *c->amg;
    const bool kcycle = H.opt.cycle == FEMSHELL_CYCLE_K;
    const SetupRules rules = setup_rules(H.opt);
    auto want_host_matrix = [&](int next_level) {
        return std::function<bool(int32_t)>([&, next_level](int32_t na) { return !rules.device_step(next_level, na); });
    };
    const bool keep_host = amg_keep_host(c->plan.nnz_blocks); // inspection exports (tests)
    SetupLap lap{kLapPrefix, 28};
    int rc = FEMSHELL_OK;
    for (int l = first_level;; l++) {
        if ((int)H.levels.size() <= l) H.levels.emplace_back(new AmgLevel());
        AmgLevel &L = *H.levels[l];
        const bool have_host = A.nr > 0 || !L.A_on_device; // the level's operator as a host matrix (else: in HBM + pattern)
        set_level_sizes(L, A, have_host);
        if (l > 0) {
            // the level operators are symmetric: diagonal and upper blocks only, like K (FEMSHELL_SYMMETRIC=0: full)
            if (!L.A_on_device) rc = upload_level_operator(L.A, A, coarse_symmetric_storage(A.nr), st);
            if (rc) return rc;
            bool bad = false;
            rc = level_block_jacobi(c, L, l, &bad);
            if (rc) return rc;
            if (bad) return FEMSHELL_ERR_BREAKDOWN; // (its text is set)
        }
        rc = alloc_level_vectors(L, l == 0, kcycle, st);
        if (rc) return rc;
        lap("upload + block-Jacobi", l);
        const DeviceMatrix &Adev = amg_level_matrix(c, l);
        if (rules.is_coarsest(l, L.n)) {
            rc = coarsest_inverse(c, L, l, A, Adev, have_host, lap);
            if (rc) return rc;
            break;
        }
        PowerIteration pw;
        rc = power_iteration_start(c, L, Adev, amg_power_iterations(), &pw);
        if (rc) return rc;
        bool lam_known = false;
        auto lam_of = [&](double *out) {
            if (!lam_known) {
                double lam = 0.0;
                const int r2 = power_iteration_finish(c, pw, &lam);
                if (r2) return r2;
                L.lam = amg_lambda_safety() * lam; // the power iteration approaches from below
                lam_known = true;
            }
            *out = L.lam;
            return (int)FEMSHELL_OK;
        };
        // coarsen
        if (L.A_on_device && !L.pattern.empty() && rules.device_step(l, L.n)) {
            // on the device: the operator is in HBM, its pattern on the host (amg_device_setup.cpp)
            if ((int)H.levels.size() <= l + 1) H.levels.emplace_back(new AmgLevel());
            AmgLevel &N = *H.levels[(size_t)l + 1];
            std::vector<double> Bc;
            DevBuf<double> Bnext;
            Bsr Anext;
            NearNullSrc src;
            if (Bdev.p == nullptr) { // (the level came from a host step)
                FS_HIP(Bdev.upload(B, st));
            }
            src.B = Bdev.p;
            rc = amg_device_coarsen(c, L.A.dm, L.pattern, L, N, src, lam_of, keep_host, want_host_matrix(l + 1), &Anext, &Bc, &Bnext, std::ref(lap));
            if (rc) return rc;
            Bdev.swap(Bnext);
            N.A_on_device = true;
            if (keep_host && have_host) L.hA = std::move(A);
            L.pattern = HostEllPattern();
            A = std::move(Anext);
            B.swap(Bc);
            continue;
        }
        // on the host (amg_setup.cpp)
        if (!have_host) return set_err(FEMSHELL_ERR_INVALID, "multigrid setup: level operator neither on the host nor coarsened on the device");
        double lam_now = 0.0;
        rc = lam_of(&lam_now);
        if (rc) return rc;
        lap("power iteration", l);
        rc = host_coarsen(c, L, l, A, B, keep_host, lap);
        if (rc) return rc;
        Bdev.release();
    }
    chebyshev_coefficients(H);
    rc = single_precision_copies(c);
    if (rc) return rc;
    FS_HIP(hipStreamSynchronize(st));
    lap("smoother coefficients, single-precision copies", (int)H.levels.size() - 1);
    H.valid = true;
    return FEMSHELL_OK;
}

} // namespace femshell

