// api_krylov_probe.cpp -- femshell_krylov_set / _get / _launch and femshell_cg_reduce: the Krylov loops of cg_driver.cpp and cg_amg
// launch by launch, for tests.  "Set, launch one, get" on the context's own CG state -- cg_vectors(c), c->scal --
// through the production launchers and nothing else: no arithmetic lives here, and no production path runs through this file.
#include "api_internal.hpp"

#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

using namespace femshell;

// the mirror of include/femshell.h is CgScalars word for word
static_assert(sizeof(femshell_krylov_scalars) == sizeof(CgScalars), "femshell_krylov_scalars mirrors CgScalars");
static_assert(sizeof(CgScalars) % sizeof(double) == 0, "the scalars travel as doubles");
#define FS_SAME_OFFSET(f) static_assert(offsetof(femshell_krylov_scalars, f) == offsetof(CgScalars, f), "femshell_krylov_scalars::" #f)
FS_SAME_OFFSET(rz);
FS_SAME_OFFSET(alpha);
FS_SAME_OFFSET(beta);
FS_SAME_OFFSET(rr);
FS_SAME_OFFSET(bb);
FS_SAME_OFFSET(tol2);
FS_SAME_OFFSET(red);
FS_SAME_OFFSET(done);
FS_SAME_OFFSET(iters);
FS_SAME_OFFSET(ticket);
FS_SAME_OFFSET(pad);
FS_SAME_OFFSET(stage);
FS_SAME_OFFSET(ring_rz);
FS_SAME_OFFSET(ring_alpha);
FS_SAME_OFFSET(pass_xx);
FS_SAME_OFFSET(pass_rhs_rr);
FS_SAME_OFFSET(pass_rtol);
#undef FS_SAME_OFFSET

namespace {

constexpr int64_t kScalarWords = (int64_t)(sizeof(CgScalars) / sizeof(double));
constexpr int64_t kHistoryMax = 4096;

// what the three entry points refuse alike; nothing of the context has changed when this returns an error
int probe_ready(femshell_ctx *c, const char *what)
{
    const std::string w(what);
    if (!c) return set_err(FEMSHELL_ERR_INVALID, w + ": null context");
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, w + ": no mesh set");
    if (c->assembly_pending) return set_err(FEMSHELL_ERR_INVALID, w + ": an assembly is pending (femshell_sync first)");
    if (c->dyn.active) return set_err(FEMSHELL_ERR_INVALID, w + ": not while dynamics is active (femshell_dynamics_end first)");
    if (!have(c, kK | kJacobi))
        return set_err(FEMSHELL_ERR_INVALID, w + ": K and its block-Jacobi inverse are not in HBM (femshell_assemble and a solve, or femshell_block_jacobi_export, first)");
    return select_device(c);
}

// the vectors by their numbers in include/femshell.h (b: the context's F)
double *probe_vector(femshell_ctx *c, int32_t which)
{
    switch (which) {
    case FEMSHELL_KRYLOV_X: return c->x.p;
    case FEMSHELL_KRYLOV_R: return c->r.p;
    case FEMSHELL_KRYLOV_Z: return c->z.p;
    case FEMSHELL_KRYLOV_P: return c->p.p;
    case FEMSHELL_KRYLOV_Q: return c->q.p;
    case FEMSHELL_KRYLOV_SV: return c->sv.p;
    case FEMSHELL_KRYLOV_B: return c->F.p;
    default: return nullptr;
    }
}

// cg_vectors with the probe's own history
CgVectors probe_vectors(femshell_ctx *c)
{
    CgVectors v = cg_vectors(c);
    v.hist = c->probe_hist_cap > 0 ? c->probe_hist.p : nullptr;
    v.hist_cap = c->probe_hist_cap;
    return v;
}

bool hierarchy_ready(const femshell_ctx *c, size_t min_levels)
{
    return c->pc.type == FEMSHELL_PC_AMG && c->amg && c->amg->valid && c->amg->levels.size() >= min_levels;
}

} // namespace

extern "C" {

int32_t femshell_krylov_grid(femshell_ctx *c)
{
    if (!c || !c->have_mesh) return -1;
    return (int32_t)slice_grid(c->dm);
}

int femshell_krylov_set(femshell_ctx *c, int32_t which, const double *data, int64_t n)
{
    const char *what = "femshell_krylov_set";
    int rc = probe_ready(c, what);
    if (rc) return rc;
    if (!data) return set_err(FEMSHELL_ERR_INVALID, "femshell_krylov_set: null argument");
    const Plan &p = c->plan;
    hipStream_t st = c->stream;
    if (double *dst = probe_vector(c, which)) {
        if (n != 6ll * p.n_nodes) return set_err(FEMSHELL_ERR_INVALID, "femshell_krylov_set: a vector holds 6 values per node of the mesh");
        std::vector<double> stage;
        rc = upload_node_block(c, NodeOrder::caller, 1, data, dst, (size_t)p.n_pad * 6, &stage); // (padding rows: zero)
        if (rc) return rc;
        FS_HIP(hipStreamSynchronize(st));
        invalidate(c, Change::krylov_probe);
        if (which == FEMSHELL_KRYLOV_B) invalidate(c, Change::loads); // HBM no longer holds the F of the loads
        return FEMSHELL_OK;
    }
    if (which == FEMSHELL_KRYLOV_PARTIALS) {
        if (n < 1 || n > (int64_t)c->partials.n) return set_err(FEMSHELL_ERR_INVALID, "femshell_krylov_set: the partial sums are 1 .. 4 G doubles");
        FS_HIP(hipMemcpyAsync(c->partials.p, data, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    } else if (which == FEMSHELL_KRYLOV_SCALARS) {
        if (n != kScalarWords) return set_err(FEMSHELL_ERR_INVALID, "femshell_krylov_set: the scalars are one femshell_krylov_scalars");
        FS_HIP(hipMemcpyAsync(c->scal.p, data, sizeof(CgScalars), hipMemcpyHostToDevice, st));
    } else if (which == FEMSHELL_KRYLOV_HISTORY) {
        if (n < 1 || n > kHistoryMax) return set_err(FEMSHELL_ERR_INVALID, "femshell_krylov_set: the history holds 1 .. 4096 words");
        FS_HIP(c->probe_hist.alloc((size_t)n));
        c->probe_hist_cap = (int32_t)n;
        FS_HIP(hipMemcpyAsync(c->probe_hist.p, data, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    } else if (which == FEMSHELL_KRYLOV_HISTORY_CAP) {
        const double cap = data[0];
        if (n != 1 || !(cap >= 0.0) || cap > (double)c->probe_hist.n || cap != (double)(int32_t)cap)
            return set_err(FEMSHELL_ERR_INVALID, "femshell_krylov_set: the cap is a whole number of 0 .. the words of the history buffer");
        c->probe_hist_cap = (int32_t)cap;
        return FEMSHELL_OK;
    } else {
        return set_err(FEMSHELL_ERR_INVALID, "femshell_krylov_set: no such array");
    }
    FS_HIP(hipStreamSynchronize(st));
    return FEMSHELL_OK;
}

int femshell_krylov_get(femshell_ctx *c, int32_t which, double *data, int64_t n)
{
    int rc = probe_ready(c, "femshell_krylov_get");
    if (rc) return rc;
    if (!data) return set_err(FEMSHELL_ERR_INVALID, "femshell_krylov_get: null argument");
    const Plan &p = c->plan;
    hipStream_t st = c->stream;
    if (const double *src = probe_vector(c, which)) {
        if (n != 6ll * p.n_nodes) return set_err(FEMSHELL_ERR_INVALID, "femshell_krylov_get: a vector holds 6 values per node of the mesh");
        return download_node_block(c, NodeOrder::caller, 1, src, 0, data);
    }
    if (which == FEMSHELL_KRYLOV_PARTIALS) {
        if (n < 1 || n > (int64_t)c->partials.n) return set_err(FEMSHELL_ERR_INVALID, "femshell_krylov_get: the partial sums are 1 .. 4 G doubles");
        FS_HIP(hipMemcpyAsync(data, c->partials.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    } else if (which == FEMSHELL_KRYLOV_SCALARS) {
        if (n != kScalarWords) return set_err(FEMSHELL_ERR_INVALID, "femshell_krylov_get: the scalars are one femshell_krylov_scalars");
        FS_HIP(hipMemcpyAsync(data, c->scal.p, sizeof(CgScalars), hipMemcpyDeviceToHost, st));
    } else if (which == FEMSHELL_KRYLOV_HISTORY) {
        if (n < 1 || n > (int64_t)c->probe_hist.n) return set_err(FEMSHELL_ERR_INVALID, "femshell_krylov_get: more words than the history buffer holds");
        FS_HIP(hipMemcpyAsync(data, c->probe_hist.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    } else if (which == FEMSHELL_KRYLOV_HISTORY_CAP) {
        if (n != 1) return set_err(FEMSHELL_ERR_INVALID, "femshell_krylov_get: the cap is one word");
        data[0] = (double)c->probe_hist_cap;
        return FEMSHELL_OK;
    } else {
        return set_err(FEMSHELL_ERR_INVALID, "femshell_krylov_get: no such array");
    }
    FS_HIP(hipStreamSynchronize(st));
    return FEMSHELL_OK;
}

int femshell_krylov_launch(femshell_ctx *c, int32_t step, const int32_t *args, double rtol, int32_t *iout, double *dout)
{
    const char *what = "femshell_krylov_launch";
    int rc = probe_ready(c, what);
    if (rc) return rc;
    if (!args) return set_err(FEMSHELL_ERR_INVALID, "femshell_krylov_launch: null argument");
    if (!(rtol >= 0.0)) return set_err(FEMSHELL_ERR_INVALID, "femshell_krylov_launch: rtol < 0 or not a number");
    const DeviceMatrix &m = c->dm;
    hipStream_t st = c->stream;
    const int G = slice_grid(m);
    const int64_t n6 = 6ll * m.n_pad;
    const int32_t a0 = args[0], a1 = args[1];
    auto flag = [](int32_t a) { return a == 0 || a == 1; };
    auto refuse = [](const char *why) { return set_err(FEMSHELL_ERR_INVALID, std::string("femshell_krylov_launch: ") + why); };
    // every refusal comes before the first launch
    switch (step) {
    case FEMSHELL_KSTEP_CG_INIT:
        if (!flag(a0)) return refuse("restart is 0 or 1");
        break;
    case FEMSHELL_KSTEP_CG_UPDATE:
        if (!flag(a0) || (a0 && !m.symmetric)) return refuse("gather is 0 or 1, and 1 on symmetric storage only");
        break;
    case FEMSHELL_KSTEP_CGCG_UPDATE:
        if (a0 < -1 || a0 > 1) return refuse("step is -1, 0 or 1");
        if (!flag(a1) || (a1 && !m.symmetric)) return refuse("gather is 0 or 1, and 1 on symmetric storage only");
        break;
    case FEMSHELL_KSTEP_PCG_UPDATE_START:
        if (!flag(a0) || (a0 && !m.symmetric)) return refuse("gather is 0 or 1, and 1 on symmetric storage only");
        if (!hierarchy_ready(c, 2) || !c->amg->levels[0]->d.p) return refuse("the fused update needs a multigrid hierarchy of two levels or more");
        break;
    case FEMSHELL_KSTEP_PC_APPLY:
        if (!flag(a0)) return refuse("pre_started is 0 or 1");
        if (!hierarchy_ready(c, a0 ? 2 : 1)) return refuse("no multigrid hierarchy (of two levels or more behind a fused update)");
        break;
    case FEMSHELL_KSTEP_PRODUCT:
        if (!flag(a0) || !flag(a1)) return refuse("the input is 0 (p) or 1 (z), the deferred gather 0 or 1");
        break;
    case FEMSHELL_KSTEP_SYM_GATHER:
        if (!m.symmetric) return refuse("symmetric storage only");
        break;
    case FEMSHELL_KSTEP_TWO_DOTS:
        if (!probe_vector(c, a0) || !probe_vector(c, a1) || !dout) return refuse("two of the vectors 0 .. 6 and a place for the sums");
        break;
    case FEMSHELL_KSTEP_SCALAR_STEP: {
        const int32_t nsums = args[0], phase = args[1], np = args[2], len3 = args[3], gate = args[4];
        if (nsums < 1 || nsums > 3) return refuse("nsums is 1 .. 3");
        if (phase < (int)CG_PHASE_NONE || phase > (int)CG_PHASE_FLEX_WARM) return refuse("no such phase");
        if (gate < -1 || gate > (int)CG_PHASE_FLEX_WARM) return refuse("no such gate phase");
        if (np < 0 || np > 2 * G) return refuse("n_partials is 0 .. 2 G");
        const int64_t each = np > 0 ? np : G, cap = (int64_t)c->partials.n;
        if (nsums == 3 ? (len3 < 1 || 2 * each + len3 > cap) : (len3 < 0 || nsums * each > cap)) return refuse("the partial sums named lie outside the 4 G doubles of the context");
        break;
    }
    case FEMSHELL_KSTEP_CG_DIRECTION:
    case FEMSHELL_KSTEP_CGCG_INIT:
    case FEMSHELL_KSTEP_PCG_INIT:
    case FEMSHELL_KSTEP_PCG_UPDATE:
    case FEMSHELL_KSTEP_PCG_NORM:
    case FEMSHELL_KSTEP_PCG_DOTS:
    case FEMSHELL_KSTEP_MINV_APPLY_NORM:
    case FEMSHELL_KSTEP_COPY_Z_TO_P:
        break;
    default:
        return refuse("no such step");
    }
    CommWatch watch(c->cfg.rank, c->comm.active() ? c->cfg.world_size : 1, "femshell_krylov_launch (halo exchange and all-reduce of one step)");
    const CgVectors v = probe_vectors(c);
    invalidate(c, Change::krylov_probe);
    int n_partials = 0;
    switch (step) {
    case FEMSHELL_KSTEP_CG_INIT: launch_cg_init(m, v, a0 != 0, st); break;
    case FEMSHELL_KSTEP_CG_UPDATE: launch_cg_update(m, v, st, a0 != 0); break;
    case FEMSHELL_KSTEP_CG_DIRECTION: launch_cg_direction(m, v, st); break;
    case FEMSHELL_KSTEP_CGCG_INIT: launch_cgcg_init(m, v, st); break;
    case FEMSHELL_KSTEP_CGCG_UPDATE: launch_cgcg_update(m, v, st, a0, a1 != 0); break;
    case FEMSHELL_KSTEP_PCG_INIT: launch_pcg_init(m, v, st); break;
    case FEMSHELL_KSTEP_PCG_UPDATE: launch_pcg_update(m, v, st); break;
    case FEMSHELL_KSTEP_PCG_UPDATE_START: {
        // (the arguments cg_amg gives it)
        AmgLevel &L0 = *c->amg->levels[0];
        const DeviceMatrix &S0 = L0.smooth_ready ? L0.smooth_dm : m;
        const bool d32_0 = S0.symmetric && S0.vals32 != nullptr && S0.vec32 == 2;
        launch_pcg_update_start(S0, v, L0.d.p, amg_apply_iterate(c, v.z), L0.inv_theta, a0 != 0, d32_0, st);
        break;
    }
    case FEMSHELL_KSTEP_PCG_NORM: launch_pcg_norm(m, v, st); break;
    case FEMSHELL_KSTEP_PCG_DOTS: launch_pcg_dots(m, v, st); break;
    case FEMSHELL_KSTEP_MINV_APPLY_NORM: launch_minv_apply_norm(m, v.q, v.z, v.partials, st); break;
    case FEMSHELL_KSTEP_PRODUCT:
        rc = a0 ? spmv_with_halo(c, v, v.z, v.q, v.partials + 2 * (size_t)G, &n_partials, a1 != 0)
                : spmv_with_halo(c, v, v.p, v.q, v.partials, &n_partials, a1 != 0);
        break;
    case FEMSHELL_KSTEP_SYM_GATHER: launch_sym_gather(m, v.q, nullptr, 1.0, v.s, st); break;
    case FEMSHELL_KSTEP_TWO_DOTS: rc = two_squared_norms(c, probe_vector(c, a0), probe_vector(c, a1), n6, dout); break;
    case FEMSHELL_KSTEP_SCALAR_STEP: rc = scalar_step(c, v, args[0], (CgPhase)args[1], rtol, args[2], args[3], args[4]); break;
    case FEMSHELL_KSTEP_PC_APPLY: rc = amg_apply(c, v.r, v.z, v.s, a0 != 0); break;
    case FEMSHELL_KSTEP_COPY_Z_TO_P: launch_copy(v.z, v.p, n6, v.s, st); break;
    default: break;
    }
    if (rc) return rc;
    FS_HIP(hipStreamSynchronize(st));
    FS_HIP(hipGetLastError());
    if (iout) {
        iout[0] = n_partials;
        iout[1] = G;
    }
    return FEMSHELL_OK;
}

int femshell_cg_reduce(femshell_ctx *c, int32_t n_partials, int32_t nsums, int32_t len3, const double *partials, double *red_out,
                       uint32_t *ticket_out)
{
    if (!c || !partials || !red_out || !ticket_out) return set_err(FEMSHELL_ERR_INVALID, "femshell_cg_reduce: null argument");
    if (n_partials < 1 || n_partials > (1 << 20)) return set_err(FEMSHELL_ERR_INVALID, "femshell_cg_reduce: n_partials is 1 .. 2^20");
    if (nsums < 1 || nsums > 3) return set_err(FEMSHELL_ERR_INVALID, "femshell_cg_reduce: nsums is 1 .. 3");
    if (nsums == 3 && (len3 < 1 || len3 > n_partials)) return set_err(FEMSHELL_ERR_INVALID, "femshell_cg_reduce: len3 is 1 .. n_partials");
    int rc = select_device(c);
    if (rc) return rc;
    hipStream_t st = c->stream;
    // (a buffer of this call alone, of the caller's size, and scalars of the probe's own: the context's partial sums and scalars are
    //  not touched.  The scalars are zeroed once and then kept: every launch starts from the ticket and the stage-1 sums the last one
    //  left, as the launches of a solve do; red[] is filled with NaN in front, so that a sum nobody wrote shows)
    const size_t words = nsums == 3 ? 2 * (size_t)n_partials + (size_t)len3 : (size_t)nsums * (size_t)n_partials;
    DevBuf<double> part;
    DevBuf<CgScalars> &scal = c->probe_scal;
    FS_HIP(part.alloc(words));
    if (!scal.p) {
        FS_HIP(scal.alloc(1));
        FS_HIP(scal.zero(st));
    }
    const double nan3[3] = {std::nan(""), std::nan(""), std::nan("")};
    FS_HIP(hipMemcpyAsync(reinterpret_cast<char *>(scal.p) + offsetof(CgScalars, red), nan3, sizeof nan3, hipMemcpyHostToDevice, st));
    FS_HIP(hipMemcpyAsync(part.p, partials, words * sizeof(double), hipMemcpyHostToDevice, st));
    CgVectors v;
    v.partials = part.p;
    v.s = scal.p;
    launch_cg_scalar(c->dm, v, true, nsums, CG_PHASE_NONE, 0.0, st, n_partials, len3, -1);
    FS_HIP(hipGetLastError());
    CgScalars hs{};
    FS_HIP(hipMemcpyAsync(&hs, scal.p, sizeof hs, hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st));
    FS_HIP(hipGetLastError());
    for (int a = 0; a < 3; a++) red_out[a] = hs.red[a];
    *ticket_out = hs.ticket;
    return FEMSHELL_OK;
}

} // extern "C"
