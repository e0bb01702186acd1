// api_state.cpp -- the derived state of a context (derived.hpp): the one place that says what is valid.
// invalidate() applies the table of derived.hpp after a change, the functions below it make a product valid, ensure() brings
// what an entry point needs up to date, have() answers for the entry points that refuse instead.  No other file assigns to
// matrix_valid, rhs_valid, jacobi_valid, mass_valid, ubar_valid, have_element_loads, have_alpha, have_thermal, have_foundation, have_springs or amg_fp64_only or drops the hierarchy; have_solution and
// warm_next are set where a solve and a hand-over produce them (api.cpp, api_dynamics.cpp) and cleared here only.
#include "api_internal.hpp"

#include <chrono>

using namespace femshell;

namespace femshell {

void invalidate(femshell_ctx *c, Change what)
{
    const uint32_t stale = stale_after(what);
    if (what == Change::mesh) c->have_mesh = false;
    if (stale & kK) c->matrix_valid = false;
    if (stale & kF) c->rhs_valid = false;
    if (stale & kJacobi) c->jacobi_valid = false;
    if (stale & kHierarchy) c->amg.reset(); // (its HBM goes back at once)
    if (stale & kMass) c->mass_valid = false;
    if (stale & kUbar) c->ubar_valid = false;
    if (stale & kSolution) c->have_solution = false;
    if (stale & kWarmStart) c->warm_next = false;
    if (stale & kFp64Only) c->amg_fp64_only = false;
    if (what == Change::fp64_fallback) c->amg_fp64_only = true;
}

bool have(const femshell_ctx *c, uint32_t products)
{
    if (!c->have_mesh) return false;
    const uint32_t valid = (c->matrix_valid ? kK : 0) | (c->rhs_valid ? kF : 0) | (c->jacobi_valid ? kJacobi : 0) |
                           ((c->amg && c->amg->valid) ? kHierarchy : 0) | (c->mass_valid ? kMass : 0) | (c->ubar_valid ? kUbar : 0) |
                           (c->have_solution ? kSolution : 0);
    return (products & ~valid) == 0;
}

// status and timing of an assembly that femshell_assemble_async enqueued (nothing where none is pending): every entry point that
// reads results, changes inputs or synchronises calls this first
int finish_pending_assembly(femshell_ctx *c)
{
    if (!c->assembly_pending) return FEMSHELL_OK;
    c->assembly_pending = false;
    int rc = select_device(c);
    if (rc) return rc;
    rc = check_and_agree(c, "femshell_assemble_async");
    if (rc) {
        invalidate(c, Change::matrix_spoiled);
        return rc;
    }
    float ms = 0.f;
    FS_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->last_assemble_s = 1e-3 * ms;
    return FEMSHELL_OK;
}

// femshell_set_mesh and femshell_set_sections forget the densities (the mass matrix in HBM goes with their entry of the table)
void forget_density(femshell_ctx *c)
{
    c->have_density = false;
    c->rho = 0.0;
    c->sec_rho.clear();
}

// ---- element loads (femshell_set_element_loads, api_element_loads.cpp).  The invariant every consumer of the loads stands on:
// c->loads in HBM holds nodal + S, S the nodal equivalents of the element loads in force (zero without), so do_rhs, the assembly's
// rhs_loads, femshell_reactions and the Newmark right-hand side read one buffer as before.  While element loads are in force
// the nodal part lies beside it in c->loads_nodal, and whoever rewrites the nodal loads writes there (nodal_loads_buffer) and
// calls combine_loads.

// Temperatures (femshell_set_thermal, api_thermal.cpp) add T, the work-equivalent loads of the free thermal state: c->loads holds
// (nodal + S) + T, one rounding per +.  The nodal part lies in c->loads_nodal while either is in force; where both are, the two
// kernels chain through c->loads_mech = nodal + S.

// femshell_set_mesh forgets the element loads: the flag, their buffers and the map of the previous mesh's lists
void forget_element_loads(femshell_ctx *c)
{
    c->have_element_loads = false;
    c->loads_nodal.release();
    c->loads_mech.release();
    c->elem_load.release();
    c->slice_elem_local.release();
}

// ... and the temperatures and alpha (the loads are zeroed by the mesh: nothing to restore)
void forget_thermal(femshell_ctx *c)
{
    c->have_thermal = false;
    c->have_alpha = false;
    c->alpha = 0.0;
    c->sec_alpha.clear();
    c->elem_temp.release();
    c->loads_mech.release();
    c->sec_thermal.release();
    if (!c->have_element_loads) c->loads_nodal.release();
}

// where an upload of the nodal loads goes (n_pad x 6, allocated here)
int nodal_loads_buffer(femshell_ctx *c, double **buf)
{
    DevBuf<double> &b = (c->have_element_loads || c->have_thermal) ? c->loads_nodal : c->loads;
    FS_HIP(b.alloc((size_t)c->plan.n_pad * 6));
    *buf = b.p;
    return FEMSHELL_OK;
}

// the slices' element lists as local element indices in HBM (Plan::slice_elems): once per mesh, at the first use
int ensure_slice_elem_local(femshell_ctx *c)
{
    if (c->slice_elem_local.p) return FEMSHELL_OK;
    FS_HIP(c->slice_elem_local.upload(c->plan.slice_elems, c->stream)); // (the plan outlives the stream's work)
    return FEMSHELL_OK;
}

// the factors of a material with expansion alpha (kernels.hpp ThermalSec): tcm = t E / (1 - nu^2), cp = E t^3 / (12 (1 - nu^2))
static ThermalSec thermal_factors(double tcm, double cp, double nu, double t, double alpha)
{
    ThermalSec r;
    r.nt = tcm * (1.0 + nu) * alpha;
    r.mt = cp * (1.0 + nu) / t * alpha;
    r.alpha = alpha;
    r.alpha_t = alpha / t;
    return r;
}

// what the kernels get of the temperatures in force
ThermalView thermal_view(const femshell_ctx *c)
{
    ThermalView tv;
    tv.elem_temp = reinterpret_cast<const double2 *>(c->elem_temp.p);
    tv.uni = thermal_factors(c->mc.t * c->mc.cm, c->mc.cp, c->mc.nu, c->mc.t, c->alpha);
    tv.sec = c->have_sections ? c->sec_thermal.p : nullptr;
    return tv;
}
const ThermalView *thermal_view_or_null(const femshell_ctx *c, ThermalView *store)
{
    if (!c->have_thermal) return nullptr;
    *store = thermal_view(c);
    return store;
}

// c->loads = (nodal + S) + T, a launch each; nothing with neither in force (c->loads is the nodal part itself then)
int combine_loads(femshell_ctx *c)
{
    if (!c->have_element_loads && !c->have_thermal) return FEMSHELL_OK;
    const double *src = c->loads_nodal.p;
    if (c->have_element_loads) {
        double *dst = c->loads.p;
        if (c->have_thermal) {
            FS_HIP(c->loads_mech.alloc((size_t)c->plan.n_pad * 6));
            dst = c->loads_mech.p;
        }
        launch_element_loads(c->dm, c->slice_elem_local.p, c->elem_load.p, src, dst, c->stream);
        src = dst;
    }
    if (c->have_thermal) launch_element_thermal(c->dm, c->slice_elem_local.p, c->ds.slice_elem_section, thermal_view(c), src, c->loads.p, c->stream);
    FS_HIP(hipGetLastError());
    return FEMSHELL_OK;
}

// the first of the two that takes force moves the nodal part aside inside HBM
static int move_nodal_aside(femshell_ctx *c)
{
    if (c->have_element_loads || c->have_thermal) return FEMSHELL_OK;
    const size_t n6 = (size_t)c->plan.n_pad * 6;
    FS_HIP(c->loads_nodal.alloc(n6));
    if (n6) FS_HIP(hipMemcpyAsync(c->loads_nodal.p, c->loads.p, n6 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return FEMSHELL_OK;
}

// one of the two left force: the chain again, or, with neither left, the nodal part back into c->loads.  Synchronises.
static int loads_after_clear(femshell_ctx *c)
{
    c->loads_mech.release();
    if (c->have_element_loads || c->have_thermal) {
        const int rc = combine_loads(c);
        if (rc) return rc;
        FS_HIP(hipStreamSynchronize(c->stream));
        return FEMSHELL_OK;
    }
    const size_t n6 = (size_t)c->plan.n_pad * 6;
    if (n6) FS_HIP(hipMemcpyAsync(c->loads.p, c->loads_nodal.p, n6 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    FS_HIP(hipStreamSynchronize(c->stream));
    c->loads_nodal.release();
    return FEMSHELL_OK;
}

// rows: four doubles per local element, which take force in place of the previous set.  The first set moves the nodal part
// aside inside HBM; no set uploads it again.  Returns after the upload of `rows` has completed.
int element_loads_apply(femshell_ctx *c, const RawVec<double> &rows)
{
    hipStream_t st = c->stream;
    int rc = ensure_slice_elem_local(c);
    if (rc) return rc;
    rc = move_nodal_aside(c);
    if (rc) return rc;
    FS_HIP(c->elem_load.upload(rows, st));
    c->have_element_loads = true;
    rc = combine_loads(c);
    if (rc) return rc;
    FS_HIP(hipStreamSynchronize(st));
    invalidate(c, Change::loads);
    return FEMSHELL_OK;
}

// no element loads any more: the loads are nodal + T, or the nodal part goes back into c->loads
int element_loads_clear(femshell_ctx *c)
{
    if (!c->have_element_loads) return FEMSHELL_OK;
    c->have_element_loads = false;
    const int rc = loads_after_clear(c);
    if (rc) return rc;
    c->elem_load.release();
    invalidate(c, Change::loads);
    return FEMSHELL_OK;
}

// femshell_set_expansion, checked: alpha for every element, or one per section.  The factors of the sections go to HBM; where
// temperatures are in force the loads follow.
int expansion_apply(femshell_ctx *c, double alpha, int32_t n_sections, const double *section_alpha)
{
    hipStream_t st = c->stream;
    if (c->have_sections) {
        std::vector<ThermalSec> table((size_t)c->n_sections);
        for (int32_t s = 0; s < c->n_sections; s++) {
            const double nu = c->sec_nu[(size_t)s], E = c->sec_E[(size_t)s], t = c->sec_thickness[(size_t)s];
            table[(size_t)s] = thermal_factors(t * (E / (1.0 - nu * nu)), E * t * t * t / (12.0 * (1.0 - nu * nu)), nu, t,
                                               n_sections > 0 ? section_alpha[s] : alpha);
        }
        FS_HIP(hipStreamSynchronize(st)); // (a launch in flight reads the table that is replaced)
        FS_HIP(c->sec_thermal.upload(table, st));
        FS_HIP(hipStreamSynchronize(st)); // the host table goes out of scope
    }
    c->alpha = n_sections > 0 ? 0.0 : alpha;
    if (n_sections > 0) c->sec_alpha.assign(section_alpha, section_alpha + n_sections);
    else c->sec_alpha.clear();
    c->have_alpha = true;
    if (c->have_thermal) {
        const int rc = combine_loads(c);
        if (rc) return rc;
        FS_HIP(hipStreamSynchronize(st));
        invalidate(c, Change::loads);
    }
    return FEMSHELL_OK;
}

// rows: (Tm, Tg) per local element, which take force in place of the previous set: 16 bytes per local element go to HBM, the
// nodal loads are not uploaded again.  Returns after the upload of `rows` has completed.
int thermal_apply(femshell_ctx *c, const RawVec<double> &rows)
{
    hipStream_t st = c->stream;
    int rc = ensure_slice_elem_local(c);
    if (rc) return rc;
    rc = move_nodal_aside(c);
    if (rc) return rc;
    FS_HIP(c->elem_temp.upload(rows, st));
    c->have_thermal = true;
    rc = combine_loads(c);
    if (rc) return rc;
    FS_HIP(hipStreamSynchronize(st));
    invalidate(c, Change::loads);
    return FEMSHELL_OK;
}

// no temperatures any more: the loads are nodal + S again
int thermal_clear(femshell_ctx *c)
{
    if (!c->have_thermal) return FEMSHELL_OK;
    c->have_thermal = false;
    const int rc = loads_after_clear(c);
    if (rc) return rc;
    c->elem_temp.release();
    invalidate(c, Change::loads);
    return FEMSHELL_OK;
}

// femshell_set_sections forgets alpha, which belongs to the sections as the densities do, and with it the temperatures
int thermal_forget_and_restore(femshell_ctx *c)
{
    const int rc = thermal_clear(c);
    if (rc) return rc;
    c->have_alpha = false;
    c->alpha = 0.0;
    c->sec_alpha.clear();
    c->sec_thermal.release();
    return FEMSHELL_OK;
}

// ---- elastic supports (femshell_set_foundation, femshell_set_springs, api_elastic_support.cpp).  The invariant:
// while a foundation or springs are in force c->support holds the table k_support_rows made of them, and every assembly adds it
// to the diagonal blocks of K behind the assembly kernel (support_add below).  A change of either set is a change of K that the
// table of derived.hpp has no row of its own for: it is reported as Change::matrix_spoiled -- K, F, block-Jacobi and the
// hierarchy, exactly what is stale -- and the next use assembles again.  (No subtraction in place: K + S - S is not K bit for bit.)

// femshell_set_mesh forgets both sets, their buffers and the table
void forget_supports(femshell_ctx *c)
{
    c->have_foundation = c->have_springs = false;
    c->elem_found.release();
    c->spring.release();
    c->support.release();
    c->sup_scratch.release();
}

// the table of what is in force, once per change of its inputs; with nothing in force its buffers go back.  Synchronises.
static int supports_changed(femshell_ctx *c)
{
    hipStream_t st = c->stream;
    if (!c->have_supports()) {
        FS_HIP(hipStreamSynchronize(st));
        c->support.release();
        c->sup_scratch.release();
    } else {
        if (c->have_foundation) {
            const int rc = ensure_slice_elem_local(c);
            if (rc) return rc;
        }
        FS_HIP(c->support.alloc((size_t)std::max(c->dm.n_slices * kSliceNodes, c->plan.n_pad) * 9));
        launch_support_rows(c->dm, c->slice_elem_local.p, c->have_foundation ? c->elem_found.p : nullptr, c->have_springs ? c->spring.p : nullptr,
                            c->support.p, st);
        FS_HIP(hipGetLastError());
        FS_HIP(hipStreamSynchronize(st)); // (the caller's host rows go out of scope)
    }
    invalidate(c, Change::matrix_spoiled);
    return FEMSHELL_OK;
}

// rows: (kn, kt) per local element, which take force in place of the previous set
int foundation_apply(femshell_ctx *c, const RawVec<double> &rows)
{
    FS_HIP(hipStreamSynchronize(c->stream)); // (a launch in flight may read the rows that are replaced)
    FS_HIP(c->elem_found.upload(rows, c->stream));
    c->have_foundation = true;
    return supports_changed(c);
}

int foundation_clear(femshell_ctx *c)
{
    if (!c->have_foundation) return FEMSHELL_OK;
    c->have_foundation = false;
    const int rc = supports_changed(c);
    c->elem_found.release();
    return rc;
}

// rows: six doubles per row of the rank (n_pad x 6, zero on the padding rows), which take force in place of the previous set
int springs_apply(femshell_ctx *c, const RawVec<double> &rows)
{
    FS_HIP(hipStreamSynchronize(c->stream));
    FS_HIP(c->spring.upload(rows, c->stream));
    c->have_springs = true;
    return supports_changed(c);
}

int springs_clear(femshell_ctx *c)
{
    if (!c->have_springs) return FEMSHELL_OK;
    c->have_springs = false;
    const int rc = supports_changed(c);
    c->spring.release();
    return rc;
}

// K in HBM becomes K + mask(K_sup): behind the assembly kernel, in front of the mass shift of an active dynamics.  Nothing
// without supports.
static void support_add(femshell_ctx *c)
{
    if (c->have_supports()) launch_support_add(c->dm, c->support.p, c->stream);
}

// u_bar of the prescribed values and the Dirichlet set in force (femshell_set_prescribed): the entries at fixed dofs, zero
// elsewhere, on the host and in HBM.  Single-rank contexts only: the owned rows are all rows.
int resolve_prescribed(femshell_ctx *c)
{
    if (c->ubar_valid) return FEMSHELL_OK;
    const Plan &p = c->plan;
    c->ubar_host.assign((size_t)p.n_nodes * 6, 0.0);
    bool nonzero = false;
    for (int32_t a = 0; a < p.n_nodes; a++) {
        const uint32_t fixed = c->dmask_global[(size_t)a];
        for (int v = 0; v < 6 && fixed; v++)
            if ((fixed >> v) & 1u) {
                const double val = c->prescribed_global[6ull * (size_t)a + v];
                c->ubar_host[6ull * (size_t)a + v] = val;
                nonzero = nonzero || val != 0.0;
            }
    }
    FS_HIP(c->ubar.alloc((size_t)p.n_local_nodes() * 6));
    FS_HIP(c->ubar.zero(c->stream));
    FS_HIP(hipMemcpyAsync(c->ubar.p, c->ubar_host.data(), (size_t)p.n_own * 6 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    FS_HIP(hipStreamSynchronize(c->stream));
    c->ubar_nonzero = nonzero;
    c->ubar_valid = true;
    return FEMSHELL_OK;
}

static int do_rhs(femshell_ctx *c)
{
    if (c->have_prescribed) {
        // F = mask(loads - K_unc u_bar): one launch of the matrix-free product with the unconstrained element matrices, the
        // masked combine in its epilogue.  (No fixed dof carries a non-zero value: the masked copy below, as without the call.)
        const int rc = resolve_prescribed(c);
        if (rc) return rc;
        if (c->ubar_nonzero) {
            const double *sub = c->loads.p;
            if (c->have_supports()) { // F = mask((loads - K_sup u_bar) - K_unc u_bar): the supports' part first, into a scratch vector
                FS_HIP(c->sup_scratch.alloc((size_t)c->plan.n_pad * 6));
                launch_support_apply(c->dm, c->support.p, c->ubar.p, nullptr, c->loads.p, -1.0, c->sup_scratch.p, c->stream);
                sub = c->sup_scratch.p;
            }
            launch_element_product(c->dm, c->mc, c->sections_or_null(), c->ubar.p, nullptr, sub, c->F.p, true, c->stream);
            FS_HIP(hipGetLastError());
            c->rhs_valid = true;
            return FEMSHELL_OK;
        }
    }
    launch_rhs(c->dm, c->loads.p, c->F.p, c->stream);
    FS_HIP(hipGetLastError());
    c->rhs_valid = true;
    return FEMSHELL_OK;
}

int do_assemble(femshell_ctx *c, bool wait)
{
    if (!c->have_mesh) return set_err(FEMSHELL_ERR_INVALID, "femshell_assemble: no mesh set");
    TraceRange trace("femshell_assemble");
    CommWatch watch(c->cfg.rank, c->comm.active() ? c->cfg.world_size : 1, "femshell_assemble (agreement of the ranks on the outcome)");
    int rc = select_device(c);
    if (rc) return rc;
    if (c->assembly_pending && wait) { // (async after async: one status word collects both)
        rc = finish_pending_assembly(c);
        if (rc) return rc;
    }
    // (the event pair costs the synchronous call its two records: without it assemble_seconds is the host's clock around launch
    //  and synchronisation; an enqueued assembly always carries the pair -- nobody else could time it)
    // (MEASURED, round 6, profiles/r06_sync_step_ab_raw.txt: neither the status word in mapped host memory, nor dropping the event
    //  pair, nor polling a word that a one-lane kernel writes behind the assembly instead of synchronising the stream, nor polled
    //  completion signals move the 40-50 us a synchronous step costs beyond its kernel: it is launch latency on an idle queue)
    const bool events = c->asm_events || !wait;
    const auto t_host = std::chrono::steady_clock::now();
    if (events) FS_HIP(hipEventRecord(c->ev0, c->stream));
    c->dm.rhs_loads = c->loads.p;
    c->dm.rhs_F = c->F.p;
    if (!launch_assemble(c->dm, c->mc, c->stream, c->sections_or_null())) // K and F (k_rhs alone serves changes of the loads)
        return set_err(FEMSHELL_ERR_INVALID, "femshell_assemble: the context's sections have no table in HBM");
    support_add(c); // (elastic supports in force: K + mask(K_sup), inside the event pair)
    // (dynamics is active: the matrix in HBM is K_eff = K + shift M, also when K is built again -- FEMSHELL_REASSEMBLE_EACH_SOLVE)
    if (c->dyn.active) launch_mass_shift(c->dm, c->mass.p, c->dyn.k.shift, c->stream);
    if (events) FS_HIP(hipEventRecord(c->ev1, c->stream));
    FS_HIP(hipGetLastError());
    if (c->have_prescribed) { // (the assembly kernel wrote the masked loads: F of the prescribed values behind it)
        rc = do_rhs(c);
        if (rc) return rc;
    }
    if (wait) {
        rc = check_and_agree(c, "femshell_assemble");
        if (rc) return rc;
        if (events) {
            float ms = 0.f;
            FS_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
            c->last_assemble_s = 1e-3 * ms;
        } else {
            c->last_assemble_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_host).count();
        }
    } else {
        c->assembly_pending = true; // (a failed element leaves its mark in the status word until someone looks)
    }
    invalidate(c, Change::assembled); // block-Jacobi and the multigrid hierarchy belong to the previous K
    c->matrix_valid = true;
    c->rhs_valid = true;
    return FEMSHELL_OK;
}

// femshell_time_kernel launched the assembly kernel itself, between its event pair: the call ends in the transition of
// do_assemble.  While dynamics is active the shift is added once, so that HBM holds K_eff as the next step expects.  F is what it
// was (the kernel rewrites the masked loads) unless prescribed values are in force, which that overwrites.
int timed_assembly_done(femshell_ctx *c)
{
    support_add(c); // (once behind the last of the timed launches, as behind every assembly)
    if (c->dyn.active) launch_mass_shift(c->dm, c->mass.p, c->dyn.k.shift, c->stream);
    if (c->dyn.active || c->have_supports()) FS_HIP(hipGetLastError());
    const int rc = check_status(c, "femshell_time_kernel");
    if (rc) return rc;
    invalidate(c, Change::assembled);
    c->matrix_valid = true;
    if (c->have_prescribed) c->rhs_valid = false;
    return FEMSHELL_OK;
}

static int do_jacobi(femshell_ctx *c)
{
    TraceRange trace("femshell block-Jacobi setup");
    FS_HIP(hipEventRecord(c->ev0, c->stream));
    launch_block_jacobi(c->dm, c->stream);
    FS_HIP(hipEventRecord(c->ev1, c->stream));
    FS_HIP(hipGetLastError());
    int rc = check_and_agree(c, "block-Jacobi setup");
    if (rc) return rc;
    float ms = 0.f;
    FS_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->last_setup_s = 1e-3 * ms;
    c->jacobi_valid = true;
    return FEMSHELL_OK;
}

// the diagonal of the lumped mass matrix of the owned rows in HBM (c->mass), computed where it is not there yet
static int ensure_mass(femshell_ctx *c)
{
    if (c->mass_valid) return FEMSHELL_OK;
    const Plan &p = c->plan;
    hipStream_t st = c->stream;
    FS_HIP(c->mass.alloc((size_t)p.n_pad * 6));
    const double2 *sec = nullptr;
    if (c->have_sections) {
        std::vector<double2> table((size_t)c->n_sections);
        for (int32_t s = 0; s < c->n_sections; s++) {
            const double rho = c->sec_rho.empty() ? c->rho : c->sec_rho[(size_t)s], t = c->sec_thickness[(size_t)s];
            table[(size_t)s] = make_double2(rho * t, rho * t * t * t / 12.0);
        }
        FS_HIP(c->sec_mass.upload(table, st));
        FS_HIP(hipStreamSynchronize(st)); // the host table goes out of scope
        sec = c->sec_mass.p;
    }
    const double t = c->cfg.thickness;
    launch_lumped_mass(c->dm, make_double2(c->rho * t, c->rho * t * t * t / 12.0), sec, c->ds.slice_elem_section, c->mass.p, st);
    FS_HIP(hipGetLastError());
    c->mass_valid = true;
    return FEMSHELL_OK;
}

// The multigrid hierarchy of the K in HBM, built where there is none (first solve, K changed, the all-FP64 rebuild): on one rank,
// or row-partitioned and collective when the context has a communicator.  *pc_setup_s += its seconds.
static int ensure_amg_hierarchy(femshell_ctx *c, double *pc_setup_s)
{
    if (c->amg && c->amg->valid) return FEMSHELL_OK;
    int rc = FEMSHELL_OK;
    if (c->comm.active()) {
        const double t0 = wall_s();
        // row-partitioned hierarchy (amg_dist.cpp); a failure only one rank sees must reach the others
        rc = agree_status(c, amg_setup_dist(c), "multigrid setup", true);
        if (rc) {
            c->amg.reset();
            return rc;
        }
        *pc_setup_s += wall_s() - t0;
    } else {
        rc = amg_setup(c);
        if (rc) {
            c->amg.reset();
            return rc;
        }
        *pc_setup_s += c->amg->setup_seconds;
    }
    return rc;
}

int ensure(femshell_ctx *c, uint32_t need, Timings *t, bool solving)
{
    Timings unused;
    if (!t) t = &unused;
    int rc = FEMSHELL_OK;
    // (the mass first: it depends on nothing here, and K_eff of an active dynamics is built with it)
    if ((need & kMass) && (rc = ensure_mass(c))) return rc;
    if ((need & kK) && (!c->matrix_valid || (solving && (c->cfg.flags & FEMSHELL_REASSEMBLE_EACH_SOLVE)))) {
        if ((rc = do_assemble(c))) return rc; // (F with it)
        t->assemble_s += c->last_assemble_s;
    }
    if ((need & kF) && !c->rhs_valid && (rc = do_rhs(c))) return rc;
    if ((need & kJacobi) && !c->jacobi_valid) {
        if ((rc = do_jacobi(c))) return rc;
        t->setup_s += c->last_setup_s;
    }
    if (need & kHierarchy) rc = ensure_amg_hierarchy(c, &t->pc_setup_s);
    return rc;
}

} // namespace femshell
