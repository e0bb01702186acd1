// context.hpp -- what the translation units of libfemshell share: error reporting, device buffers, the context
// behind a femshell_ctx handle and the CG driver's entry points (cg_driver.cpp).
#pragma once
#include <cstdio>

#include "femshell.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <iterator>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "comm.hpp"
#include "dev_pool.hpp"
#include "errors.hpp"
#include "kernels.hpp"
#include "plan.hpp"

namespace femshell {

struct Amg; // multigrid hierarchy (amg_device.hpp)

inline const char *fs_basename(const char *path)
{
    const char *b = path;
    for (const char *q = path; *q; q++)
        if (*q == '/') b = q + 1;
    return b;
}

#define FS_HIP(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return set_err(FEMSHELL_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_) +      \
                                                 " (" + fs_basename(__FILE__) + ":" + std::to_string(__LINE__) + ")"); \
    } while (0)

} // namespace femshell

struct femshell_ctx;
// zero the status word after a failure was read (mapped: by the host, behind a stream synchronisation)
int clear_status_word(femshell_ctx *c, hipStream_t st);
// the status word on the host after everything enqueued on st (mapped: no copy)
int fetch_status_word(femshell_ctx *c, hipStream_t st, int32_t *out);

struct femshell_ctx {
    // (global namespace: the opaque type of include/femshell.h)
    femshell_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int32_t *status_host = nullptr; // pinned landing place of the device status word
    // Two regions of 32 MB of pinned host memory through which the multigrid setup moves its arrays (staged_download / staged_upload
    // in amg_device_setup.cpp; region 0: the calling thread, region 1: the setup's helper thread).  Why not plain copies from and to
    // the arrays themselves: the runtime registers the pages of a large pageable copy with the driver, and a host array that is
    // FREED soon after -- the 48 MB of node normals, released when the first coarsening step is through -- takes that registration
    // down through the MMU notifier, which evicts the process's queues: the next launch on the main stream waited 24-31 ms (found
    // with FEMSHELL_AMG_VERBOSE laps around the block-Jacobi kernel of level 1; gone with the array kept, or copied through here).
    // nullptr when the allocation failed: the copies then go the pageable way.
    void *stage_host = nullptr;
    size_t stage_bytes = 0; // of ONE region
    // the status word as the kernels see it: c->status in HBM, or -- FEMSHELL_STATUS_MAPPED, the default -- the device address of
    // status_host itself (kernels write the word on failure only, with a system-scope compare-and-swap; the host reads it after the
    // stream synchronisation without a copy: 12 us of every femshell_assemble)
    int32_t *status_word = nullptr;
    bool status_mapped = false;
    bool asm_events = true; // FEMSHELL_ASM_EVENTS=0: no event pair around the assembly kernel (assemble_seconds by the host's clock)
    double *agree_host = nullptr;   // pinned word of the cross-rank agreement on a rank-local failure (api.cpp)
    femshell::DevBuf<double> agree;
    // halo exchange beside the interior SpMV (multi-rank contexts): second stream + hand-off events
    hipStream_t halo_stream = nullptr;
    // femshell_set_initial_guess: the iterate the NEXT femshell_solve starts from (owned rows, internal numbering), consumed by it
    femshell::DevBuf<double> x0;
    bool warm_next = false;
    hipStream_t aux_stream = nullptr; // the look-ahead of the dense inverse (amg_dense.hip)
    // uploads a helper thread of the multigrid setup makes beside the main stream (the node normals, amg_hierarchy.cpp): made by that
    // thread at its first use in a single-rank context and kept.  (Not at femshell_create: HIP maps streams onto four hardware queues,
    // and one stream more per context was enough, with two ranks sharing a card in the tests, for the look-ahead of the dense
    // inverse -- two streams that must run side by side -- to run into its bounded wait one time in four.)
    hipStream_t copy_stream = nullptr;
    int aux_streams_side_by_side = 0; // 0: not asked yet, 1: stream and aux_stream run concurrently, -1: they share a hardware queue
    // first-contact self-test of femshell_comm_init (comm.cpp comm_selftest): microseconds of its three patterns
    double comm_selftest_us[3] = {-1.0, -1.0, -1.0};
    bool comm_selftest_done = false;
    hipEvent_t ev_p_ready = nullptr, ev_halo_done = nullptr;
    bool halo_overlap = false;
    femshell::MatConst mc{};
    femshell::Plan plan;
    // (what is valid -- these, mass_valid, ubar_valid, amg, amg_fp64_only below -- is written by api_state.cpp only: derived.hpp)
    bool have_mesh = false, matrix_valid = false, rhs_valid = false, jacobi_valid = false, have_solution = false;

    // optional renumbering (reorder.cpp): internal node i is the caller's node perm[i]; iperm is the inverse; both empty
    // when the caller's numbering is kept.  dmask_global / loads_global and everything below are in internal numbering.
    std::vector<int32_t> perm, iperm;
    std::vector<uint8_t> dmask_global;  // n_nodes
    femshell::RawVec<double> loads_global; // n_nodes*6

    femshell::DevBuf<double> xyz, vals, minv, loads, F;
    femshell::DevBuf<int32_t> tri, quad, slice_width, cols, pair_ptr, status;
    femshell::DevBuf<int64_t> slice_base, in_base;
    femshell::DevBuf<int32_t> in_width, in_slots, in_rows; // symmetric storage: per-row lists of transposed blocks
    femshell::DevBuf<int32_t> gat_slots;                    // ... without the blocks whose product stays inside the slice
    femshell::DevBuf<uint8_t> loc_index, loc_list;
    femshell::DevBuf<double> tbuf;                          // ... and their products K_ac^T x_a (6 doubles per slot)
    femshell::DevBuf<int32_t> slice_elem_ptr, slice_elem_nodes, item_ptr, slice_desc;
    femshell::DevBuf<femshell::Plan::Item> items;
    femshell::DevBuf<uint32_t> item_flags;
    femshell::DevBuf<uint8_t> dmask;
    // shell sections (femshell_set_sections): table, index per entry of slice_elem_nodes and per local element, and the view of
    // them the kernels get.  pipe_without_sections: what femshell_set_mesh decided for the uniform material (Plan::pipe) -- a
    // context with sections packs its items for the two-phase kernel and goes back to that layout when they are cleared.
    bool have_sections = false, pipe_without_sections = false;
    int32_t n_sections = 0;
    femshell::DevBuf<femshell::SecConst> sec_table;
    femshell::DevBuf<int32_t> slice_elem_section, elem_section;
    femshell::DeviceSections ds{};
    const femshell::DeviceSections *sections_or_null() const { return have_sections ? &ds : nullptr; }
    // structural dynamics (femshell_set_density, femshell_dynamics_*).  The densities are the caller's; the diagonal of the lumped
    // mass matrix lies in HBM (owned rows, internal numbering) once it has been asked for, until mesh, sections or density change.
    std::vector<double> sec_thickness; // thickness of every section (the table in HBM keeps products only)
    std::vector<double> sec_nu, sec_E; // ... and its material, for what is derived from a section later (the thermal factors)
    bool have_density = false, mass_valid = false;
    double rho = 0.0;
    std::vector<double> sec_rho;       // per section, or empty: rho for every element
    femshell::DevBuf<double> mass;
    femshell::DevBuf<double2> sec_mass; // {rho t, rho t^3 / 12} per section
    struct Dynamics {
        bool active = false, have_candidate = false;
        femshell::NewmarkCoef k{};
        int cur = 0; // u[cur], v[cur], a[cur]: committed; [cur ^ 1]: candidate (femshell_dynamics_accept swaps)
        femshell::DevBuf<double> u[2], v[2], a[2], b, e_partials, e_sums;
        void reset() // drops the state and gives its buffers back
        {
            for (int i = 0; i < 2; i++) {
                u[i].release();
                v[i].release();
                a[i].release();
            }
            b.release();
            e_partials.release();
            e_sums.release();
            active = have_candidate = false;
            k = femshell::NewmarkCoef{};
            cur = 0;
        }
    } dyn;
    // prescribed displacements (femshell_set_prescribed): the values as the caller gave them (n_nodes x 6, internal numbering; which
    // of them count is decided by the Dirichlet set when the right-hand side is built) and u_bar in HBM -- the entries at fixed dofs,
    // zero elsewhere -- resolved by resolve_prescribed (api_state.cpp) after every change of either.  The solution vector in HBM stays the
    // homogeneous part; u_bar is added where a solution leaves the library.
    bool have_prescribed = false, ubar_valid = false, ubar_nonzero = false;
    std::vector<double> prescribed_global, ubar_host;
    femshell::DevBuf<double> ubar;
    // element loads (femshell_set_element_loads): while they are in force `loads` holds nodal + S -- what every consumer of the
    // loads reads --, loads_nodal the nodal part alone (HBM, allocated only then) and elem_load the caller's rows in the local
    // element order.  slice_elem_local: Plan::slice_elems in HBM, uploaded at the first use per mesh.  (have_element_loads is
    // written by api_state.cpp only.)
    bool have_element_loads = false;
    femshell::DevBuf<double> loads_nodal, elem_load;
    femshell::DevBuf<int32_t> slice_elem_local;
    // thermal loads (femshell_set_expansion, femshell_set_thermal): alpha of the uniform material or one per
    // section (sec_alpha, else empty), and while temperatures are in force elem_temp, (Tm, Tg) per LOCAL element.  `loads` then
    // holds (nodal + S) + T: the nodal part lies in loads_nodal as with element loads, and where both are in force the kernels
    // chain through loads_mech = nodal + S.  sec_thermal: the factors of every section in HBM (contexts with sections, from
    // femshell_set_expansion on).  (have_alpha and have_thermal are written by api_state.cpp only.)
    bool have_alpha = false, have_thermal = false;
    double alpha = 0.0;
    std::vector<double> sec_alpha;
    femshell::DevBuf<double> elem_temp, loads_mech;
    femshell::DevBuf<femshell::ThermalSec> sec_thermal;
    // elastic supports (femshell_set_foundation, femshell_set_springs): elem_found, (kn, kt) per LOCAL element, and
    // spring, six doubles per owned row, while the one or the other is in force; support, the table of nine words per slice row
    // that k_support_rows makes of them once per change (kernels.hpp), which every assembly adds to K's diagonal blocks.
    // sup_scratch: loads - K_sup u_bar of a right-hand side with prescribed values.  With neither in force no buffer exists and
    // no launch is made.  (have_foundation and have_springs are written by api_state.cpp only.)
    bool have_foundation = false, have_springs = false;
    bool have_supports() const { return have_foundation || have_springs; }
    femshell::DevBuf<double> elem_found, spring, support, sup_scratch;
    // CG state
    femshell::DevBuf<double> x, r, z, p, q, sv, partials, hist, sendbuf, ufull;
    femshell::DevBuf<double> xacc, rres; // iterative refinement of the multigrid-preconditioned solve: accumulated solution, residual
    femshell::DevBuf<femshell::CgScalars> scal;
    // femshell_krylov_* (api_krylov_probe.cpp, tests): the residual history its launches write, with the cap the caller chose
    femshell::DevBuf<double> probe_hist;
    int32_t probe_hist_cap = 0;
    // femshell_cg_reduce: its scalars, zeroed once and kept from call to call (every launch starts from the ticket the last one left)
    femshell::DevBuf<femshell::CgScalars> probe_scal;
    femshell::DevBuf<int32_t> send_nodes, spmv_order;
    std::vector<int32_t> send_offsets; // per peer, in nodes
    // scratch for femshell_time_kernel
    femshell::DevBuf<double> bx, br, bz, bp, bq, bpart;
    femshell::DevBuf<femshell::CgScalars> bscal;

    femshell::DeviceMatrix dm{};
    femshell::Comm comm;
    std::vector<int32_t> all_begin, all_end;

    femshell_pc_options pc{};           // preconditioner of femshell_solve (block-Jacobi unless set otherwise)
    // the multigrid hierarchy keeps everything FP64 (no single-precision copies, vectors or coarsest inverse): set by
    // femshell_solve after a breakdown of the flexible CG with a hierarchy that used them -- the rounded preconditioner of a
    // very thin shell is not positive definite any more --, cleared by femshell_set_mesh / femshell_set_preconditioner
    bool amg_fp64_only = false;
    std::shared_ptr<femshell::Amg> amg; // hierarchy of the multigrid preconditioner, rebuilt when K changes
    // contexts with a communicator: the centre of the WHOLE mesh, about which the rigid-body modes of the row-partitioned
    // multigrid turn on every rank alike (amg_dist.cpp; a rank's plan holds its own rows and their ghosts only)
    double mesh_centre[3] = {0.0, 0.0, 0.0};
    bool have_mesh_centre = false;

    // error estimate of the last multigrid-preconditioned solve (femshell_solve_info, cg_amg)
    struct RefineStats {
        int32_t passes = 0;
        double correction_rel = -1.0, residual_reduction = 0.0;
    } refine;
    femshell::DevBuf<double> dots_scratch;

    double last_assemble_s = 0.0, last_setup_s = 0.0;
    bool assembly_pending = false; // femshell_assemble_async: status word and timing of the last assembly not collected yet
    std::vector<double> hist_host;
    int32_t last_iters = 0;
};

namespace femshell {

CgVectors cg_vectors(femshell_ctx *c);
// pack + grouped send/recv of the ghost entries of vec (owned | padding | ghosts) on stream st
int halo_exchange(femshell_ctx *c, double *vec, hipStream_t st);
// yout = K xin with the halo exchange beside the interior slices (xin carries ghost space); partial sums of xin.yout when
// partials != nullptr (*n_partials of them, 0 = slice_grid); defer_gather: symmetric storage, the caller's next kernel
// collects the transposed products
// (vals32: the products read this single-precision copy of K's values -- smoothing products of the multigrid cycle)
int spmv_with_halo(femshell_ctx *c, const CgVectors &v, double *xin, double *yout, double *partials, int *n_partials,
                   bool defer_gather = false, const float *vals32 = nullptr, int vec32 = 0);
// the two recurrences (cg_driver.cpp); the CG state is left in the context's vectors and scalars
int cg_classic(femshell_ctx *c, const CgVectors &v, double rtol, int32_t max_it, const double *x0 = nullptr);
int cg_single_reduction(femshell_ctx *c, const CgVectors &v, double rtol, int32_t max_it);
bool use_single_reduction(const femshell_ctx *c);
// reduction of the partial sums [+ all-reduce on contexts with a communicator] + scalar step
int scalar_step(femshell_ctx *c, const CgVectors &v, int nsums, CgPhase phase, double rtol, int n_partials = 0, int len3 = 0,
                int gate_phase = -1);

} // namespace femshell
