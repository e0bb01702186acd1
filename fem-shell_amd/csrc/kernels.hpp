// kernels.hpp -- host-callable launchers of the gfx950 kernels: assembly (kernels.hip), sparse products (spmv_kernels.hip),
// conjugate gradients (cg_kernels.hip), structural dynamics (dynamics_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "shell_element.hpp"

namespace femshell {

constexpr int32_t kStatusDirect = 0x40000000; // status values above this carry a local element id directly
// constraint word of an assembly work item (DeviceMatrix::item_flags, k_item_flags): width of the contribution count and
// the bit that marks a diagonal slot.  23 bits in all: the pipelined layout keeps the word in item.w above the 9 bits of
// the wave word (assemble_kernel.hpp kPipeFlagShift).
constexpr uint32_t kFlagValenceMask = 1023u;
constexpr int kFlagDiagBit = 22;

// Device view of the mesh + matrix structure of one rank (see plan.hpp for the layout).
struct DeviceMatrix {
    int32_t n_own = 0, n_pad = 0, n_ghost = 0, n_slices = 0;
    int32_t n_ltri = 0, n_lquad = 0;
    const double *xyz = nullptr;        // (n_pad+n_ghost) x 3
    const int32_t *tri = nullptr;       // n_ltri x 3, local node ids
    const int32_t *quad = nullptr;      // n_lquad x 4
    const int32_t *slice_width = nullptr;
    const int64_t *slice_base = nullptr;
    const int32_t *cols = nullptr;      // per slot
    const int32_t *pair_ptr = nullptr;  // per slot + 1
    const int32_t *slice_elem_ptr = nullptr; // n_slices+1
    const int4 *slice_desc = nullptr;        // 2 per slice: {elem begin, elem count, item begin, item count},
                                             // {slot base lo, hi, width, 0} -- what k_assemble needs of a slice
    const int4 *slice_elem_nodes = nullptr;  // per slice element: its local node ids (w = -1 for TRI3)
    int32_t max_slice_elems = 0;
    int32_t max_slice_width = 0;             // widest slice (block slots per node row)
    const int32_t *item_ptr = nullptr;       // n_slices+1
    const uint4 *items = nullptr;            // assembly work items (plan.hpp)
    uint32_t *item_flags = nullptr;          // per item: what its owner lane needs to know about the slot besides the
                                             // contributions (k_item_flags): Dirichlet mask of the row node (bits 0-5)
                                             // and of the column node (6-11), contributions in the slot (12-21: up to
                                             // the 765 the plan accepts), bit 22 = diagonal slot; 0 for items that do
                                             // not own their slot
    int32_t max_stage_rows = 0;
    int32_t lds_bytes = 0;                   // dynamic LDS of k_assemble (assemble_lds_layout)
    int32_t lds_rec_off = 0, lds_stage_off = 0; // offsets in doubles (pipe: lds_rec_off = doubles of one record buffer)
    int32_t pipe = 0;                        // items laid out for k_assemble_pipe (Plan::pipe)
    int32_t slice_elem_ptr_last = 0;         // entries of slice_elem_nodes
    const uint8_t *dmask = nullptr;     // per local node (owned, padding, ghosts)
    double *vals = nullptr;             // total_slots x 36, sliced layout
    const float *vals32 = nullptr;      // the same in single precision (smoothing products of the multigrid cycle only)
    // ... and what such a product (symmetric storage) keeps in single precision besides: 1 = its results -- the direct part
    // y and the transposed products in tbuf, six floats where the FP64 product writes six doubles, in the same buffers --,
    // 2 = its input vector as well.  The arithmetic stays FP64.  k_cheb_start_node / k_cheb_step_node / k_sym_gather_node are told the
    // same number (amg_solve.cpp Cycle::smooth).
    int32_t vec32 = 0;
    const double *rhs_loads = nullptr;  // n_pad x 6 nodal loads and
    double *rhs_F = nullptr;            // the right-hand side k_assemble fills beside K (nullptr: K only)
    // symmetric storage (plan.hpp): transposed products K_ac^T x_a next to every slot, collected per row
    int32_t symmetric = 0;
    // ... and of a diagonal block (slot 0 of a row, symmetric itself) only the 12 of its 18 words that hold the upper
    // triangle are ever WRITTEN: word (jp, i) carries the columns 2jp, 2jp+1 of row i and lies below the diagonal when
    // 2jp+1 < i.  The assembly kernels skip those six stores (192 of 288 bytes per node reach HBM), the other six words of
    // the slot are never-written memory, and every reader of a diagonal slot takes (i, j), j < i, from (j, i): k_spmv_sym,
    // k_residual_dd_sym, k_block_jacobi, the multigrid setup's block loads, the exports.  K only (1 with symmetric storage
    // unless FEMSHELL_DIAG_UPPER=0); the level operators of the multigrid write whole blocks.
    int32_t diag_upper = 0;
    int32_t max_in_width = 0;
    const int32_t *in_width = nullptr;  // n_slices
    const int64_t *in_base = nullptr;   // n_slices+1
    const int32_t *in_slots = nullptr;  // per in-entry: slot index or -1
    const int32_t *in_rows = nullptr;   // per in-entry: local row of that block
    // products that stay inside a slice go through LDS in k_spmv_sym (plan.hpp); loc_index == nullptr: all through tbuf
    const int32_t *gat_slots = nullptr; // in_slots without the in-slice entries: what the collecting kernels walk
    const uint8_t *loc_index = nullptr; // per slot
    const uint8_t *loc_list = nullptr;  // per in-entry
    int32_t max_loc = 0;
    double *tbuf = nullptr;             // total_slots x 6: per (slice, slot k) [component j][node n]
    double *minv = nullptr;             // n_slices x 21 x 32: upper triangles of the inverse diagonal blocks
    const float *minv32 = nullptr;      // the same in single precision: the Chebyshev smoothers of the multigrid cycle read it
                                        // when set (amg_solve.cpp); the CG's own block-Jacobi step never does
    unsigned long long *stamps = nullptr; // profiling builds of k_assemble only (tools/lab)
    int32_t *status = nullptr;          // device int: 0 ok, e+1 = first degenerate local element,
                                        // -(node+1) = singular diagonal block
};

// Record i of a slice in a record buffer of k_assemble_pipe.  34 (66) doubles per record are 68 (132) dwords = 4 mod 64
// banks: records whose indices differ by 16 start in the same bank, and on a structured slice the lanes n and n + 8 of a wave
// read exactly such records (node n's elements sit at 2n + const in the slice's list) -- a four-way conflict per 32-lane
// group.  Two doubles of padding behind every 16 records move them four banks apart; the records stay 16-byte aligned.
// MEASURED (round 4, 4M-triangle panel, alternating libraries on one box): 0.550-0.552 ms with the padding against
// 0.543-0.552 ms without -- the conflicts the counters show (33 % of the LDS-active cycles) are not on the critical path.
// Off by default; -DFEMSHELL_PIPE_REC_PAD=2 builds the padded layout.
#ifndef FEMSHELL_PIPE_REC_PAD
#define FEMSHELL_PIPE_REC_PAD 0
#endif
constexpr int kPipeRecPad = FEMSHELL_PIPE_REC_PAD;
__host__ __device__ constexpr int pipe_rec_offset(int i, int rec_doubles) { return i * rec_doubles + kPipeRecPad * (i >> 4); }

// LDS layout of k_assemble for a plan with at most max_slice_elems element records and max_stage_rows partial-sum
// rows per slice: [records | partial sums].  Returns the dynamic LDS size in bytes.
inline size_t assemble_lds_layout(DeviceMatrix &m, int32_t max_slice_elems, int32_t max_stage_rows, bool has_quads,
                                  bool sections = false)
{
    if (m.pipe) { // k_assemble_pipe: two buffers of lean records, no staging
        // (+ two doubles of padding behind every 16 records: pipe_rec_offset)
        m.lds_rec_off = pipe_rec_offset(max_slice_elems, has_quads ? kRecDoublesQuad : (sections ? RecLeanSec::doubles : RecLean::doubles));
        m.lds_stage_off = 0;
        m.lds_bytes = (int32_t)(2 * (size_t)m.lds_rec_off * sizeof(double));
        return (size_t)m.lds_bytes;
    }
    const int rec = has_quads ? kRecDoublesQuad : kRecDoubles;
    m.lds_rec_off = 0;
    m.lds_stage_off = max_slice_elems * rec;
    m.lds_bytes = (int32_t)(((size_t)max_slice_elems * rec + (size_t)max_stage_rows * 36) * sizeof(double));
    return (size_t)m.lds_bytes;
}
// Scalars of the CG recurrence, resident in HBM (no host round trip per iteration).
struct CgScalars {
    double rz;     // r.z of the current iterate
    double alpha;
    double beta;
    double rr;     // r.r
    double bb;     // b.b
    double tol2;   // rtol^2 * b.b
    double red[3]; // local sums before / global sums after the all-reduce
    int32_t done;  // 0 running, 1 converged, -1 breakdown
    int32_t iters; // iterations performed
    uint32_t ticket;     // arrival counter of the two-stage reduction (0 between launches)
    uint32_t pad;
    double stage[3][64]; // stage-1 sums of the reduction workgroups
    // single-reduction recurrence with the scalar step folded into the update kernel (k_cgcg_update): every workgroup
    // derives alpha / beta from red[] and the previous (r.z, alpha); those are read from ring[parity] while workgroup 0
    // writes ring[parity ^ 1] and the fields above
    double ring_rz[2], ring_alpha[2];
    // a refinement pass of the multigrid-preconditioned solve (cg_amg): ||x||^2 of the iterate the pass corrects (uploaded by the
    // host in front of CG_PHASE_FLEX_RESTART; 0: no adaptive stopping), ||rhs||^2 of the pass, the tolerance of the solve
    double pass_xx, pass_rhs_rr, pass_rtol;
};

struct CgVectors {
    double *x = nullptr;  // solution, n_pad*6
    double *r = nullptr;  // residual
    double *z = nullptr;  // preconditioned residual
    double *p = nullptr;  // search direction, (n_pad+n_ghost)*6 (ghost part filled by the halo exchange)
    double *q = nullptr;  // A p (single-reduction recurrence: w = A z)
    double *sv = nullptr; // single-reduction recurrence only: s = A p by recurrence
    const double *b = nullptr; // right-hand side
    double *partials = nullptr; // 2 x grid doubles
    CgScalars *s = nullptr;
    double *hist = nullptr; // r.r / b.b per iteration
    int32_t hist_cap = 0;
};

enum CgPhase : int {
    CG_PHASE_NONE = 0, CG_PHASE_INIT = 1, CG_PHASE_ALPHA = 2, CG_PHASE_BETA = 3, CG_PHASE_RESTART = 4,
    CG_PHASE_FUSED_INIT = 5, CG_PHASE_FUSED_STEP = 6, // single-reduction (Chronopoulos-Gear) recurrence
    // flexible PCG around a general preconditioner (multigrid cycle, amg_solve.cpp):
    CG_PHASE_FLEX_INIT = 7, // red[0] = b.b
    CG_PHASE_FLEX_RZ0 = 8,  // red[0] = r.z of the initial residual
    CG_PHASE_FLEX_CONV = 9, // red[0] = r.r after the update: iteration count, history, stopping test
    CG_PHASE_FLEX_BETA = 10, // red[0] = r.z, red[1] = z.q: beta = z.(r - r_old) / rz_old = -alpha z.q / rz_old
    CG_PHASE_FLEX_RESTART = 11, // red[0] = r.r of the right-hand side of a refinement pass (the double-double residual
                                // of the accumulated solution); tolerance, iteration count and history carry on
    CG_PHASE_FLEX_WARM = 12     // a solve from an initial guess: red[0] = r.r of b - K x0 (double-double), the first phase solves the
                                // correction equation down to the threshold CG_PHASE_FLEX_INIT derived from b
};

int slice_grid(const DeviceMatrix &m); // workgroups of the per-slice kernels (8 * ceil(n_slices / 8), capped by FEMSHELL_SLICE_GRID through grid_cap of plan.hpp: a multiple of 8, at least 8, 65536 by default)

// sections != nullptr: a context with shell sections (m.lds_* laid out for the sectioned records: assemble_lds_layout)
// returns false, having launched nothing, when `sections` is given without its table or indices
bool launch_assemble(const DeviceMatrix &m, const MatConst &mc, hipStream_t st, const DeviceSections *sections = nullptr);
void launch_rhs(const DeviceMatrix &m, const double *loads /* n_pad x 6 */, double *F, hipStream_t st);
// fills m.item_flags from cols / dmask / pair_ptr (after every change of the Dirichlet set)
void launch_item_flags(const DeviceMatrix &m, int64_t n_items, hipStream_t st);
void launch_block_jacobi(const DeviceMatrix &m, hipStream_t st);
// agree[0] = 1 if *status > 0 (degenerate element), agree[1] = 1 if *status < 0 (singular diagonal block): the counters the
// ranks of a row partition sum up after an assembly / block-Jacobi setup
void launch_status_flags(const int32_t *status, double *agree, hipStream_t st);
void launch_element_matrices(const DeviceMatrix &m, const MatConst &mc, int32_t first, int32_t count,
                             double *Ke_out, hipStream_t st, const DeviceSections *sections = nullptr);

// Matrix-free product with the UNCONSTRAINED stiffness (element_product.hip), from the slices' element lists and the element
// routines of shell_element.hpp: y = sum_e K_e (x + xp)_e - sub on the owned rows, zero on padding rows; xp (a second input, added to
// x entry by entry) and sub may be nullptr.  rhs: y = mask(sub - sum_e K_e (x + xp)_e) instead, zero on the fixed dofs -- the
// right-hand side of prescribed displacements.  x and xp hold n_pad + n_ghost nodes, sub and y n_pad.  No atomics, the additions
// of a row in the order of its slice's element list: two launches give the same bits.  A degenerate element reports through
// m.status as in launch_assemble.
void launch_element_product(const DeviceMatrix &m, const MatConst &mc, const DeviceSections *sections, const double *x, const double *xp,
                            const double *sub, double *y, bool rhs, hipStream_t st);

// Element stress resultants and surface stresses (element_resultants.hip): out[(n_ltri + n_lquad)][14] in the LOCAL
// element order (triangles, then quadrilaterals) -- membrane force tensor, moment tensor (global axes, xx yy zz xy yz zx) and the von
// Mises stress at the top and the bottom surface, the element means by the element's own quadrature -- from u + up (each
// (n_pad + n_ghost) x 6; up may be nullptr).  sec_t: the thickness of every section where `sections` is given (its table keeps
// products only), nullptr otherwise.  One lane per element, no atomics: two launches give the same bits.  A degenerate element
// writes zeros and reports kStatusDirect + its index through m.status.
// thermal != nullptr: temperatures are in force: N_loc = t Dm (eps - eps0), M_loc = -Dp (kappa - kappa0) with the
// element's (Tm, Tg) and alpha -- the kThermal instantiations of the kernel; nullptr launches the instantiations without.
struct ThermalView;
void launch_element_resultants(const DeviceMatrix &m, const MatConst &mc, const DeviceSections *sections, const double *sec_t, const double *u,
                               const double *up, double *out, hipStream_t st, const ThermalView *thermal = nullptr);

// Thermal loads (element_thermal.hip).  What the kernels take from a material and its expansion coefficient: the
// factors of the equivalent loads, N_T = nt Tm and M_T = mt Tg, and of the free state, eps0 = alpha Tm, kappa0 = -alpha_t Tg.
// 32 bytes: each kernel reads its half of a row as one 16-byte word.
struct ThermalSec {
    double nt;      // E t alpha / (1 - nu)
    double mt;      // E t^2 alpha / (12 (1 - nu))
    double alpha;
    double alpha_t; // alpha / t
};
struct ThermalView {
    const double2 *elem_temp = nullptr; // (Tm, Tg) per LOCAL element (triangles, then quadrilaterals)
    ThermalSec uni{};                   // the context's uniform material
    const ThermalSec *sec = nullptr;    // per section, or nullptr: uni for every element
};
// out[n_pad][6] = base + T on all six components of the owned rows, zero on padding rows; base == nullptr: zero.  T_a: the
// work-equivalent nodal loads of the free thermal state of the elements that contain row a, added in the order of the slice's
// list from zero, no atomics: two launches give the same bits at every grid size.  slice_elem_local as for launch_element_loads;
// slice_elem_section: the section of every entry of the lists where tv.sec is given.  base may not be out.
void launch_element_thermal(const DeviceMatrix &m, const int32_t *slice_elem_local, const int32_t *slice_elem_section, const ThermalView &tv,
                            const double *base, double *out, hipStream_t st);

// Nodal equivalents of per-element pressure and traction (element_loads.hip): out[n_pad][6] = base + S on the
// translations of the owned rows, base on their rotations, zero on padding rows; base == nullptr: zero.  elem_load: four doubles
// (p, qx, qy, qz) per LOCAL element (triangles, then quadrilaterals), 16-byte aligned; slice_elem_local: the local element of
// every entry of the slices' element lists (Plan::slice_elems).  S_a: the shares of the elements that contain row a, added in
// the order of the slice's list from zero, no atomics: two launches give the same bits at every grid size.  base may not be out.
void launch_element_loads(const DeviceMatrix &m, const int32_t *slice_elem_local, const double *elem_load, const double *base, double *out,
                          hipStream_t st);

// Elastic supports (elastic_support.hip).  The support table: nine doubles per row of the slices (n_slices * 32
// rows) -- the tensor sum of the element foundations, xx yy zz xy yz zx, with the translational springs added to its first three
// words, then the three rotational springs; zeros on padding rows.
// launch_support_rows: elem_found, (kn, kt) per LOCAL element (triangles, then quadrilaterals), 16-byte aligned, or nullptr: no
// foundation (the lists are not walked); spring[n_pad][6] in global axes, or nullptr: no springs.  The additions of a row run in
// the order of its slice's list from zero, no atomics: two launches give the same bits at every grid size.  slice_elem_local as
// for launch_element_loads.
void launch_support_rows(const DeviceMatrix &m, const int32_t *slice_elem_local, const double *elem_found, const double *spring, double *table,
                         hipStream_t st);
// vals(diagonal slot of row a)(i, j) += K_sup(i, j) where neither dof i nor dof j of the node is fixed, one addition per entry
// and image: behind the assembly kernel, in front of launch_mass_shift
void launch_support_add(const DeviceMatrix &m, const double *table, hipStream_t st);
// y[n_pad][6] = base + s K_sup (x + xp) on the owned rows (not masked), zero on padding rows; xp and base may be nullptr
void launch_support_apply(const DeviceMatrix &m, const double *table, const double *x, const double *xp, const double *base, double s,
                          double *y, hipStream_t st);
// the table as two node vectors: lo[n_pad][6] = words 0-5, hi[n_pad][6] = words 6-8 and three zeros
void launch_support_words(const DeviceMatrix &m, const double *table, double *lo, double *hi, hipStream_t st);

// Nodal stress recovery and the Zienkiewicz-Zhu indicator (nodal_recovery.hip).  res: the rows launch_element_resultants
// left, (n_ltri + n_lquad) x 14 in the LOCAL element order.
// launch_nodal_recovery: nodes[n_slices * 32][14] = per owned row the area-weighted averages N* (words 0-5) and M* (6-11) of the
// elements that contain it, W = sum A_e (12) and the fold measure 1 - |sum a_e| / W (13); zeros on padding rows and where W = 0.
// The additions of a row run in the order of its slice's list from zero, no atomics: two launches give the same bits at every
// grid size.  slice_elem_local as for launch_element_loads.
void launch_nodal_recovery(const DeviceMatrix &m, const int32_t *slice_elem_local, const double *res, double *nodes, hipStream_t st);
// what k_recovery_error takes from a material: the factors of the complementary energy.  32 bytes: two 16-byte loads per section.
struct RecoveryMat {
    double cn;  // 1 / (E t)
    double cm;  // 12 / (E t^3)
    double nu;
    double pad;
};
// out[(n_ltri + n_lquad)][2], LOCAL element order: e2 = A_e c(sigma_e, sigma_e) and eta^2 = A_e sum_ij w_ij c(d_i, d_j), d_i the
// difference of the recovered field at corner i and the element's own value.  sec_mat / elem_section: a RecoveryMat per section and
// the section of every local element, or nullptr twice: `mat` for every element.  One lane per element, no sums across lanes.
void launch_recovery_error(const DeviceMatrix &m, const RecoveryMat &mat, const RecoveryMat *sec_mat, const int32_t *elem_section,
                           const double *res, const double *nodes, double *out, hipStream_t st);

// Load combinations (envelope.hip).
// launch_case_resultants: table[n_cases][6][n_ltri + n_lquad] = per case and LOCAL element (Nxx, Nyy, Nxy, Mxx, Myy, Mxy) in the
// element frame, N_loc = t Dm (eps(u_j) - tau_j eps0), M_loc = -Dp (kappa(u_j) - tau_j kappa0), from the columns u + j * ld (each
// (n_pad + n_ghost) x 6).  thermal != nullptr: the instantiations that read case_tau[n_cases] (HBM) and the element temperatures;
// nullptr: tau = 0 for every case, case_tau is not looked at.  A case's words do not depend on the other cases or on its index.
// A degenerate element writes zeros and reports kStatusDirect + its index through m.status.
// launch_envelope: per LOCAL element env[6] = (max q0, max q1, max q2, min q3, max q4, min q5) over the n_combos rows
// sum_j factors[c][j] table[j] (summed in index order) and gov[6] = the lowest c that attains each; elem_section / sec_t: the
// section of every local element and the thickness of every section, or nullptr twice: mc.t.  gov holds 6 (n_ltri + n_lquad) + 2
// int32: the last wave stores whole 16-byte words.  One lane per element, no atomics: two launches give the same bits.
constexpr int kEnvCombosPerPass = 4; // combinations k_envelope forms from one reading of the table
void launch_case_resultants(const DeviceMatrix &m, const MatConst &mc, const DeviceSections *sections, const ThermalView *thermal, const double *u,
                            int64_t ld, int n_cases, const double *case_tau, double *table, hipStream_t st);
void launch_envelope(const DeviceMatrix &m, const MatConst &mc, const int32_t *elem_section, const double *sec_t, const double *table, int n_cases,
                     const double *factors, int n_combos, double *env, int32_t *gov, hipStream_t st);

// ---- sparse products (spmv_kernels.hip) ----
// What a product does with its result besides storing it: what the callers fill and what k_spmv receives.
struct SpmvEpilogue {
    // y = base_vec + sign * K x (nullptr: y = K x): residuals b - K x and prolongations x + P x_c of the multigrid cycle; on full
    // storage base_vec may be y itself
    const double *base_vec = nullptr;
    double sign = 1.0;
    // full storage only -- one Chebyshev step of the smoother in D^-1 A fused with its product (multigrid levels that are bound by
    // the latency between launches), x the direction d_in, base_vec the residual r_in with sign -1, y the new residual r_out:
    // d_out = a d_in + c D^-1 r_out; xsol += d_out.  d_out must not be x (other workgroups still read it); y may be base_vec.
    // start != 0: the FIRST step of a smoothing instead, x the vector the residual is taken of: d_out = c D^-1 r_out (c = 1 / theta);
    // xsol += d_out -- or xsol = d_out from a zero guess (start == 2)
    double *d_out = nullptr, *xsol = nullptr;
    double a = 0.0, c = 0.0;
    int start = 0;
    // full storage only: the product itself, K x without the base vector, is stored as well -- as floats in that buffer when
    // prod_float (the coarse correction P x_c, which the cycle adds to its iterate and then multiplies with the level operator)
    double *prod_out = nullptr;
    int prod_float = 0;
};
// the slices a launch works on: order[begin, begin + count) -- the interior / boundary halves of a product whose halo exchange runs
// beside the interior half -- or, by default (count < 0), all of them in their own order.  A span of count 0 launches nothing.
struct SpmvSpan {
    const int32_t *order = nullptr;
    int begin = 0, count = -1;
    bool all() const { return count < 0; }
};
// y = K x with epilogue e; partials != nullptr: also partials[wg] = sum over the workgroup's rows of x * (K x), the p.Ap of CG.
// (s != nullptr: no-op once s->done != 0.)  K may be rectangular (x indexed by the block columns, y and base_vec by the block rows).
// Over all slices: symmetric storage runs both phases (launch_spmv_sym_phase1 + launch_sym_gather); full-storage operators with
// narrow rows (FEMSHELL_SPMV_NODE_WIDTH) that come with a base vector or a kept product go through k_spmv_node; k_spmv otherwise.
// Over a span: full storage only, k_spmv.  Returns the number of partial sums a launch with partials writes (0: nothing launched,
// or k_spmv_node, which writes none); -1, having launched nothing, for a Chebyshev step or a kept product on symmetric storage,
// whose second phase has no such epilogue.
int launch_spmv(const DeviceMatrix &m, const double *x, double *y, const SpmvEpilogue &e, const CgScalars *s, hipStream_t st,
                const SpmvSpan &span = SpmvSpan(), double *partials = nullptr);
// symmetric storage: first phase of y = K x only (direct part of y, transposed products into m.tbuf, fused x.Kx sums).  The caller
// runs launch_sym_gather once every span is through, or a kernel that collects the transposed products itself (k_cg_update_node<true>,
// k_cheb_step_node<true, *>, ...).  single_precision_values: a smoothing product of the multigrid cycle on m.vals32, storing what
// m.vec32 says in single precision.  Returns the number of partial sums written.
int launch_spmv_sym_phase1(const DeviceMatrix &m, const double *x, double *y, double *partials, const CgScalars *s, hipStream_t st,
                           const SpmvSpan &span = SpmvSpan(), bool single_precision_values = false);
// symmetric storage: second phase of a product whose transposed products are all in place:
// y = base_vec + sign * (y + sum of the row's transposed products)
// (q32: y and the transposed products come from a smoothing product that stored them in single precision -- DeviceMatrix::vec32 --
//  and the result goes to `out`, FP64, which may be base_vec)
void launch_sym_gather(const DeviceMatrix &m, double *y, const double *base_vec, double sign, const CgScalars *s, hipStream_t st,
                       bool q32 = false, double *out = nullptr);
// r = b - K x with double-double products and row sums (accurate residual for the residual replacement; r != x)
void launch_residual_dd(const DeviceMatrix &m, const double *x, const double *b, double *r, hipStream_t st);
// dst = (float)src
void launch_to_f32(const double *src, float *dst, int64_t n, hipStream_t st);

// ---- conjugate gradients (cg_kernels.hip) ----
// CG steps; every kernel is a no-op once s->done != 0
// restart = false: x=0, r=b;  restart = true: x kept, r = b - q (q = K x computed by the caller);
// then z = M^-1 r, p = z, partial sums of r.z and (b.b | r.r)
void launch_cg_init(const DeviceMatrix &m, const CgVectors &v, bool restart, hipStream_t st);
// p[owned rows] = x (to run q = K x through the SpMV kernel, whose input carries the ghost entries)
void launch_copy_x_to_p(const DeviceMatrix &m, const CgVectors &v, hipStream_t st);
// x += alpha p, r -= alpha q, z = M^-1 r + partial sums of r.z, r.r.  gather (symmetric storage): v.q holds the direct part of
// K p only (launch_spmv_sym_phase1); the kernel adds the transposed products of each row's in-list itself
void launch_cg_update(const DeviceMatrix &m, const CgVectors &v, hipStream_t st, bool gather = false);

void launch_cg_direction(const DeviceMatrix &m, const CgVectors &v, hipStream_t st); // p = z + beta p
// single-workgroup scalar step: optional reduction of `nsums` partial arrays into s->red, then the
// scalar update of `phase` (rtol only used by CG_PHASE_INIT)
// (n_partials > 0: length of each partial array, default slice_grid(m); nsums == 3: the third array, the SpMV's,
// starts at 2 * n_partials and holds len3 entries)
// gate_phase >= 0: the phase whose skip rule applies (the reduce-only launch in front of an all-reduce runs phase
// NONE on behalf of another phase; INIT / RESTART steps must also run on a finished solve)
void launch_cg_scalar(const DeviceMatrix &m, const CgVectors &v, bool reduce, int nsums, CgPhase phase,
                      double rtol, hipStream_t st, int n_partials = 0, int len3 = 0, int gate_phase = -1);

// Single-reduction preconditioned CG (Chronopoulos & Gear): one all-reduce of (r.z, r.r, z.Az) per iteration.
//   init:   x = 0, r = b, z = M^-1 r, p = s = 0, partial sums of r.z and r.r
//   update: p = z + beta p, s = w + beta s, x += alpha p, r -= alpha s, z = M^-1 r, partial sums of r.z and r.r
// with w = A z (v.q) from the SpMV kernel, whose fused dot is z.w
void launch_cgcg_init(const DeviceMatrix &m, const CgVectors &v, hipStream_t st);
// step >= 0: the kernel first performs the scalar step that closes the previous iteration (red[] holds its global sums;
// reads ring[step & 1], writes ring[(step & 1) ^ 1]); gather: q holds the direct part of a symmetric product only, the
// rows add the transposed products of their in-lists
void launch_cgcg_update(const DeviceMatrix &m, const CgVectors &v, hipStream_t st, int step = -1, bool gather = false);

// ---- structural dynamics (dynamics_kernels.hip; femshell_dynamics_*): lumped mass and the vector kernels of a Newmark step.  One lane per node, 48
// bytes per node and vector, no LDS, no barriers; every kernel is row-local (owned rows of the rank).
struct NewmarkCoef {
    double a0, a1, a2, a3, a4, a5; // include/femshell.h
    double alpha, dt, gamma;
    double shift;                  // a0 + alpha a1: K_eff = K + shift M on the free dofs
};
// mass[n_pad][6]: the diagonal of the lumped mass matrix of the owned rows (0 on the padding rows).  rho_t = {rho t, rho t^3/12} of
// the uniform material; sec_mass != nullptr: one such pair per section, the element's index from slice_elem_section (where the
// sectioned assembly kernels take it)
void launch_lumped_mass(const DeviceMatrix &m, double2 rho_t, const double2 *sec_mass, const int32_t *slice_elem_section, double *mass,
                        hipStream_t st);
// vals(diagonal slot of row a)(i, i) += shift * mass[a][i] on the free dofs of the owned rows (both storages: the diagonal block is
// slot 0 of its row and its diagonal words belong to the upper triangle)
void launch_mass_shift(const DeviceMatrix &m, const double *mass, double shift, hipStream_t st);
// begin: u = mask(u0), v = mask(v0) (nullptr: 0), a = mask((F - alpha M v - Ku) / M) with Ku = K u0 (nullptr: 0)
void launch_newmark_init(const DeviceMatrix &m, const double *mass, const double *F, const double *Ku, const double *u0, const double *v0,
                         double alpha, double *u, double *v, double *a, hipStream_t st);
// b = mask(F + M [(a0 u + a2 v + a3 a) + alpha (a1 u + a4 v + a5 a)]): the dynamic sibling of k_rhs (F is its output)
void launch_newmark_rhs(const DeviceMatrix &m, const NewmarkCoef &k, const double *mass, const double *F, const double *u, const double *v,
                        const double *a, double *b, hipStream_t st);
// candidate state from the solve's x: u' = mask(x), a' = a0 (u' - u) - a2 v - a3 a, v' = v + dt [(1 - gamma) a + gamma a']
void launch_newmark_update(const DeviceMatrix &m, const NewmarkCoef &k, const double *x, const double *u, const double *v, const double *a,
                           double *u1, double *v1, double *a1, hipStream_t st);
constexpr int kEnergyGrid = 256; // workgroups (= partial sums per quantity) of launch_newmark_energy
// partials[3][kEnergyGrid]: per workgroup the sums of v.Mv, u.q (q = K_eff u) and u.Mu over its stretch of the owned rows, then
// out3[j] = the partials of quantity j added in index order by one lane (fixed order: the result is reproducible)
void launch_newmark_energy(const DeviceMatrix &m, const double *mass, const double *u, const double *v, const double *q, double *partials,
                           double *out3, hipStream_t st);

// halo: gather owned entries of p into a contiguous send buffer (width doubles per node: 6 for the vectors of the solve;
// the multigrid setup of row-partitioned contexts sends rows of 1, 36 and more doubles the same way)
void launch_pack(const double *p, const int32_t *send_nodes, int32_t count, double *sendbuf, hipStream_t st, int width = 6);

} // namespace femshell
